"""ops.token_guide (csrc/kernels/token_guide.hip) against tests/token_guide_reference.py on the same bf16 rows: BIT
equality — a barred entry is 0xFF80, an allowed one keeps its bits, so there is no tolerance to choose. The case
(token_guide_reference.build_case) masks rows by 1 edge, ids {0, vocab - 1}, 1025 edges and the whole vocabulary,
with and without an advance (one advance finds no edge), maps rows to permuted slots of a region that does not
start at the arenas' origin, and leaves one row at slot -1. Corrupted tables are compared on the CPU only
(tests/test_guided_cpu.py): nothing here launches one."""

import functools

import numpy as np
import pytest
import torch

from src import ops

from tests import token_guide_reference as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
VOCABS = (1024, 8200, 32000, 128256)


@functools.lru_cache(maxsize=None)
def case(vocab: int):
    return oracle.build_case(vocab)


@functools.lru_cache(maxsize=None)
def tables(vocab: int):
    """The case's tables on the device (read-only for the kernel: shared by the tests)."""
    c = case(vocab)
    return tuple(torch.from_numpy(c[k].copy()).to(DEV) for k in ("desc", "rowptr", "edges"))


def as_bits(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def launch(vocab, rows, stride, with_advance, with_lm):
    c = case(vocab)
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = c["bits"][:rows]
    logits = torch.from_numpy(buf.view(np.int16)).view(torch.bfloat16).to(DEV)
    cur = torch.from_numpy(c["cur"].copy()).to(DEV)
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32, device=DEV)
    lm = torch.from_numpy(oracle.start_lm(rows).view(np.int32).copy()).to(DEV) if with_lm else None
    slot = torch.tensor(oracle.ROW_SLOT[:rows], dtype=torch.int32, device=DEV)
    ops.token_guide(logits[:, :vocab], slot, *tables(vocab), cur, err,
                    advance_ids=torch.from_numpy(c["advance"][:rows]).to(DEV) if with_advance else None, lm_part=lm)
    torch.cuda.synchronize()
    return logits, cur, err, lm


@pytest.mark.parametrize("with_lm", [False, True], ids=["no_lm_part", "lm_part"])
@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
@pytest.mark.parametrize("pad", [0, 8], ids=["stride_eq_vocab", "stride_gt_vocab"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("vocab", VOCABS)
def test_rows_state_and_candidates_match_the_oracle_bit_for_bit(vocab, rows, pad, with_advance, with_lm):
    want, w_cur, w_err, w_lm = oracle.run_oracle(case(vocab), rows, vocab + pad, with_advance, with_lm)
    logits, cur, err, lm = launch(vocab, rows, vocab + pad, with_advance, with_lm)
    got = as_bits(logits)
    for r in range(rows):
        bad = np.nonzero(got[r] != want[r])[0]
        assert bad.size == 0, (r, bad[:5].tolist())
    assert np.array_equal(cur.cpu().numpy(), w_cur) and np.array_equal(err.cpu().numpy(), w_err)
    if with_lm:
        assert np.array_equal(lm.cpu().numpy().view(np.uint32), w_lm)
    if rows == 5:
        assert np.array_equal(got[1, :vocab], case(vocab)["bits"][1])    # slot -1: byte-identical before and after
        assert w_err[2] == (ops.GUIDE_ERR_NO_EDGE if with_advance else 0) and not w_err[[0, 3, 6]].any()


@pytest.mark.parametrize("vocab", [1024, 128256])
def test_candidates_make_the_sampler_return_the_best_allowed_token(vocab):
    want, _, _, w_lm = oracle.run_oracle(case(vocab), 5, vocab, True, True)
    logits, _, _, lm = launch(vocab, 5, vocab, True, True)
    # rows 0, 2, 3, 4 only: row 1 (slot -1) keeps start_lm's made-up candidates, which name no real maximum
    keep = [0, 2, 3, 4]
    out = ops.sample(logits[keep], lm_part=lm[keep].contiguous()).cpu().tolist()
    assert out == [int(w_lm[r, 0, 1]) for r in keep]
    vals = oracle.bf16_value(want[:, :vocab])
    clean = torch.from_numpy(np.nan_to_num(vals[keep], nan=-np.inf)).to(torch.bfloat16).to(DEV)   # row 3 holds a NaN
    assert ops.sample(clean).cpu().tolist() == out               # the sampler's own pass over the masked rows


def test_the_sampler_draws_only_allowed_ids():
    vocab, seeds = 32000, 256
    c = case(vocab)
    allowed = [0, vocab - 1]                                      # state 1
    row = torch.from_numpy(c["bits"][2:3].view(np.int16).copy()).view(torch.bfloat16)
    row[0, 0], row[0, vocab - 1] = 1.0, 1.5                      # p = 0.38 / 0.62: both are drawn in 256 seeds
    logits = row.repeat(seeds, 1).to(DEV)
    slot = torch.zeros(seeds, dtype=torch.int32, device=DEV)      # every row reads slot 0 (state 1, no advance:
    cur = torch.from_numpy(c["cur"].copy()).to(DEV)               # nothing writes but equal values)
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32, device=DEV)
    ops.token_guide(logits, slot, *tables(vocab), cur, err)
    f = torch.float32
    out = ops.sample(logits, torch.full((seeds,), 1.0, dtype=f, device=DEV), torch.zeros(seeds, dtype=torch.int32, device=DEV),
                     torch.ones(seeds, dtype=f, device=DEV), torch.arange(seeds, dtype=torch.int64, device=DEV),
                     torch.zeros(seeds, dtype=torch.int64, device=DEV)).cpu().tolist()
    assert set(out) <= set(allowed) and len(set(out)) == 2, sorted(set(out))
    assert int(err.sum()) == 0
    # the logprobs of a masked row: two finite values that sum to 1, three -inf, valid ids
    lp, rank, top_lp, top_id = ops.token_logprobs(logits[:4], torch.tensor(out[:4], device=DEV), 5)
    top_lp, top_id = top_lp.cpu(), top_id.cpu()
    for r in range(4):
        assert sorted(top_id[r, :2].tolist()) == allowed and torch.isfinite(top_lp[r, :2]).all()
        assert torch.isneginf(top_lp[r, 2:]).all()
        assert ((top_id[r] >= 0) & (top_id[r] < vocab)).all() and len(set(top_id[r].tolist())) == 5
        # each logprob is z - max - lse over values below 2 in magnitude: every fp32 rounding there is at most
        # 2^-23, and the chain has at most 8 of them, the fast exponentials and the logarithm counted at 2 ulp each;
        # d exp(lp) / d lp <= 1, so the two probabilities sum to 1 within 16 * 2^-23 ~ 1.9e-6
        total = float(top_lp[r, :2].double().exp().sum())
        print(f"row {r}: logprobs {top_lp[r, :2].tolist()}, sum of probabilities - 1 = {total - 1.0:.3e}")
        assert abs(total - 1.0) <= 16 * 2.0 ** -23
        assert torch.isfinite(lp[r].cpu()) and int(rank[r]) in (0, 1)


def test_launcher_rejects_bad_arguments():
    vocab = 1024
    c = case(vocab)
    desc, rowptr, edges = tables(vocab)
    logits = torch.from_numpy(c["bits"].view(np.int16).copy()).view(torch.bfloat16).to(DEV)
    slot = torch.tensor(oracle.ROW_SLOT, dtype=torch.int32, device=DEV)
    cur = torch.from_numpy(c["cur"].copy()).to(DEV)
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32, device=DEV)
    bad = "HIP launch failed"
    with pytest.raises(RuntimeError, match=bad):                  # vocab % 8 != 0
        ops.token_guide(logits[:, :vocab - 4], slot, desc, rowptr, edges, cur, err)
    # a row stride that breaks the 16-B groups: the launcher refuses it too, the binding's row check comes first
    with pytest.raises(RuntimeError, match="row stride must be a multiple of 8"):
        wide = torch.zeros(5, vocab + 4, dtype=torch.bfloat16, device=DEV)
        ops.token_guide(wide[:, :vocab], slot, desc, rowptr, edges, cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # no slot table (a null descriptor pointer)
        ops.token_guide(logits, slot, torch.empty(0, 4, dtype=torch.int32, device=DEV), rowptr, edges, cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # no edges (a null arena)
        ops.token_guide(logits, slot, desc, rowptr, torch.empty(0, 2, dtype=torch.int32, device=DEV), cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # an arena above GUIDE_ROWPTR_ARENA
        big = torch.zeros(ops.GUIDE_ROWPTR_ARENA + 1, dtype=torch.int32, device=DEV)
        ops.token_guide(logits, slot, desc, big, edges, cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # a bitmap above 48 KiB: vocab > 393,216
        huge = torch.zeros(1, 393216 + 8, dtype=torch.bfloat16, device=DEV)
        ops.token_guide(huge, slot, desc, rowptr, edges, cur, err)
    torch.cuda.synchronize()
    assert np.array_equal(as_bits(logits), c["bits"])             # nothing ran
    assert np.array_equal(cur.cpu().numpy(), c["cur"]) and int(err.sum()) == 0
