"""ops.byte_guide (csrc/kernels/byte_guide.hip) against tests/byte_guide_reference.py on the same bf16 rows: BIT
equality — a barred entry is 0xFF80, an allowed one keeps its bits, so there is no tolerance to choose. The case
(byte_guide_reference.build_case) holds two guides in one arena, one on each side of the kernel's LDS boundary
(6 and 300 states against GUIDE_BYTE_LDS_STATES); tokens of 1, 2, 16, exactly GUIDE_MAX_TOKEN_BYTES and one byte
more, and tokens without bytes; a table shorter than the vocabulary; a state that allows nothing but EOS, one that
allows the full vocabulary, and the sink; EOS from an accepting and from a non-accepting state (GUIDE_ERR_NO_EDGE);
one row at slot -1. Corrupted tables are compared on the CPU only (tests/test_byte_guide_reference_cpu.py): nothing
here launches one."""

import functools

import numpy as np
import pytest
import torch

from src import ops

from tests import byte_guide_reference as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
VOCABS = (1024, 8200, 128256)
TABLE_KEYS = ("desc", "trans", "accept", "tok_off", "tok_bytes")


@functools.lru_cache(maxsize=None)
def case(vocab: int):
    return oracle.build_case(vocab)


@functools.lru_cache(maxsize=None)
def tables(vocab: int):
    """The case's tables on the device (read-only for the kernel: shared by the tests)."""
    c = case(vocab)
    return tuple(torch.from_numpy(c[k].copy()).to(DEV) for k in TABLE_KEYS)


def as_bits(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def launch(vocab, rows, stride, with_advance, with_lm, cur=None, advance=None):
    c = case(vocab)
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = c["bits"][:rows]
    logits = torch.from_numpy(buf.view(np.int16)).view(torch.bfloat16).to(DEV)
    cur = torch.from_numpy((c["cur_adv" if with_advance else "cur_plain"] if cur is None else cur).copy()).to(DEV)
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32, device=DEV)
    lm = torch.from_numpy(oracle.start_lm(rows).view(np.int32).copy()).to(DEV) if with_lm else None
    slot = torch.tensor(oracle.ROW_SLOT[:rows], dtype=torch.int32, device=DEV)
    adv = c["advance"][:rows] if advance is None else advance
    ops.byte_guide(logits[:, :vocab], slot, *tables(vocab), cur, err,
                   advance_ids=torch.from_numpy(adv.copy()).to(DEV) if with_advance else None, lm_part=lm)
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
        # a second launch on the masked rows, without an advance, changes nothing
        c2, e2 = cur.clone(), err.clone()
        lm2 = lm.clone() if with_lm else None
        slot = torch.tensor(oracle.ROW_SLOT, dtype=torch.int32, device=DEV)
        ops.byte_guide(logits[:, :vocab], slot, *tables(vocab), c2, e2, lm_part=lm2)
        torch.cuda.synchronize()
        assert np.array_equal(as_bits(logits), got)
        assert torch.equal(c2, cur) and torch.equal(e2, err) and (lm2 is None or torch.equal(lm2, lm))


def test_every_kind_of_advance():
    vocab = 1024
    c = case(vocab)
    kinds = oracle.ADVANCE_KINDS + ((0, vocab - 3, 0, oracle.ERR_NO_EDGE),)    # an id beyond the table
    for start, tok, want_state, want_err in kinds:
        cur = c["cur_plain"].copy()
        cur[3] = start
        adv = np.array([tok], dtype=np.int64)
        buf = c["bits"][:1].copy()
        o_cur, o_err = cur.copy(), np.zeros(oracle.SLOTS, dtype=np.int32)
        oracle.byte_guide(buf, oracle.ROW_SLOT[:1], c["desc"], c["trans"], c["accept"], c["tok_off"], c["tok_bytes"],
                          o_cur, o_err, vocab, advance=adv)
        assert (int(o_cur[3]), int(o_err[3])) == (want_state, want_err), (start, tok)
        logits, g_cur, g_err, _ = launch(vocab, 1, vocab, True, False, cur=cur, advance=adv)
        assert np.array_equal(as_bits(logits), buf), (start, tok)
        assert np.array_equal(g_cur.cpu().numpy(), o_cur) and np.array_equal(g_err.cpu().numpy(), o_err), (start, tok)


@pytest.mark.parametrize("vocab", [1024, 128256])
def test_candidates_make_the_sampler_return_the_best_allowed_token(vocab):
    want, _, _, w_lm = oracle.run_oracle(case(vocab), 5, vocab, True, True)
    logits, _, _, lm = launch(vocab, 5, vocab, True, True)
    # rows 0, 2, 3, 4 only: row 1 (slot -1) keeps start_lm's made-up candidates, which name no real maximum
    keep = [0, 2, 3, 4]
    out = ops.sample(logits[keep], lm_part=lm[keep].contiguous()).cpu().tolist()
    assert out == [int(w_lm[r, 0, 1]) for r in keep]
    assert out[1] == oracle.EOS                                   # the sink: nothing but EOS
    vals = oracle.bf16_value(want[:, :vocab])
    clean = torch.from_numpy(np.nan_to_num(vals[keep], nan=-np.inf)).to(torch.bfloat16).to(DEV)   # row 3 holds a NaN
    assert ops.sample(clean).cpu().tolist() == out               # the sampler's own pass over the masked rows


def test_launcher_rejects_bad_arguments():
    vocab = 1024
    c = case(vocab)
    desc, trans, accept, tok_off, tok_bytes = tables(vocab)
    logits = torch.from_numpy(c["bits"].view(np.int16).copy()).view(torch.bfloat16).to(DEV)
    slot = torch.tensor(oracle.ROW_SLOT, dtype=torch.int32, device=DEV)
    cur = torch.from_numpy(c["cur_plain"].copy()).to(DEV)
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32, device=DEV)
    bad = "HIP launch failed"
    i16, u8, i32 = torch.int16, torch.uint8, torch.int32
    with pytest.raises(RuntimeError, match=bad):                  # vocab % 8 != 0
        ops.byte_guide(logits[:, :vocab - 4], slot, desc, trans, accept, tok_off, tok_bytes, cur, err)
    with pytest.raises(RuntimeError, match="row stride must be a multiple of 8"):
        wide = torch.zeros(5, vocab + 4, dtype=torch.bfloat16, device=DEV)
        ops.byte_guide(wide[:, :vocab], slot, desc, trans, accept, tok_off, tok_bytes, cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # a stride below the vocabulary
        ops.byte_guide(logits.as_strided((5, vocab), (vocab - 8, 1)), slot, desc, trans, accept, tok_off, tok_bytes,
                       cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # no slot table (a null descriptor pointer)
        ops.byte_guide(logits, slot, torch.empty(0, 4, dtype=i32, device=DEV), trans, accept, tok_off, tok_bytes, cur,
                       err)
    with pytest.raises(RuntimeError, match=bad):                  # a null trans arena
        ops.byte_guide(logits, slot, desc, torch.empty(0, 256, dtype=i16, device=DEV), accept, tok_off, tok_bytes, cur,
                       err)
    with pytest.raises(RuntimeError, match=bad):                  # a null byte table
        ops.byte_guide(logits, slot, desc, trans, accept, tok_off, torch.empty(0, dtype=u8, device=DEV), cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # a byte table below the kernel's 8-byte fetch
        ops.byte_guide(logits, slot, desc, trans, accept, tok_off, torch.zeros(7, dtype=u8, device=DEV), cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # an offset table without a token
        ops.byte_guide(logits, slot, desc, trans, accept, torch.zeros(1, dtype=i32, device=DEV), tok_bytes, cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # an accept arena above GUIDE_BYTE_STATE_ARENA
        big = torch.zeros(ops.GUIDE_BYTE_STATE_ARENA + 1, dtype=u8, device=DEV)
        ops.byte_guide(logits, slot, desc, trans, big, tok_off, tok_bytes, cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # a trans arena above it
        big = torch.zeros(ops.GUIDE_BYTE_STATE_ARENA + 1, 256, dtype=i16, device=DEV)
        ops.byte_guide(logits, slot, desc, big, accept, tok_off, tok_bytes, cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # a byte table above GUIDE_TOK_BYTES_MAX
        big = torch.zeros(ops.GUIDE_TOK_BYTES_MAX + 1, dtype=u8, device=DEV)
        ops.byte_guide(logits, slot, desc, trans, accept, tok_off, big, cur, err)
    with pytest.raises(RuntimeError, match=bad):                  # a bitmap above 48 KiB: vocab > 393,216
        huge = torch.zeros(1, 393216 + 8, dtype=torch.bfloat16, device=DEV)
        ops.byte_guide(huge, slot, desc, trans, accept, tok_off, tok_bytes, cur, err)
    torch.cuda.synchronize()
    assert np.array_equal(as_bits(logits), c["bits"])             # nothing ran
    assert np.array_equal(cur.cpu().numpy(), c["cur_plain"]) and int(err.sum()) == 0
