"""ops.json_guide (csrc/kernels/json_guide.hip) against tests/json_guide_reference.py on the same bf16 rows: BIT
equality — a barred entry is 0xFF80, an allowed one keeps its bits, so there is no tolerance to choose. The case
(json_guide_reference.build_case) holds a seeded byte table with tokens of 0..40 bytes, rich in JSON punctuation and
shorter than the vocabulary, and the start configurations of json_guide_reference.STARTS: inside keys, escapes and
multi-byte characters, inside numbers, after values, DONE, the sink, and the depths 1, 31 and 32 with tokens that
push or pop more than once. One row of five is at slot -1. Corrupted tables are launched too: the kernel must
reject them by its checks (GUIDE_ERR_TABLE, nothing written), every index it forms stays in bounds."""

import functools

import numpy as np
import pytest
import torch

from src import ops

from tests import json_guide_reference as oracle
from tests.test_json_guide_reference_cpu import corruptions

pytestmark = pytest.mark.gpu

DEV = "cuda"
VOCABS = (1024, 8200, 128256)   # 8200: 257 bitmap words, so the table's LDS copy sits behind padding and the
                                # dense pass ends in a partial word
TABLE_KEYS = ("desc", "trans", "tok_off", "tok_bytes")


@functools.lru_cache(maxsize=None)
def case(vocab: int):
    return oracle.build_case(vocab)


def as_bits(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def launch(vocab, rows, stride, with_advance, with_lm, row_slot=None, advance=None, bits=None, **over):
    c = case(vocab)
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = (c["bits"] if bits is None else bits)[:rows]
    logits = torch.from_numpy(buf.view(np.int16)).view(torch.bfloat16).to(DEV)
    desc, trans, tok_off, tok_bytes = (dev(over.get(k, c[k])) for k in TABLE_KEYS)
    cur, jstk = dev(over.get("cur", c["cur"])), dev(over.get("jstk", c["jstk"]))
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32, device=DEV)
    lm = dev(oracle.start_lm(rows).view(np.int32)) if with_lm else None
    if row_slot is None:
        row_slot = (oracle.ROW_SLOT_ADV if with_advance else oracle.ROW_SLOT_PLAIN)[:rows]
    slot = torch.tensor(row_slot, dtype=torch.int32, device=DEV)
    adv = None
    if with_advance:
        adv = dev(c["advance"][:rows] if advance is None else advance)
    ops.json_guide(logits[:, :vocab], slot, desc, trans, tok_off, tok_bytes, cur, jstk, err, advance_ids=adv,
                   lm_part=lm)
    torch.cuda.synchronize()
    return logits, cur, jstk, err, lm, (slot, desc, trans, tok_off, tok_bytes)


@pytest.mark.parametrize("with_lm", [False, True], ids=["no_lm_part", "lm_part"])
@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
@pytest.mark.parametrize("pad", [0, 8], ids=["stride_eq_vocab", "stride_gt_vocab"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("vocab", VOCABS)
def test_rows_state_and_candidates_match_the_oracle_bit_for_bit(vocab, rows, pad, with_advance, with_lm):
    want, w_cur, w_jstk, w_err, w_lm = oracle.run_oracle(case(vocab), rows, vocab + pad, with_advance, with_lm)
    logits, cur, jstk, err, lm, tabs = launch(vocab, rows, vocab + pad, with_advance, with_lm)
    got = as_bits(logits)
    for r in range(rows):
        bad = np.nonzero(got[r] != want[r])[0]
        assert bad.size == 0, (r, bad[:5].tolist())
    assert np.array_equal(cur.cpu().numpy(), w_cur) and np.array_equal(jstk.cpu().numpy(), w_jstk)
    assert np.array_equal(err.cpu().numpy(), w_err)
    if with_lm:
        assert np.array_equal(lm.cpu().numpy().view(np.uint32), w_lm)
    if rows == 5:
        assert np.array_equal(got[1, :vocab], case(vocab)["bits"][1])    # slot -1: byte-identical before and after
        assert int(w_err.sum()) == (ops.GUIDE_ERR_NO_EDGE if with_advance else 0)
        # a second launch on the masked rows, without an advance, changes nothing
        c2, j2, e2 = cur.clone(), jstk.clone(), err.clone()
        lm2 = lm.clone() if with_lm else None
        slot, desc, trans, tok_off, tok_bytes = tabs
        ops.json_guide(logits[:, :vocab], slot, desc, trans, tok_off, tok_bytes, c2, j2, e2, lm_part=lm2)
        torch.cuda.synchronize()
        assert np.array_equal(as_bits(logits), got)
        assert torch.equal(c2, cur) and torch.equal(j2, jstk) and torch.equal(e2, err)
        assert lm2 is None or torch.equal(lm2, lm)


def test_every_start_configuration():
    vocab, n = 1024, oracle.SLOTS
    c = case(vocab)
    rng = np.random.default_rng(3)
    bits = (rng.integers(-3, 5, size=(n, vocab)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    slots = tuple(range(n))
    want, w_cur, w_jstk, w_err, w_lm = oracle.run_oracle(c, n, vocab, False, True, row_slot=slots, bits=bits)
    logits, cur, jstk, err, lm, _ = launch(vocab, n, vocab, False, True, row_slot=slots, bits=bits)
    got = as_bits(logits)
    for r in range(n):
        bad = np.nonzero(got[r] != want[r])[0]
        assert bad.size == 0, (oracle.STARTS[r][0], bad[:5].tolist())
    assert np.array_equal(lm.cpu().numpy().view(np.uint32), w_lm)
    assert np.array_equal(cur.cpu().numpy(), c["cur"]) and np.array_equal(jstk.cpu().numpy(), c["jstk"])
    assert not err.cpu().numpy().any()
    allowed = got[:, :vocab] != oracle.NINF_BF16
    tok = lambda name, t: bool(allowed[oracle.SLOT[name], t])
    bid = oracle.byte_id
    for name in ("depth32_value", "depth32_array_value"):     # the cap: pushing tokens barred, '"' and digits allowed
        assert not tok(name, bid("{")) and not tok(name, bid("[")) and not tok(name, oracle.ID_KEY)
        assert tok(name, bid('"')) and all(tok(name, bid(d)) for d in "0123456789")
    assert tok("depth31_value", bid("[")) and tok("depth31_value", oracle.ID_KEY)      # one push
    assert not tok("depth31_value", oracle.ID_ARR2) and not tok("depth31_value", oracle.ID_ARR_OBJ)   # two
    assert tok("depth1_number", bid("}")) and not tok("depth1_number", oracle.ID_CLOSE2)
    assert not any(tok("after_zero", bid(d)) for d in "0123456789")
    assert tok("in_string_in_object_in_array", oracle.ID_POP_PUSH)


def test_every_kind_of_advance():
    vocab = 1024
    c = case(vocab)
    kinds = oracle.ADVANCE_KINDS + (("in_key", vocab - 3, False, oracle.ERR_NO_EDGE),)    # an id beyond the table
    for name, tok, _, want_err in kinds:
        s = oracle.SLOT[name]
        adv = np.array([tok], dtype=np.int64)
        want, w_cur, w_jstk, w_err, _ = oracle.run_oracle(c, 1, vocab, True, False, row_slot=(s,), advance=adv)
        assert int(w_err[s]) == want_err, (name, tok)
        logits, cur, jstk, err, _, _ = launch(vocab, 1, vocab, True, False, row_slot=(s,), advance=adv)
        assert np.array_equal(as_bits(logits), want), (name, tok)
        assert np.array_equal(cur.cpu().numpy(), w_cur) and np.array_equal(jstk.cpu().numpy(), w_jstk), (name, tok)
        assert np.array_equal(err.cpu().numpy(), w_err), (name, tok)


def test_every_out_of_bounds_value_is_a_table_error_and_nothing_is_touched():
    vocab = 1024
    c = case(vocab)
    s, kinds = corruptions(c)
    for name, over in kinds:
        over = dict(over)
        row_slot = over.pop("row_slot", (s,))
        adv = over.pop("advance", None)
        logits, cur, jstk, err, lm, _ = launch(vocab, 1, vocab, adv is not None, True, row_slot=row_slot,
                                               advance=adv, **over)
        err = err.cpu().numpy()
        assert int(err[row_slot[0]]) == ops.GUIDE_ERR_TABLE and int(err.sum()) == ops.GUIDE_ERR_TABLE, name
        assert np.array_equal(as_bits(logits)[0], c["bits"][0]), name
        assert np.array_equal(cur.cpu().numpy(), over.get("cur", c["cur"])), name
        assert np.array_equal(jstk.cpu().numpy(), over.get("jstk", c["jstk"])), name
        assert np.array_equal(lm.cpu().numpy().view(np.uint32), oracle.start_lm(1)), name


@pytest.mark.parametrize("vocab", VOCABS)
def test_candidates_make_the_sampler_return_the_best_allowed_token(vocab):
    want, _, _, _, w_lm = oracle.run_oracle(case(vocab), 5, vocab, True, True)
    logits, _, _, _, lm, _ = launch(vocab, 5, vocab, True, True)
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
    desc, trans, tok_off, tok_bytes = (dev(c[k]) for k in TABLE_KEYS)
    logits = torch.from_numpy(c["bits"].view(np.int16).copy()).view(torch.bfloat16).to(DEV)
    slot = torch.tensor(oracle.ROW_SLOT_PLAIN, dtype=torch.int32, device=DEV)
    cur, jstk = dev(c["cur"]), dev(c["jstk"])
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32, device=DEV)
    bad = "HIP launch failed"
    i16, u8, i32 = torch.int16, torch.uint8, torch.int32
    with pytest.raises(RuntimeError, match=bad):                  # vocab % 8 != 0
        ops.json_guide(logits[:, :vocab - 4], slot, desc, trans, tok_off, tok_bytes, cur, jstk, err)
    with pytest.raises(RuntimeError, match="row stride must be a multiple of 8"):
        wide = torch.zeros(5, vocab + 4, dtype=torch.bfloat16, device=DEV)
        ops.json_guide(wide[:, :vocab], slot, desc, trans, tok_off, tok_bytes, cur, jstk, err)
    with pytest.raises(RuntimeError, match=bad):                  # a stride below the vocabulary
        ops.json_guide(logits.as_strided((5, vocab), (vocab - 8, 1)), slot, desc, trans, tok_off, tok_bytes, cur,
                       jstk, err)
    with pytest.raises(RuntimeError, match=bad):                  # no slot table (a null descriptor pointer)
        ops.json_guide(logits, slot, torch.empty(0, 4, dtype=i32, device=DEV), trans, tok_off, tok_bytes, cur, jstk,
                       err)
    with pytest.raises(RuntimeError, match=bad):                  # a null table
        ops.json_guide(logits, slot, desc, torch.empty(0, 256, dtype=i16, device=DEV), tok_off, tok_bytes, cur, jstk,
                       err)
    with pytest.raises(RuntimeError, match=bad):                  # a table above GUIDE_JSON_MAX_STATES
        big = torch.full((ops.GUIDE_JSON_MAX_STATES + 1, 256), -1, dtype=i16, device=DEV)
        ops.json_guide(logits, slot, desc, big, tok_off, tok_bytes, cur, jstk, err)
    with pytest.raises(RuntimeError, match=bad):                  # a table that is not 16-byte aligned
        odd = torch.full((trans.shape[0] + 1, 256), -1, dtype=i16, device=DEV).view(-1)[4:4 + trans.numel()]
        ops.json_guide(logits, slot, desc, odd.view(-1, 256), tok_off, tok_bytes, cur, jstk, err)
    with pytest.raises(RuntimeError, match=bad):                  # a null byte table
        ops.json_guide(logits, slot, desc, trans, tok_off, torch.empty(0, dtype=u8, device=DEV), cur, jstk, err)
    with pytest.raises(RuntimeError, match=bad):                  # a byte table below the kernel's 8-byte fetch
        ops.json_guide(logits, slot, desc, trans, tok_off, torch.zeros(7, dtype=u8, device=DEV), cur, jstk, err)
    with pytest.raises(RuntimeError, match=bad):                  # an offset table without a token
        ops.json_guide(logits, slot, desc, trans, torch.zeros(1, dtype=i32, device=DEV), tok_bytes, cur, jstk, err)
    with pytest.raises(RuntimeError, match=bad):                  # a bitmap above 48 KiB: vocab > 393,216
        huge = torch.zeros(1, 393216 + 8, dtype=torch.bfloat16, device=DEV)
        ops.json_guide(huge, slot, desc, trans, tok_off, tok_bytes, cur, jstk, err)
    torch.cuda.synchronize()
    assert np.array_equal(as_bits(logits), c["bits"])             # nothing ran
    assert np.array_equal(cur.cpu().numpy(), c["cur"]) and np.array_equal(jstk.cpu().numpy(), c["jstk"])
    assert int(err.sum()) == 0
