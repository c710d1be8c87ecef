"""ops.schema_guide (csrc/kernels/schema_guide.hip) against tests/schema_guide_reference.py on the same bf16 rows: BIT
equality — a barred entry is 0xFF80, an allowed one keeps its bits, so there is no tolerance to choose. The case
(schema_guide_reference.build_case) holds two compiled guides at different bases of one arena, a seeded byte table
with tokens of 0..40 bytes (four and five live pushes, pops below the start depth followed by pushes), shorter than
the vocabulary, and the start configurations of schema_guide_reference.STARTS: depths 0, 1, 31 and 32, inside a frame
and inside an inlined container, an accepting state at depth 0 and at depth 1, the sink. One row of five is at slot
-1. Corrupted tables are launched too: the kernel must reject them by its checks (GUIDE_ERR_TABLE, nothing written);
every corrupt value lies inside the allocations, so a missed check is a mismatch, never a stray access."""

import numpy as np
import pytest
import torch

from src import ops

from tests import schema_guide_reference as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
VOCABS = (1024, 8200, 128256)   # 8200: 257 bitmap words, the dense pass ends in a partial word
PAD_STATES = 8   # the arenas are views of larger allocations: a region "beyond the arena" still lies in memory


def as_bits(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def padded(a, fill):
    full = np.full((len(a) + PAD_STATES,) + a.shape[1:], fill, dtype=a.dtype)
    full[:len(a)] = a
    return dev(full)[:len(a)]


def launch(vocab, rows, stride, with_advance, with_lm, row_slot=None, advance=None, **over):
    c = oracle.build_case(vocab)
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = c["bits"][:rows]
    logits = torch.from_numpy(buf.view(np.int16)).view(torch.bfloat16).to(DEV)
    get = lambda k: over.get(k, c[k])
    trans, accept = padded(get("trans"), -1), padded(get("accept"), 0)
    desc, tok_off, tok_bytes = dev(get("desc")), dev(get("tok_off")), dev(get("tok_bytes"))
    cur, sdep, sstk = dev(get("cur")), dev(get("sdep")), dev(get("sstk"))
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32, device=DEV)
    lm = dev(oracle.start_lm(rows).view(np.int32)) if with_lm else None
    if row_slot is None:
        row_slot = (oracle.ROW_SLOT_ADV if with_advance else oracle.ROW_SLOT_PLAIN)[:rows]
    slot = torch.tensor(row_slot, dtype=torch.int32, device=DEV)
    adv = None
    if with_advance:
        adv = dev(c["advance"][:rows] if advance is None else advance)
    args = (slot, desc, trans, accept, tok_off, tok_bytes, cur, sdep, sstk, err)
    ops.schema_guide(logits[:, :vocab], *args, advance_ids=adv, lm_part=lm)
    torch.cuda.synchronize()
    return logits, cur, sdep, sstk, err, lm, args


def check(got, want, rows, with_lm):
    logits, cur, sdep, sstk, err, lm = got[:6]
    w_bits, w_cur, w_sdep, w_sstk, w_err, w_lm = want
    bits = as_bits(logits)
    for r in range(rows):
        bad = np.nonzero(bits[r] != w_bits[r])[0]
        assert bad.size == 0, (r, bad[:5].tolist())
    assert np.array_equal(cur.cpu().numpy(), w_cur)
    assert oracle.live_equal(sdep.cpu().numpy(), sstk.cpu().numpy(), w_sdep, w_sstk)
    assert np.array_equal(err.cpu().numpy(), w_err)
    if with_lm:
        assert np.array_equal(lm.cpu().numpy().view(np.uint32), w_lm)
    return bits


@pytest.mark.parametrize("with_lm", [False, True], ids=["no_lm_part", "lm_part"])
@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
@pytest.mark.parametrize("pad", [0, 8], ids=["stride_eq_vocab", "stride_gt_vocab"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("vocab", VOCABS)
def test_rows_configuration_and_candidates_match_the_oracle_bit_for_bit(vocab, rows, pad, with_advance, with_lm):
    c = oracle.build_case(vocab)
    want = oracle.run_oracle(c, rows, vocab + pad, with_advance, with_lm)
    got = launch(vocab, rows, vocab + pad, with_advance, with_lm)
    bits = check(got, want, rows, with_lm)
    if rows == 5:
        assert np.array_equal(bits[1, :vocab], c["bits"][1])    # slot -1: byte-identical before and after
        assert int(want[4].sum()) == (ops.GUIDE_ERR_NO_EDGE if with_advance else 0)
        # a second launch on the masked rows, without an advance, changes nothing
        logits, cur, sdep, sstk, err, lm, (slot, desc, trans, accept, tok_off, tok_bytes, *_rest) = got
        before = (bits.copy(), cur.cpu().numpy().copy(), sdep.cpu().numpy().copy(), sstk.cpu().numpy().copy())
        ops.schema_guide(logits[:, :vocab], slot, desc, trans, accept, tok_off, tok_bytes, cur, sdep, sstk, err)
        torch.cuda.synchronize()
        assert np.array_equal(as_bits(logits), before[0]) and np.array_equal(cur.cpu().numpy(), before[1])
        assert np.array_equal(sdep.cpu().numpy(), before[2]) and np.array_equal(sstk.cpu().numpy(), before[3])


@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
def test_every_start_configuration(with_advance):
    """All of STARTS, the sink and the accepting state at depth 1, five rows at a time; with an advance every row
    takes a token chosen for its configuration (pops, pushes written back, EOS, a token without an edge)."""
    vocab = 1024
    c = oracle.build_case(vocab)
    tid, eos = c["tid"], c["eos"]
    adv_of = {0: tid[b"{"], 1: tid[b"}"], 2: tid[b"n"], 3: tid[b"}"], 4: tid[b"[[[["], 5: tid[b"["], 6: tid[b"]]],[[["],
              7: eos, 8: tid[b"}"], 9: tid[b"]"], 10: tid[b"{"], 11: tid[b"\x98"], oracle.SLOT_SINK: eos,
              oracle.SLOT_ACCEPT_DEEP: eos}
    slots = oracle.ALL_SLOTS
    flags = 0
    for at in range(0, len(slots), 5):
        rs = slots[at:at + 5]
        adv = np.array([adv_of[s] for s in rs], dtype=np.int64)
        want = oracle.run_oracle(c, len(rs), vocab, with_advance, True, row_slot=rs, advance=adv)
        got = launch(vocab, len(rs), vocab, with_advance, True, row_slot=rs, advance=adv)
        check(got, want, len(rs), True)
        flags += int((want[4] != 0).sum())
    if with_advance:
        # '[[[[' at depth 31, '[' at depth 32 and EOS at depth 1 have no edge; everything else advances
        assert flags == 3
    else:
        w = oracle.run_oracle(c, 2, vocab, False, False, row_slot=(oracle.SLOT_ACCEPT_DEEP, 7))[0]
        assert w[0, eos] == 0xFF80 and w[1, eos] == c["bits"][1, eos]   # EOS barred at depth 1, allowed at depth 0


@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
def test_corrupted_tables_report_a_table_error_and_write_nothing(with_advance):
    vocab = 1024
    c = oracle.build_case(vocab)
    tid = c["tid"]
    for name, over, slots in oracle.corruptions(c):
        adv = np.array([tid[b'"'] if s else tid[b"{"] for s in slots], dtype=np.int64)
        bad = dict(c, **over)
        want = oracle.run_oracle(bad, len(slots), vocab, with_advance, True, row_slot=slots, advance=adv)
        assert all(want[4][s] == ops.GUIDE_ERR_TABLE for s in slots), name
        got = launch(vocab, len(slots), vocab, with_advance, True, row_slot=slots, advance=adv, **over)
        check(got, want, len(slots), True)
        assert np.array_equal(as_bits(got[0])[:, :vocab], c["bits"][:len(slots)]), name     # rows untouched
        assert np.array_equal(got[3].cpu().numpy(), bad["sstk"]), name                      # and the whole stack
