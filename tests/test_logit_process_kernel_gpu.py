"""ops.logit_process (csrc/kernels/logit_process.hip) against tests/logit_process_reference.py on the same bf16
rows: BIT equality — the contract is a fixed sequence of individually rounded fp32 operations, so there is no
tolerance to choose. Integer-valued rows make ties; the state holds prompt bits and counts 0, 1, small, 32766 and
32767; the bias lists have 0, 1 and 300 entries and name ids 0 and vocab - 1; rows map to permuted slots and one
row has slot -1.

The named cases of tests/logit_process_reference.py follow (tests/test_logit_process_reference_cpu.py proves their
premises): the `rounding` rows, found by a seeded search, on which an FMA contraction, a folded epilogue, float64
arithmetic, a division or a misplaced bias or penalty each change >= 8 bf16 outputs; the bias-table families (probe
chains, the wrap from slot 1023 to 0, all eight ids of a group, stray list entries, counts outside [0, cap], bias
-inf) at vocab 8 .. 393,216; tied processed maxima across threads, waves and sweeps for the candidates."""

import functools

import numpy as np
import pytest
import torch

from src import ops

from tests import logit_process_reference as lpr
from tests.logit_process_reference import COUNT_MAX, inv_f32, logit_process

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOTS = 7
ROW_SLOT = (3, -1, 0, 6, 2)                      # row r -> slot; row 1 is not processed
PARAMS = {3: (1.3, 0.7, 0.3), 0: (2.0, -0.25, 1.1), 6: (0.5, 1.5, -2.0), 2: (1.0, 0.0, 0.0)}  # rp, freq, pres
BIAS_N = {3: 300, 0: 1, 6: 0, 2: 1}
PARTS = 5
VOCABS = (1016, 128256)                          # 1016: no multiple of the 8192-entry sweep, a ragged last pass


@functools.lru_cache(maxsize=None)
def case(vocab: int):
    """Inputs on the CPU and the oracle's rows for count_ids given / null: computed once per vocabulary."""
    g = torch.Generator().manual_seed(vocab)
    rows = len(ROW_SLOT)
    x = torch.randint(-3, 4, (rows, vocab), generator=g).to(torch.bfloat16)
    prompt = torch.rand(SLOTS, vocab, generator=g) < 0.3
    counts = torch.zeros(SLOTS, vocab, dtype=torch.int64)
    pick = torch.rand(SLOTS, vocab, generator=g)
    counts[pick < 0.30] = 1
    counts[pick < 0.15] = 3
    counts[pick < 0.05] = COUNT_MAX - 1
    counts[pick < 0.03] = COUNT_MAX
    bias_cnt = torch.zeros(SLOTS, dtype=torch.int32)
    bias_ids = torch.zeros(SLOTS, ops.LOGIT_BIAS_MAX, dtype=torch.int32)
    bias_vals = torch.zeros(SLOTS, ops.LOGIT_BIAS_MAX, dtype=torch.float32)
    for s, n in BIAS_N.items():
        ids = torch.randperm(vocab - 2, generator=g)[:max(n - 2, 0)] + 1
        ids = torch.cat([torch.tensor([vocab - 1]), ids, torch.tensor([0])])[:n] if n else ids[:0]
        if s == 2:
            ids = torch.tensor([0])              # the two one-entry lists: vocab - 1 (slot 0) and 0 (slot 2)
        bias_cnt[s] = n
        bias_ids[s, :n] = ids.int()
        bias_vals[s, :n] = (torch.rand(n, generator=g) * 200 - 100).round()   # integers in [-100, 100]: ties stay
        bias_ids[s, n:] = 5                      # beyond the count: must be ignored
        bias_vals[s, n:] = 77.0
    params = torch.zeros(SLOTS, 4)
    for s, (rp, freq, pres) in PARAMS.items():
        params[s] = torch.tensor([rp, inv_f32(rp), freq, pres])
    # this step's input ids: a saturated entry, (row 1: unused), a biased id, a count-0 entry, a 32766 entry
    cid = torch.zeros(rows, dtype=torch.int64)
    cid[0] = int((counts[3] == COUNT_MAX).nonzero()[0, 0])
    cid[1] = 1
    cid[2] = vocab - 1
    cid[3] = int(((counts[6] == 0) & ~prompt[6]).nonzero()[0, 0])
    cid[4] = int((counts[2] == COUNT_MAX - 1).nonzero()[0, 0])
    want = {}
    for counted in (True, False):
        c = counts.clone()
        outs = x.clone()
        for r, s in enumerate(ROW_SLOT):
            if s < 0:
                continue
            if counted:
                c[s, cid[r]] = min(int(c[s, cid[r]]) + 1, COUNT_MAX)
            b = torch.zeros(vocab)
            n = int(bias_cnt[s])
            b[bias_ids[s, :n].long()] = bias_vals[s, :n]
            rp, inv, freq, pres = (float(v) for v in params[s])
            outs[r] = logit_process(x[r], prompt[s], c[s], rp, inv, freq, pres, b)
        want[counted] = (outs, c)
    return x, prompt, counts, params, bias_cnt, bias_ids, bias_vals, cid, want


def pack_state(prompt, counts):
    """uint16 entries (bit 15: in the prompt, bits 0-14: count) as the int16 tensor the op takes."""
    v = counts + prompt.long() * 32768
    return torch.where(v >= 32768, v - 65536, v).to(torch.int16)


def bits(t):
    return t.contiguous().view(torch.int16)


def strided(x, stride):
    buf = torch.full((x.shape[0], stride), 1000.0, dtype=torch.bfloat16)
    buf[:, :x.shape[1]] = x
    return buf.to(DEV)


@pytest.mark.parametrize("counted", [True, False], ids=["count_ids", "no_count_ids"])
@pytest.mark.parametrize("vocab", VOCABS)
def test_rows_and_state_match_the_oracle_bit_for_bit(vocab, counted):
    x, prompt, counts, params, bcnt, bids, bvals, cid, want = case(vocab)
    w_rows, w_counts = want[counted]
    buf = strided(x, vocab + 8)
    state = pack_state(prompt, counts).to(DEV)
    slot = torch.tensor(ROW_SLOT, dtype=torch.int32, device=DEV)
    ops.logit_process(buf[:, :vocab], slot, state, params.to(DEV), bcnt.to(DEV), bids.to(DEV), bvals.to(DEV),
                      count_ids=cid.to(DEV) if counted else None)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(bits(got[:, vocab:]), bits(torch.full((len(ROW_SLOT), 8), 1000.0, dtype=torch.bfloat16)))
    for r in range(len(ROW_SLOT)):
        bad = (bits(got[r, :vocab]) != bits(w_rows[r])).nonzero()
        assert bad.numel() == 0, (r, bad[:5].tolist())
    assert torch.equal(bits(got[1, :vocab]), bits(x[1]))        # slot -1: the row's bytes are unchanged
    assert not torch.equal(bits(got[0, :vocab]), bits(x[0]))
    assert torch.equal(state.cpu(), pack_state(prompt, w_counts))
    if counted:   # the saturated entry stayed, 32766 became 32767, the prompt bit of a counted entry survived
        assert w_counts[3, cid[0]] == COUNT_MAX and w_counts[2, cid[4]] == COUNT_MAX
        assert w_counts[6, cid[3]] == 1 and counts[6, cid[3]] == 0


@pytest.mark.parametrize("vocab", VOCABS)
def test_candidates_make_the_sampler_return_the_processed_argmax(vocab):
    x, prompt, counts, params, bcnt, bids, bvals, cid, want = case(vocab)
    w_rows, w_counts = want[True]
    rows = len(ROW_SLOT)
    logits = x.to(DEV)
    state = pack_state(prompt, counts).to(DEV)
    # the candidates as the LM head leaves them: each row's raw (max, lowest index) in a LATER part, garbage-free
    lm = torch.empty(rows, PARTS, 2, dtype=torch.int32)
    lm[:, :, 0] = torch.tensor(float("-inf")).view(torch.int32)
    lm[:, :, 1] = 0x7fffffff
    raw = [int((x[r].float() == x[r].float().max()).nonzero()[0, 0]) for r in range(rows)]
    for r in range(rows):
        lm[r, 3, 0] = x[r].float().max().view(torch.int32)
        lm[r, 3, 1] = raw[r]
    lm = lm.to(DEV)
    slot = torch.tensor(ROW_SLOT, dtype=torch.int32, device=DEV)
    ops.logit_process(logits, slot, state, params.to(DEV), bcnt.to(DEV), bids.to(DEV), bvals.to(DEV),
                      count_ids=cid.to(DEV), lm_part=lm)
    out = ops.sample(logits, lm_part=lm).cpu().tolist()
    whole = ops.sample(logits).cpu().tolist()                   # the sampler's own pass over the rewritten rows
    wantmax = [int((w_rows[r].float() == w_rows[r].float().max()).nonzero()[0, 0]) for r in range(rows)]
    assert out == wantmax and whole == wantmax
    assert out[1] == raw[1]                                     # slot -1: the LM head's candidates were left alone
    assert any(out[r] != raw[r] for r in (0, 2, 3, 4))          # the processing moved an argmax
    got = lm.cpu()
    for r, s in enumerate(ROW_SLOT):
        if s >= 0:
            assert got[r, 0, 1] == wantmax[r] and torch.all(got[r, 1:, 1] == 0x7fffffff)
            assert got[r, 0, 0].view(torch.float32) == w_rows[r].float().max()
    assert torch.equal(state.cpu(), pack_state(prompt, w_counts))


def test_launcher_rejects_bad_arguments():
    vocab = VOCABS[0]
    x, prompt, counts, params, bcnt, bids, bvals, cid, _ = case(vocab)
    slot = torch.tensor(ROW_SLOT, dtype=torch.int32, device=DEV)
    state = pack_state(prompt, counts).to(DEV)
    args = (params.to(DEV), bcnt.to(DEV), bids.to(DEV), bvals.to(DEV))
    logits = x.to(DEV)
    with pytest.raises(RuntimeError, match="HIP launch failed"):            # vocab % 8 != 0
        ops.logit_process(logits[:, :vocab - 4], slot, state[:, :vocab - 4].contiguous(), *args)
    with pytest.raises(RuntimeError, match="HIP launch failed"):            # a bias list wider than 300
        wide_i = torch.zeros(SLOTS, ops.LOGIT_BIAS_MAX + 1, dtype=torch.int32, device=DEV)
        ops.logit_process(logits, slot, state, args[0], args[1], wide_i, wide_i.float())
    with pytest.raises(RuntimeError, match="HIP launch failed"):            # no state table
        ops.logit_process(logits, slot, torch.empty(0, dtype=torch.int16, device=DEV), *args)
    torch.cuda.synchronize()
    assert torch.equal(bits(logits.cpu()), bits(x))                         # nothing ran


# ------------------------------------------------------------------------------------------------- the named cases
GAP = 64
NEG_INF_I32 = int(torch.tensor(float("-inf")).view(torch.int32))


def bf16_of(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def u16(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def raw_candidates(c, parts):
    """The candidates as the LM head leaves them: each row's raw (max, lowest index) in the last part."""
    rows = c.x.shape[0]
    lm = torch.empty(rows, parts, 2, dtype=torch.int32)
    lm[:, :, 0], lm[:, :, 1] = NEG_INF_I32, lpr.NO_INDEX
    for r in range(rows):
        v = lpr.bits_f32(c.x[r])
        lm[r, parts - 1, 0] = int(np.float32(v.max()).view(np.int32))
        lm[r, parts - 1, 1] = int(np.flatnonzero(v == v.max())[0])
    return lm


def launch_named(c, counted, parts=0):
    """One launch from fresh copies: rows in a strided buffer with a loud gap. -> (buffer, state, candidates, view)."""
    v = c.vocab
    buf = strided(bf16_of(c.x), v + GAP)
    state = torch.from_numpy(c.state.view(np.int16).copy()).to(DEV)
    lm = raw_candidates(c, parts).to(DEV) if parts else None
    view = buf[:, :v]
    assert view.stride(0) == v + GAP
    ops.logit_process(view, torch.from_numpy(c.slot).to(DEV), state, torch.from_numpy(c.params).to(DEV),
                      torch.from_numpy(c.bias_cnt).to(DEV), torch.from_numpy(c.bias_ids).to(DEV),
                      torch.from_numpy(c.bias_vals).to(DEV),
                      count_ids=torch.from_numpy(c.count_ids).to(DEV) if counted else None, lm_part=lm)
    torch.cuda.synchronize()
    return buf, state, lm, view


def check_rows_and_state(c, buf, state, w_rows, w_state):
    got = u16(buf)
    v = c.vocab
    assert np.array_equal(got[:, v:], u16(torch.full((c.x.shape[0], GAP), 1000.0, dtype=torch.bfloat16)))
    for r in range(c.x.shape[0]):
        bad = np.flatnonzero(got[r, :v] != w_rows[r])
        assert bad.size == 0, (r, bad[:5].tolist(), got[r, bad[:5]].tolist(), w_rows[r, bad[:5]].tolist())
    assert torch.equal(state.cpu(), torch.from_numpy(w_state.view(np.int16)))


@pytest.mark.parametrize("counted", [True, False], ids=["count_ids", "no_count_ids"])
@pytest.mark.parametrize("name", lpr.ROWS_CASE_NAMES)
def test_named_case_rows_and_state_bit_for_bit(name, counted):
    c = lpr.rows_case(name)
    w_rows, w_state, _ = lpr.rows_expected(name, counted)
    buf, state, _, _ = launch_named(c, counted)
    check_rows_and_state(c, buf, state, w_rows, w_state)
    buf2, state2, _, _ = launch_named(c, counted)                 # again from fresh copies: bit-identical
    assert np.array_equal(u16(buf), u16(buf2)) and torch.equal(state.cpu(), state2.cpu())


@pytest.mark.parametrize("parts", [1, 5])
@pytest.mark.parametrize("name", lpr.ROWS_CASE_NAMES)
def test_named_case_candidates_and_the_sampler(name, parts):
    c = lpr.rows_case(name)
    w_rows, w_state, w_cand = lpr.rows_expected(name, True)
    buf, state, lm, view = launch_named(c, True, parts)
    check_rows_and_state(c, buf, state, w_rows, w_state)
    got = lm.cpu()
    raw = raw_candidates(c, parts)
    want_ids = []
    for r in range(c.x.shape[0]):
        if r in w_cand:       # candidate 0 holds the exact bits, the others (-inf, 0x7fffffff)
            assert int(got[r, 0, 0]) & 0xffffffff == w_cand[r][0] and int(got[r, 0, 1]) == w_cand[r][1]
            assert bool((got[r, 1:, 0] == NEG_INF_I32).all()) and bool((got[r, 1:, 1] == lpr.NO_INDEX).all())
            want_ids.append(w_cand[r][1])
        else:                 # an unprocessed row: the LM head's candidates were left alone
            assert torch.equal(got[r], raw[r])
            want_ids.append(int(raw[r, parts - 1, 1]))
    assert ops.sample(view, lm_part=lm).cpu().tolist() == want_ids
    assert ops.sample(view).cpu().tolist() == want_ids            # the sampler's own pass over the rewritten rows
    lm2 = launch_named(c, True, parts)[2]
    assert torch.equal(got, lm2.cpu())


def test_launcher_rejects_a_vocabulary_past_the_bitmap_s_share_of_lds():
    vocab = 393224
    logits = torch.full((1, vocab), 1.5, dtype=torch.bfloat16, device=DEV)
    state = torch.full((2, vocab), 3, dtype=torch.int16, device=DEV)
    z = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="HIP launch failed"):
        ops.logit_process(logits, torch.ones(1, dtype=torch.int32, device=DEV), state,
                          torch.ones(2, 4, device=DEV), z, torch.zeros(2, 300, dtype=torch.int32, device=DEV),
                          torch.ones(2, 300, device=DEV), count_ids=torch.zeros(1, dtype=torch.long, device=DEV))
    torch.cuda.synchronize()
    assert bool((logits == 1.5).all()) and bool((state == 3).all())           # nothing was written
