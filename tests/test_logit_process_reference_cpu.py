"""tests/logit_process_reference.py judged before logit_process_kernel is judged by it: the numpy oracle (float64
with an explicit fp32 rounding per step, the bf16 rounding written out) bit-identical to the torch-fp32 oracle and to
the engine's CPU path on every case; per case the premises of its families (probe chains from the table's hash, the
bitmap groups, stray entries, counts); every claimed mutant changing >= 8 elements of its row; the row mutants."""

import pathlib

import numpy as np
import pytest
import torch

from src.ops import reference as ref

from tests import logit_process_reference as lpr

NAMES = lpr.ROWS_CASE_NAMES
PARTS = 5


def bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def torch_impl(zbits, prompt, counts, rp, inv, freq, pres, bias):
    out = lpr.logit_process(bf16(zbits), torch.from_numpy(prompt), torch.from_numpy(counts), float(rp), float(inv),
                            float(freq), float(pres), None if bias is None else torch.from_numpy(bias))
    return out.view(torch.int16).numpy().view(np.uint16)


def test_hash_constants_are_the_kernel_s():
    src = (pathlib.Path(__file__).resolve().parents[1] / "csrc" / "kernels" / "logit_process.hip").read_text()
    assert f"(id * {lpr.LP_HASH_MULT}u) >> {lpr.LP_HASH_SHIFT}" in src
    assert f"constexpr int LP_HASH = {lpr.LP_HASH};" in src
    assert "LP_MAX_MAP_BYTES = 48 * 1024" in src and 393216 // 8 == 48 * 1024
    assert int(lpr.lp_hash([1])[0]) == 2654435761 >> 22 and int(lpr.lp_hash([3])[0]) == ((3 * 2654435761) % 2 ** 32) >> 22
    h, occ = lpr.slot_ids(8200)
    assert occ.max() == 9 and h.max() == 1023           # at 8200 ids a slot has up to 9 ids
    assert lpr.slot_ids(1016)[1].max() <= 2             # the small vocabulary makes no chain of any length


def test_rne_bf16_is_torch_s_rounding():
    rng = np.random.default_rng(1)
    x = np.concatenate([(rng.standard_normal(200000) * 50).astype(np.float32),
                        rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    x = x[~np.isnan(x)]
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(lpr.rne_bf16(x), want)
    ties = (np.arange(0x3f80, 0x3fa0, dtype=np.uint32) << 16 | 0x8000).view(np.float32)   # exact halves: to even
    assert np.array_equal(lpr.rne_bf16(ties), torch.from_numpy(ties).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


@pytest.mark.parametrize("counted", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_the_two_oracles_and_the_engine_path_agree_bit_for_bit(name, counted):
    c = lpr.rows_case(name)
    rows, state, cand = lpr.rows_expected(name, counted)
    t_rows, t_state, t_cand = lpr.rows_oracle(c, counted, impl=torch_impl)
    assert np.array_equal(rows, t_rows) and np.array_equal(state, t_state) and cand == t_cand
    # the engine's CPU path on the kernel's own arguments, stray entries and out-of-range counts included
    logits = bf16(c.x).clone()
    st = torch.from_numpy(c.state.view(np.int16).copy())
    lm = torch.zeros(c.x.shape[0], PARTS, 2, dtype=torch.int32)
    ref.logit_process_rows(logits, torch.from_numpy(c.slot), st, torch.from_numpy(c.params),
                           torch.from_numpy(c.bias_cnt), torch.from_numpy(c.bias_ids), torch.from_numpy(c.bias_vals),
                           torch.from_numpy(c.count_ids) if counted else None, lm)
    assert np.array_equal(logits.view(torch.int16).numpy().view(np.uint16), rows)
    assert np.array_equal(st.numpy().view(np.uint16), state)
    for r, (vbits, idx) in cand.items():
        assert int(lm[r, 0, 0]) & 0xffffffff == vbits and int(lm[r, 0, 1]) == idx
        assert bool((lm[r, 1:, 1] == lpr.NO_INDEX).all())


@pytest.mark.parametrize("name", NAMES)
def test_rows_and_state_premises(name):
    c = lpr.rows_case(name)
    rows, state, cand = lpr.rows_expected(name)
    ns, v = c.state.shape[0], c.vocab
    assert v % 8 == 0 and c.bias_ids.shape == (ns, lpr.CAP)
    live = [r for r in range(c.x.shape[0]) if 0 <= c.slot[r] < ns]
    slots = [int(c.slot[r]) for r in live]
    assert len(set(slots)) == len(slots)                                  # no two rows share a state
    if name != "cap_393216":
        assert -1 in c.slot.tolist() and ns in c.slot.tolist() and slots != sorted(slots)
    else:
        assert len(live) == 1 and ns == 2
    for r in range(c.x.shape[0]):
        if r not in live:
            assert np.array_equal(rows[r], c.x[r]) and r not in cand       # left untouched
        else:
            assert (rows[r] != c.x[r]).sum() >= min(v, 8) // 2
    # the state: only the counted entry changed
    changed = np.argwhere(state != c.state)
    want = set()
    for r in live:
        s, t = int(c.slot[r]), int(c.count_ids[r])
        if 0 <= t < v and (int(c.state[s, t]) & 0x7fff) < lpr.COUNT_MAX:
            want.add((s, t))
            assert int(state[s, t]) == int(c.state[s, t]) + 1 and (state[s, t] ^ c.state[s, t]) & 0x8000 == 0
    assert {tuple(x) for x in changed.tolist()} == want
    # the bias values are no integers (banned entries aside), the entries beyond the count are other values
    for s in range(ns):
        nb = min(max(int(c.bias_cnt[s]), 0), lpr.CAP)
        vals = c.bias_vals[s, :nb]
        assert np.all((vals != np.round(vals)) | np.isinf(vals))
        beyond = c.bias_ids[s, nb:]
        assert nb == lpr.CAP or ((beyond >= 0) & (beyond < v)).any()       # valid ids there: they must be ignored


def test_count_id_kinds_of_the_main_case():
    c = lpr.rows_case("main_8200")
    _, state, _ = lpr.rows_expected("main_8200")
    kinds = {}
    for r, s in enumerate(c.slot.tolist()):
        if not 0 <= s < c.state.shape[0]:
            continue
        t = int(c.count_ids[r])
        if t == -1 or t == c.vocab:
            kinds["outside" + str(t < 0)] = True
            continue
        before, after = int(c.state[s, t]), int(state[s, t])
        if before & 0x7fff == lpr.COUNT_MAX:
            kinds["saturated"] = after == before
        elif before & 0x7fff == lpr.COUNT_MAX - 1:
            kinds["c32766"] = after & 0x7fff == lpr.COUNT_MAX and after & 0x8000 == before & 0x8000
        elif before == 0x8000:
            kinds["prompt_only"] = after == 0x8001
        if lpr.bias_row(c, s) is not None and lpr.bias_row(c, s)[t] != 0:
            kinds["biased"] = after == before + 1
    assert kinds == {k: True for k in ("saturated", "c32766", "prompt_only", "biased", "outsideTrue", "outsideFalse")}


def test_bias_table_families():
    c = lpr.rows_case("main_8200")
    v = c.vocab
    fam = {f: s for s, fs in c.families.items() for f in fs}
    assert set(fam) >= {"rounding", "chain", "wrap", "group", "edges", "full", "stray", "banned", "tie", "last_max"}
    s = fam["chain"]
    ids = c.bias_ids[s, :c.bias_cnt[s]].astype(np.int64)
    h = lpr.lp_hash(ids).astype(np.int64)
    assert np.bincount(h, minlength=lpr.LP_HASH).max() >= 8                # >= 8 ids of one slot
    assert ((h >= 1021) & (h <= 1023)).sum() >= 12                          # more than slots 1021..1023 hold: wraps
    assert (h <= 1).sum() >= 4                                              # slots 0 and 1 are wanted by their own ids
    groups = {g: set((ids[ids // 8 == g] % 8).tolist()) for g in (300, 511, 777)}
    assert groups == {300: set(range(8)), 511: {0}, 777: {7}}
    assert {0, v - 1} <= set(ids.tolist())
    s = fam["full"]
    assert c.bias_cnt[s] == lpr.CAP + 5 and np.unique(c.bias_ids[s]).size == lpr.CAP
    strays = [s for s, fs in c.families.items() if "stray" in fs]
    a, b = strays
    head = c.bias_ids[a, :c.bias_cnt[a]].astype(np.int64)
    assert {-1, v, 2 ** 31 - 1} <= set(head.tolist()) and ((head >= 0) & (head < v)).sum() >= 30
    assert head[0] == -1 and head[-1] < 0                                   # first and last entries of the list stray
    assert c.bias_cnt[b] == -3 and lpr.bias_row(c, b) is None
    rows, _, cand = lpr.rows_expected("main_8200")
    ra = int(np.flatnonzero(c.slot == a)[0])
    applied = np.flatnonzero(lpr.bias_row(c, a))
    assert applied.size >= 30 and (rows[ra, applied] != lpr.process_np(c.x[ra], (c.state[a] & 0x8000) != 0,
                                                                        c.state[a] & 0x7fff, *c.params[a])[applied]).sum() >= 24
    # banned: the raw argmax is banned, the processed maximum ties across threads, waves and sweeps; lowest id wins
    s = fam["banned"]
    r = int(np.flatnonzero(c.slot == s)[0])
    raw = int(np.argmax(lpr.bits_f32(c.x[r])))
    assert np.isneginf(lpr.bias_row(c, s)[raw]) and rows[r, raw] == 0xff80
    vals = lpr.bits_f32(rows[r])
    tie = np.flatnonzero(vals == vals.max())
    thread = (tie % 8192) // 8
    assert tie.size == 4 and len(set(thread.tolist())) == 4 and len(set((thread // 64).tolist())) >= 3
    assert (tie >= 8192).any() and cand[r][1] == tie.min() and cand[r][1] != raw
    r = int(np.flatnonzero(c.slot == fam["last_max"])[0])
    assert cand[r][1] == v - 1
    # the other shapes: all eight ids of the only group; bitmap bytes that are no multiple of 4; the LDS cap
    t = lpr.rows_case("shape_8")
    assert sorted(t.bias_ids[0, :8].tolist()) == list(range(8)) and (1016 // 8) % 4 != 0
    big = lpr.rows_case("cap_393216")
    assert big.vocab // 8 == 48 * 1024 and {0, big.vocab - 1} <= set(big.bias_ids[1].tolist())
    assert {lpr.rows_case(n).vocab for n in NAMES} == {8, 1016, 8192, 8200, 32776, 393216}


@pytest.mark.parametrize("name", NAMES)
def test_claimed_element_mutants_change_eight_elements_of_their_row(name):
    c = lpr.rows_case(name)
    rows, _, _ = lpr.rows_expected(name)
    for r, muts in c.claims.items():
        for m in muts:
            bad, _, _ = lpr.rows_oracle(c, True, m)
            assert (bad[r] != rows[r]).sum() >= 8, (r, m, int((bad[r] != rows[r]).sum()))


def test_row_mutants_change_the_main_case():
    c = lpr.rows_case("main_8200")
    rows, state, _ = lpr.rows_expected("main_8200")
    assert set(c.row_claims) == set(lpr.ROW_MUTATIONS)
    for m in c.row_claims:
        bad_rows, bad_state, _ = lpr.rows_oracle(c, True, m)
        n = int((bad_rows != rows).sum()) + int((bad_state != state).sum())
        assert n >= (8 if m.endswith(("by_row", "by_slot")) else 1), (m, n)
    bad_rows, bad_state, _ = lpr.rows_oracle(c, True, "nosat")     # the saturated count runs over into the prompt bit
    assert (bad_state != state).sum() == 1


def test_every_mutation_is_claimed():
    claimed = {m for n in NAMES for ms in lpr.rows_case(n).claims.values() for m in ms}
    assert claimed == set(lpr.ELEMENT_MUTATIONS)
    assert set(lpr.rows_case("main_8200").row_claims) == set(lpr.ROW_MUTATIONS)


def test_search_is_seeded_and_finds_every_element_mutant():
    p = lpr.rows_case("main_8200").params[1]
    for m in ("fma3", "fold34", "f64", "div"):
        a = lpr.search_rounding(p, m, 5, want=16, draws=50000)
        b = lpr.search_rounding(p, m, 5, want=16, draws=50000)
        assert a[0].size == 16 and all(np.array_equal(x, y) for x, y in zip(a, b)), m
