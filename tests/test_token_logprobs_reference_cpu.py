"""tests/token_logprobs_reference.py judged before token_logprobs_kernel is judged by it: the oracle against
ref.token_logprobs and closed forms; for every GPU case by name its premise (the kernel's branch, computed from the
row with the geometry written out in the reference), the two tolerance conditions and every mutation it claims;
every mutation claimed by some case; the coverage of the lists."""

import math

import numpy as np
import pytest
import torch

from src.ops import reference as ref

from tests import token_logprobs_reference as tlr

NAMES = tlr.case_names()


def as_torch(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def assert_matches_ref(bits, targets, top_n):
    lp, rank, top_lp, top_id = tlr.oracle(bits, targets, top_n)
    x = as_torch(bits)
    rlp, rrank, rtop_lp, rtop_id = ref.token_logprobs(x, torch.as_tensor(np.asarray(targets)), top_n)
    assert np.array_equal(rank, rrank.numpy()) and np.array_equal(top_id, rtop_id.numpy())
    # the engine's function returns fp32: the float64 values it rounds are log_softmax's
    lsm = torch.log_softmax(x.double(), -1).numpy()
    for r, t in enumerate(np.asarray(targets)):
        if 0 <= t < bits.shape[1] and np.isfinite(lp[r]):
            assert abs(lp[r] - lsm[r, t]) <= 1e-12
        fin = np.isfinite(top_lp[r])
        assert np.abs(top_lp[r][fin] - lsm[r, top_id[r]][fin]) .max(initial=0.0) <= 1e-12
        assert np.array_equal(np.isfinite(top_lp[r]), np.isfinite(lsm[r, top_id[r]]))
    for a, b in ((lp, rlp.numpy()), (top_lp, rtop_lp.numpy())):
        fin = np.isfinite(a)
        assert np.array_equal(a[~fin], b[~fin].astype(np.float64))
        assert np.all(np.abs(a[fin] - b[fin]) <= 2.0 ** -23 * np.maximum(np.abs(a[fin]), 1e-30))


def test_bf16_helpers_round_trip():
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    fin = np.isfinite(tlr.f32(bits))
    assert np.array_equal(tlr.bf16_bits(tlr.f32(bits[fin])), bits[fin])
    assert np.array_equal(as_torch(bits[fin]).float().numpy(), tlr.f32(bits[fin]))
    k = tlr.key16(bits[fin])
    v = tlr.f32(bits[fin]).astype(np.float64)
    o = np.argsort(k, kind="stable")
    assert np.all(np.diff(v[o]) >= 0)                                  # the key orders as the value does
    keep = bits[fin] != 0x8000
    assert np.array_equal(tlr.bits_of_key16(k[keep]), bits[fin][keep]) and 0x7fff not in set(k.tolist())


def test_equals_the_engine_reference_on_the_random_family_and_the_hand_made_rows():
    c = tlr.by_name("random_8200")
    assert_matches_ref(c.bits, c.targets, 20)
    inf = 0xff80
    v = 1000
    x = np.full((1, v), inf, dtype=np.uint16)                           # fewer finite entries than asked
    x[0, [900, 17, 450]] = tlr.bf16_bits([2.0, 1.0, 2.0])
    assert_matches_ref(x, [17], 20)
    x = np.full((1, v), tlr.bf16_bits(-1.0), dtype=np.uint16)           # signed zeros
    x[0, 10], x[0, 20], x[0, 30] = 0x8000, 0x0000, 0x8000
    assert_matches_ref(x, [30], 5)
    assert tlr.oracle(x, [30], 5)[3][0, :3].tolist() == [10, 20, 30] and tlr.oracle(x, [30], 5)[1][0] == 2
    rng = np.random.default_rng(3)                                      # an outlier above a flat row, keys across 0
    x = tlr.bf16_bits(rng.standard_normal((3, 32000)) * 0.01)
    x[0, 5] = tlr.bf16_bits(50.0)
    x[1, [7, 31999]] = tlr.bf16_bits([50.0, 12.0])
    x[2] = tlr.bf16_bits(-np.abs(tlr.f32(x[2])) - 1.0)
    x[2, 100] = tlr.bf16_bits(3.0)
    assert_matches_ref(x, [5, 9, 100], 20)
    x = tlr.bf16_bits(rng.standard_normal((2, v)) * 4)                  # mostly -inf, a target on a -inf entry
    dead = rng.random((2, v)) < 0.9
    x[dead] = inf
    assert_matches_ref(x, [int(np.flatnonzero(dead[0])[5]), v + 5], 20)
    assert_matches_ref(np.full((3, 32000), 0x3fc0, dtype=np.uint16), [0, 77, 31999], 20)


def test_closed_forms():
    for v in (8, 1000, 8200):
        lp, rank, top_lp, top_id = tlr.oracle(np.full((1, v), 0x3fc0, dtype=np.uint16), [v - 1], min(v, 20))
        assert abs(lp[0] + math.log(v)) <= 1e-12 and rank[0] == v - 1
        assert np.abs(top_lp + math.log(v)).max() <= 1e-12 and top_id[0].tolist() == list(range(min(v, 20)))
    for k in (1, 3, 500):
        x = np.full((1, 1000), 0xff80, dtype=np.uint16)
        x[0, 1000 - k:] = 0
        lp, rank, top_lp, top_id = tlr.oracle(x, [999], 1)
        assert abs(lp[0] + math.log(k)) <= 1e-12 and rank[0] == k - 1 and top_id[0, 0] == 1000 - k
    lp, rank, _, _ = tlr.oracle(np.zeros((2, 8), dtype=np.uint16), [-1, 8], 0)
    assert np.all(lp == -np.inf) and rank.tolist() == [8, 8]


@pytest.mark.parametrize("name", NAMES)
def test_premise(name):
    c = tlr.by_name(name)
    assert c.bits.dtype == np.uint16 and c.vocab % 8 == 0 and 1 <= c.bits.shape[0] <= 3
    assert 0 <= c.top_n <= min(tlr.MAX_TOP, c.vocab)
    z = tlr.f32(c.bits)
    assert not np.isnan(z).any() and not (z == np.inf).any() and np.isfinite(z).any(axis=1).all()
    assert len(c.premise) in (0, c.bits.shape[0])
    for r, want in enumerate(c.premise):
        g = tlr.geometry(c.bits[r], c.top_n)
        for key, val in want.items():
            if key == "n_ties":
                assert g["ties"].size == val, (key, g["ties"].size)
            elif key == "slab_ties":
                assert tuple(g["slab_ties"].tolist()) == tuple(val), g["slab_ties"]
            elif key == "negzero_bin_empty":    # -0.0 entries exist, file under +0.0, and their own key's bin is empty
                kmax = int(tlr.key16(c.bits[r]).max())
                assert (c.bits[r] == 0x8000).any() and 0 < kmax - 0x7fff < tlr.WINDOW
                assert g["whist"][kmax - 0x7fff] == 0 and g["whist"][kmax - 0x8000] >= (c.bits[r] == 0x8000).sum()
            else:
                assert g[key] == val, (key, g[key], val)
        if want.get("bin", 0) is None:
            assert g["whist"].sum() < c.top_n                           # the window holds fewer than asked
        # the oracle's list and the geometry agree: the entries above the threshold, then its ties by id
        ids = tlr.expected(name)[0][3][r]
        above = np.flatnonzero(tlr.key16(c.bits[r]) > g["t16"])
        assert set(above.tolist()) <= set(ids.tolist()) and above.size < c.top_n <= above.size + g["ties"].size
        assert sorted(set(ids.tolist()) - set(above.tolist())) == g["ties"][:c.top_n - above.size].tolist()


def test_family_premises_that_span_cases():
    c = tlr.by_name("slabs_lane_32776")           # index order differs from lane-major order inside one iteration
    s = tlr.slab_of(32776)
    assert s == 2056 > tlr.WALK
    off = tlr.geometry(c.bits[0], c.top_n)["ties"] - 2 * s
    assert off[0] == 8 and 512 in off.tolist() and (off >= tlr.WALK).sum() == 2
    assert tlr.slab_of(1000) == 64 and 1000 - 15 * 64 == 40 and tlr.slab_of(8200) == 520 and tlr.slab_of(8) == 8
    g = tlr.geometry(tlr.by_name("slabs_many_8200").bits[0], 5)
    assert g["slab_ties"][0] > 5 and g["slab_ties"][5] > 5
    assert np.flatnonzero(tlr.geometry(tlr.by_name("slabs_ragged_1000").bits[0], 5)["slab_ties"]).tolist() == [15]
    assert np.flatnonzero(tlr.geometry(tlr.by_name("slabs_ragged_8200").bits[0], 5)["slab_ties"]).tolist() == [15]
    # rank: targets at both ends, tied with many entries on both sides
    for v in (1000, 8200):
        c = tlr.by_name(f"rank_ties_{v}")
        assert c.targets.tolist() == [0, v - 1, v // 2]
        same = c.bits[2] == c.bits[2, v // 2]
        assert same[:v // 2].sum() > 100 and same[v // 2 + 1:].sum() > 100
    c = tlr.by_name("rank_negzero")
    assert c.bits[0, 500] == 0x8000 and (c.bits[0, :500] == 0).sum() > 100 and (c.bits[0, 501:] == 0).sum() > 100
    c = tlr.by_name("rank_minus_inf")
    assert c.bits[0, c.targets[0]] == 0xff80 and c.targets.tolist()[1:] == [-1, 1000]
    # mass: the maximum sits in the last 16-byte group, past row_argmax's eight-deep sweep
    c = tlr.by_name("mass_last_group_65544")
    assert int(np.argmax(tlr.f32(c.bits[0]))) >= tlr.SWEEP_MAX and c.vocab - tlr.SWEEP_MAX == 8
    z = tlr.f32(tlr.by_name("mass_loud_8200").bits)
    with np.errstate(over="ignore"):
        assert z.min() >= 100 and z.max() <= 120 and np.exp(z.astype(np.float32)).sum(dtype=np.float32) == np.inf


@pytest.mark.parametrize("name", NAMES)
def test_tolerance_conditions(name):
    c = tlr.by_name(name)
    (lp, _, top_lp, _), (tol_lp, tol_top) = tlr.expected(name)
    assert max(tol_lp.max(), tol_top.max(initial=0.0)) <= 2e-5
    for r in range(c.bits.shape[0]):
        z = tlr.f32(c.bits[r]).astype(np.float64)
        big_l = math.log(np.exp(z - z.max()).sum())
        assert abs(tlr.model_lse(c.bits[r]) - big_l) <= tlr.tol_const(c.vocab) / 4


@pytest.mark.parametrize("name", NAMES)
def test_claimed_mutations_change_the_result(name):
    c = tlr.by_name(name)
    base, (tol_lp, tol_top) = tlr.expected(name)
    for m in c.claims:
        assert tlr.differs(base, tlr.oracle(c.bits, c.targets, c.top_n, m), (4 * tol_lp, 4 * tol_top)), m
    if "sum_drop_chunk" in c.claims:      # ANY single 16-byte chunk, not only the mutant's lightest one
        z = tlr.f32(c.bits[0]).astype(np.float64)
        p = np.exp(z - z.max()).reshape(-1, 8).sum(1) / np.exp(z - z.max()).sum()
        assert -math.log1p(-p.min()) > 4 * tol_lp.max()
    if "rank_drop_chunk" in c.claims:     # every chunk holds an entry that comes before the target
        t = int(c.targets[0])
        z = tlr.f32(c.bits[0])
        before = (z > z[t]) | ((z == z[t]) & (np.arange(c.vocab) < t))
        assert before.reshape(-1, 8).sum(1).min() >= 1


def test_every_mutation_is_claimed():
    claimed = {m for c in tlr.cases() for m in c.claims}
    assert claimed == set(tlr.MUTATIONS)
    assert len(tlr.MUTATIONS) == 15


def test_coverage():
    cs = tlr.cases()
    geo = [(c, tlr.geometry(c.bits[r], c.top_n)) for c in cs if c.top_n for r in range(c.bits.shape[0])]
    lad = [(c, g) for c, g in geo if c.family == "ladder"]
    assert {g["bin"] for c, g in lad if g["bin"] is not None} == set(tlr.LADDER_WINDOW_D)
    dists = {int(c.name.split("_D")[1].split("_")[0]) for c, g in lad if g["bin"] is None}
    assert dists == set(tlr.LADDER_FALLBACK_D)
    # both ends of the window, both sides of a lane's group of four bins and of the scan's halves
    bins = {g["bin"] for c, g in geo if g["bin"] is not None}
    assert {0, 255} <= bins and {3, 4} <= bins and {127, 128} <= bins
    assert {g["half"] for c, g in geo if g["bin"] is not None} == {"zeros", "ones"}
    fb = [g for c, g in geo if g["bin"] is None]
    assert {g["patch"] for g in fb} == {True, False} and {g["half"] for g in fb} == {"zeros", "ones"}
    assert any(g["t16"] == 0x8000 and not g["patch"] for g in fb)       # the fallback's threshold exactly at +0.0
    assert {c.vocab for c in cs} == set(tlr.VOCABS)
    assert {c.top_n for c in cs} == {0, 1, 5, 8, 20}
    assert {c.vocab for c in cs if c.top_n == 20} >= {24, 1000, 8200, 65544}
    assert {c.family for c in cs} == {"ladder", "zero", "slabs", "rank", "mass", "random"}
    # the ladder's a and t: none, one and top_n - 1 above; one, exactly enough, five more and 3 top_n at the level
    kinds_a, kinds_t = set(), set()
    for c, g in lad:
        a, t, n = g["above"], g["ties"].size, c.top_n
        kinds_a |= {k for k, v in (("0", 0), ("1", 1), ("n-1", n - 1)) if a == v}
        kinds_t |= {k for k, v in (("1", 1), ("n-a", n - a), ("n-a+5", n - a + 5), ("3n", 3 * n)) if t == v}
    assert kinds_a == {"0", "1", "n-1"} and kinds_t == {"1", "n-a", "n-a+5", "3n"}
