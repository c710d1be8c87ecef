"""The sampling oracle (tests/sampling_reference.py) has to be trusted before the kernel is judged by it:

* its draws follow the float64 softmax of the kept set (chi-square at significance 1e-4 over 20,480 fixed draws);
* its uniform is strictly inside (0, 1) and exact in fp32, and equals, bit for bit, what csrc/kernels/rng_hash.h
  computes (a stand-alone host program prints it);
* the record of why the mapping has 23 bits: the 24-bit one, emulated in numpy float32, gives exactly 1.0;
* the conditions under which a float32 kernel must agree with it hold for every input of
  tests/test_sampling_kernel_gpu.py: few undecided draws, top-p cuts far from moving, float32 score error within
  the figure that DELTA is built on — conditions on the reference alone, not measurements of the kernel.
"""

import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import sampling_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK64 = (1 << 64) - 1


def hash64_int(seed, step, token):
    """The same mix on Python integers."""
    z = (seed ^ (step * 0x9E3779B97F4A7C15) ^ (token * 0xD1B54A32D192ED03)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def old_uniform_fp32(z):
    """The mapping that hash_uniform had: 24 hash bits, fp32 arithmetic."""
    return (np.float32(int(z) >> 40) + np.float32(0.5)) * np.float32(2.0 ** -24)


def test_hash64_wraps_like_integers_mod_2_64():
    rng = np.random.default_rng(0)
    seeds = rng.integers(-2 ** 63, 2 ** 63, size=200)
    steps = rng.integers(0, 5000, size=200)
    toks = rng.integers(0, sr.LLAMA_VOCAB, size=200)
    got = sr.hash64(seeds, steps, toks)
    for s, a, b, g in zip(seeds.tolist(), steps.tolist(), toks.tolist(), got.tolist()):
        assert hash64_int(s & MASK64, a, b) == g
    assert int(sr.hash64(0x5eed, 0, 0)) == hash64_int(0x5eed, 0, 0)


def test_uniform_is_inside_the_unit_interval_and_exact_in_fp32():
    h = np.concatenate([[0, sr.H_MAX], np.random.default_rng(1).integers(0, sr.H_MAX + 1, size=10 ** 6)])
    u = sr.uniform_from_h(h)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24 and np.all((u > 0.0) & (u < 1.0))
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    # the kernel's fp32 expression gives the same value without rounding
    u32 = (h.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert u32.dtype == np.float32 and np.array_equal(u32.astype(np.float64), u)
    z = sr.hash64(77, 3, np.arange(1000))
    assert np.array_equal(sr.uniform(77, 3, np.arange(1000)), sr.uniform_from_h(z >> np.uint64(41)))


def test_the_24_bit_mapping_rounded_to_one():
    """Why the mapping changed: 16777215 + 0.5 is a tie in fp32 and rounds to 2^24, so u = 1.0, the Gumbel noise
    -log(-log(1)) = +inf, and the token wins the draw whatever its logit."""
    assert old_uniform_fp32(((1 << 24) - 1) << 40) == np.float32(1.0)
    assert old_uniform_fp32(((1 << 24) - 2) << 40) < np.float32(1.0)
    for seed, step, token in sr.EXTREME_MAX[:5]:
        z = hash64_int(seed, step, token)
        assert z >> 40 == (1 << 24) - 1 and old_uniform_fp32(z) == np.float32(1.0), (seed, token)
        assert float(sr.uniform(seed, step, token)) == 1.0 - 2.0 ** -24
    assert (256, 0, 99355) in sr.EXTREME_MAX[:5]
    with np.errstate(divide="ignore"):
        assert -np.log(-np.log(np.float32(1.0))) == np.inf


def test_extreme_triples_have_the_extreme_uniforms():
    assert len(sr.EXTREME_MAX) >= 5 and len(sr.EXTREME_MIN) >= 1 and len(sr.EXTREME_BOTH) >= 1
    for seed, step, token in sr.EXTREME_MAX:
        assert hash64_int(seed, step, token) >> 41 == sr.H_MAX and token < sr.LLAMA_VOCAB
    for seed, step, token in sr.EXTREME_MIN:
        assert hash64_int(seed, step, token) >> 41 == 0 and token < sr.LLAMA_VOCAB
    for seed, step, hi, lo in sr.EXTREME_BOTH:
        assert hash64_int(seed, step, hi) >> 41 == sr.H_MAX and hash64_int(seed, step, lo) >> 41 == 0


def test_host_program_matches_the_oracle_bit_for_bit(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "rng_hash_dump")
    src = os.path.join(ROOT, "csrc", "kernels", "tests", "rng_hash_dump.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, src], check=True)
    triples = list(sr.EXTREME_MAX[:5]) + [(0x5eed, 0, 0), (2 ** 63 + 12345, 977, sr.LLAMA_VOCAB - 1)]
    raws = [0, (1 << 41) - 1, 1 << 41, MASK64 - (1 << 41), MASK64]  # h = 0, 0, 1, 2^23 - 2, 2^23 - 1
    args = [str(v) for t in triples for v in t] + [a for r in raws for a in ("raw", str(r))]
    lines = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(lines) == len(triples) + len(raws)
    want = [hash64_int(*t) for t in triples] + raws
    for line, z in zip(lines, want):
        got_z, got_bits = (int(v, 16) for v in line.split())
        u = sr.uniform_from_h(z >> 41)
        assert got_z == z
        assert got_bits == int(np.float32(u).view(np.uint32)) and float(np.float32(u)) == float(u), (line, z)
    assert int(lines[-1].split()[1], 16) == int(np.float32(1.0 - 2.0 ** -24).view(np.uint32))
    assert int(lines[len(triples)].split()[1], 16) == int(np.float32(2.0 ** -24).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------


def chi2_sf(x, df):
    """P(chi-square with df degrees of freedom > x): the regularised upper incomplete gamma function Q(df / 2,
    x / 2) by its recurrence Q(a + 1, y) = Q(a, y) + y^a e^-y / Gamma(a + 1) from Q(1, y) or Q(1/2, y)."""
    y = x / 2.0
    a, q = (1.0, math.exp(-y)) if df % 2 == 0 else (0.5, math.erfc(math.sqrt(y)))
    while a < df / 2.0 - 1e-9:
        q += math.exp(a * math.log(y) - y - math.lgamma(a + 1.0))
        a += 1.0
    return q


def test_chi2_sf_against_tabulated_values():
    assert abs(chi2_sf(23.513, 4) - 1e-4) < 2e-7 and abs(chi2_sf(3.841, 1) - 0.05) < 1e-4
    assert abs(chi2_sf(18.307, 10) - 0.05) < 1e-4 and abs(chi2_sf(82.529, 63) - 0.05) < 2e-4


DIST_ROW = sr._bf16(np.random.default_rng(3).normal(0.0, 1.0, size=64))


@pytest.mark.parametrize("top_k,target", [(0, None), (10, None), (0, 0.7), (20, 0.8)])
def test_oracle_draws_follow_the_softmax_of_the_kept_set(top_k, target):
    t = 0.9
    top_p = 1.0 if target is None else sr.midpoint_p(DIST_ROW, t, top_k, target)
    seeds = np.repeat(np.arange(2048, dtype=np.int64) * 104729 + 17, 10)
    steps = np.tile(np.arange(10, dtype=np.int64), 2048)
    pred = sr.predict(DIST_ROW, t, top_k, top_p, seeds, steps)
    # the exact probabilities, from this test's own reading of the contract (a sort, not the oracle's levels)
    zz = torch.as_tensor(sr.scaled(DIST_ROW, t)).double()
    keep = torch.ones(64, dtype=torch.bool)
    if top_k:
        keep &= zz >= torch.topk(zz, top_k).values[-1]
    if top_p < 1.0:
        pr = torch.softmax(zz.masked_fill(~keep, -math.inf), -1)
        sp, _ = torch.sort(pr, descending=True)
        cut = int(torch.searchsorted(torch.cumsum(sp, 0), torch.tensor(top_p, dtype=torch.float64)))
        keep &= pr >= sp[cut]
    assert np.array_equal(pred.mask, keep.numpy()) and 1 < int(keep.sum()) <= 64
    if target is not None:
        assert int(keep.sum()) < (top_k or 64), "the top-p cut removes something"
    probs = torch.softmax(zz.masked_fill(~keep, -math.inf), -1).numpy()
    n = seeds.size
    counts = np.bincount(pred.token, minlength=64)
    assert counts[~keep.numpy()].sum() == 0
    expected = probs * n
    small = (expected < 5.0) & keep.numpy()
    obs = list(counts[keep.numpy() & ~small]) + ([counts[small].sum()] if small.any() else [])
    exp = list(expected[keep.numpy() & ~small]) + ([expected[small].sum()] if small.any() else [])
    stat = sum((o - e) ** 2 / e for o, e in zip(obs, exp))
    p_value = chi2_sf(stat, len(obs) - 1)
    print(f"top_k {top_k} top_p {top_p:.4f}: kept {int(keep.sum())} bins {len(obs)} chi2 {stat:.2f} p {p_value:.4f}")
    assert n >= 20000 and p_value >= 1e-4


def test_scores_is_the_single_draw_form_of_predict():
    c = sr.case("topp_v1024_t1.0_p0.5")
    pred = sr.reference(c.name)
    for i in (0, 100, 511):
        s = sr.scores(c.row, c.temperature, c.top_k, c.top_p, c.seeds[i], c.steps[i])
        order = np.argsort(-s, kind="stable")
        assert order[0] == pred.token[i] and order[1] == pred.second[i]
        assert s[order[0]] - s[order[1]] == pred.gap[i]
        assert np.array_equal(np.isfinite(s), pred.mask)


def test_advance_model_on_a_hand_computed_step():
    st = {"out": torch.tensor([7, 8, 9]), "ids": torch.tensor([1, 2, 3]), "pos": torch.tensor([3, 6, 7]),
          "ctx": torch.tensor([4, 7, 8], dtype=torch.int32), "slots": torch.tensor([0, 0, 0]),
          "bt": torch.tensor([[5, 6], [2, 9], [4, 1]], dtype=torch.int32), "step": torch.tensor([0, 10, 20]),
          "tokens": torch.full((2, 3), -1), "cnt": torch.tensor([1], dtype=torch.int32),
          "n_real": torch.tensor([2], dtype=torch.int32)}
    s = sr.advance_model(st, 3, 4)
    assert s["tokens"].tolist() == [[-1, -1, -1], [7, 8, 9]] and s["cnt"].tolist() == [2]
    assert s["ids"].tolist() == [7, 8, 3] and s["pos"].tolist() == [4, 7, 7] and s["ctx"].tolist() == [5, 8, 8]
    assert s["slots"].tolist() == [6 * 4 + 0, 9 * 4 + 3, 0] and s["step"].tolist() == [1, 11, 20]
    s2 = sr.advance_model(s, 3, 4)  # the window is full: no token row, the counter still grows; row 1 leaves the table
    assert s2["tokens"].tolist() == s["tokens"].tolist() and s2["cnt"].tolist() == [3]
    assert s2["slots"].tolist() == [6 * 4 + 1, -1, 0] and st["cnt"].tolist() == [1]


# ------------------------------------------------------------------------------------------------------------
# conditions on the inputs of the GPU tests


@pytest.mark.parametrize("name", list(sr.CASES))
def test_input_conditions(name):
    c = sr.case(name)
    pred = sr.reference(name, True)
    n = c.seeds.size
    assert c.row.dtype == torch.bfloat16 and c.row.numel() % 8 == 0 and c.steps.size == n
    assert float(np.float32(c.top_p)) == c.top_p
    print(f"{name}: kept {int(pred.mask.sum())} undecided {pred.undecided:.4f} margins {pred.margin_hi:.4f} "
          f"{pred.margin_lo:.4f} e32 {pred.e32:.3g} min gap {pred.gap.min():.3g}")
    assert pred.undecided <= sr.UNDECIDED_CAP
    assert pred.e32 <= sr.E32
    if c.top_p < 1.0 and c.margins:
        assert pred.margin_hi >= sr.MARGIN_MIN and pred.margin_lo >= sr.MARGIN_MIN
    if pred.mask.any():
        assert pred.mask[pred.token].all() and pred.mask[pred.second].all()
    else:
        assert not pred.token.any()


@pytest.mark.parametrize("name", list(sr.GROUPS["topk"]))
def test_topk_rows_have_a_sharp_boundary(name):
    c = sr.case(name)
    kept = sr.reference(name).mask
    zz = sr.scaled(c.row, c.temperature).astype(np.float64)
    vocab = zz.size
    assert int(kept.sum()) == (7 if name == "topk_tie4" else min(c.top_k, vocab))
    order = np.sort(zz)[::-1]
    if name == "topk_tie4":
        assert order[2] > order[3] == order[4] == order[5] == order[6] > order[7]
    elif c.top_k < vocab:
        assert order[c.top_k - 2] > order[c.top_k - 1] > order[c.top_k] > order[c.top_k + 1]
    # near-flat: the first dropped token would be drawn about as often as a kept one
    assert order[0] - order[min(c.top_k, vocab - 1)] < 0.15 and zz.std() < 0.08
    # every kept token is drawable, so a set one too small shows as well
    if c.top_k <= 50:
        assert set(np.unique(sr.reference(name).token)) == set(np.nonzero(kept)[0])


def test_radix_rows_exercise_the_digits():
    for side in ("below", "above"):
        c = sr.case(f"radix_lowbits_{side}")
        key = np.sort(sr.f2key(sr.scaled(c.row, c.temperature)))[::-1].astype(np.int64)
        k = c.top_k
        kth, other = key[k - 1], (key[k] if side == "below" else key[k - 2])
        assert kth != other and kth >> 16 == other >> 16 and (kth >> 24) == (key[k] >> 24) == (key[k - 2] >> 24)
        assert all(0 < ((kth >> s) & 255) < 255 for s in (0, 8, 16, 24))
        assert int(sr.reference(c.name).mask.sum()) == k
    c = sr.case("radix_sign")
    zz = np.sort(sr.scaled(c.row, c.temperature))[::-1]
    assert zz[7] > 0 > zz[8] and zz[c.top_k - 2] > zz[c.top_k - 1] > zz[c.top_k] and zz[c.top_k - 1] < 0
    assert int(sr.reference("radix_sign").mask.sum()) == c.top_k
    c = sr.case("radix_exponent")
    key = np.sort(sr.f2key(sr.scaled(c.row, c.temperature)))[::-1].astype(np.int64)
    top = key[: c.top_k + 8]
    assert len(set((top >> 23).tolist())) >= 12, "the entries around the threshold differ in the exponent"
    assert int(sr.reference("radix_exponent").mask.sum()) == c.top_k
    for name in sr.GROUPS["radix"]:  # the filler below the threshold would be drawn if the floor let it in
        c = sr.case(name)
        mass = np.exp(sr.scaled(c.row, c.temperature).astype(np.float64))
        assert mass[~sr.reference(name).mask].sum() / mass.sum() > 0.2


@pytest.mark.parametrize("name", list(sr.GROUPS["topp"]) + ["kp_differ", "kp_loose", "k_zero"])
def test_topp_boundary_level_is_heavy(name):
    c = sr.case(name)
    lv, cum = sr.levels(c.row, c.temperature, c.top_k)
    i = int(np.searchsorted(cum, c.top_p))
    assert cum[i] - (cum[i - 1] if i else 0.0) >= 2e-2
    zz = sr.scaled(c.row, c.temperature).astype(np.float64)
    assert np.unique(zz[zz >= lv[min(i + 1, lv.size - 1)]]).size == min(i + 2, lv.size), "distinct levels"
    if name in sr.GROUPS["topp"]:
        target = float(name.rsplit("_p", 1)[1])
        assert abs(c.top_p - target) < 0.04


def test_combined_rows_mean_what_they_say():
    c = sr.case("kp_differ")
    within, whole = sr.reference("kp_differ").mask, sr.kept_set(c.row, c.temperature, 0, c.top_p)[0]
    topk = sr.kept_set(c.row, c.temperature, c.top_k, 1.0)[0]
    assert within.sum() < topk.sum() == c.top_k and whole.sum() != within.sum()
    # the other reading (top-p over the whole row, then intersect with top-k) keeps another set
    assert not np.array_equal(whole & topk, within)
    mass = np.exp(sr.scaled(c.row, c.temperature).astype(np.float64))
    assert 1.0 - mass[topk].sum() / mass.sum() > 10 * sr.MARGIN_MIN
    c = sr.case("kp_loose")
    assert np.array_equal(sr.reference("kp_loose").mask, sr.kept_set(c.row, c.temperature, c.top_k, 1.0)[0])
    assert sr.kept_set(c.row, c.temperature, 0, c.top_p)[0].sum() > c.top_k
    a, b, z = (sr.reference(n) for n in ("k_eq_vocab", "k_gt_vocab", "k_zero"))
    assert np.array_equal(a.token, z.token) and np.array_equal(b.token, z.token) and z.mask.sum() < 22
    assert int(sr.reference("p_one").mask.sum()) == 1024
    c = sr.case("p_zero")
    top = int(torch.argmax(c.row.float()))
    for name in ("p_zero", "p_tiny"):
        assert (sr.reference(name).token == top).all() and sr.reference(name).mask.sum() == 1


def test_masked_and_extreme_rows():
    for name in ("masked3_v1024", f"masked3_v{sr.LLAMA_VOCAB}"):
        pred = sr.reference(name)
        finite = np.nonzero(np.isfinite(sr.row_f32(sr.case(name).row)))[0]
        assert finite.size == 3 and set(np.unique(pred.token)) == set(finite) and pred.mask.sum() == 3
    assert (sr.reference("masked_all").token == 0).all() and not sr.reference("masked_all").mask.any()
    c = sr.case("extreme")
    pred = sr.reference("extreme")
    row = sr.row_f32(c.row)
    special = np.nonzero(row == -10.0)[0]
    assert row.max() == 10.0 and special.size >= 7 and not np.isin(pred.token, special).any()
    assert 20.0 > sr.G_MAX - sr.G_MIN and abs(sr.G_MAX - 16.6355) < 1e-3
    for i in range(c.seeds.size):  # each draw has a special token at an extreme uniform, and it loses by a margin
        u = sr.uniform(c.seeds[i], c.steps[i], special)
        assert u.max() == 1.0 - 2.0 ** -24 or u.min() == 2.0 ** -24
        s = sr.scores(c.row, 1.0, 0, 1.0, c.seeds[i], c.steps[i])
        assert s.max() - s[special].max() > 0.5
