"""A float64 oracle of the sampling op (csrc/kernels/sampling.hip) and of the decode-step advance
(csrc/kernels/decode_step.hip), written from their documented contracts, plus the inputs that the CPU tests
(tests/test_sampling_reference_cpu.py) qualify and the GPU tests (tests/test_sampling_kernel_gpu.py) run: both
import the very same rows from here.

The contract:

* ``hash64(seed, step, token)`` is splitmix64's finaliser of ``seed ^ step * 0x9E3779B97F4A7C15 ^ token *
  0xD1B54A32D192ED03`` (mod 2^64) and ``uniform = (h + 0.5) * 2^-23`` with ``h = hash64 >> 41``
  (csrc/kernels/rng_hash.h): exactly representable in fp32 and strictly inside (0, 1).
* The scaled logit is ``zz = fl32(z * fl32(1 / t))``, the one fp32 step that the oracle repeats so that ties stay
  ties; everything after it is float64 here.
* Top-k keeps every entry ``>=`` the k-th largest (ties at the threshold are kept); ``top_k <= 0`` or ``>= vocab``
  filters nothing. Top-p keeps the smallest set of value levels, from the top, whose mass WITHIN the top-k set
  reaches ``p`` (whole tie levels, at least the top one). ``-inf`` entries are never drawn; a row without a
  finite entry gives token 0.
* The draw is Gumbel-max: the argmax over the kept set of ``zz - log(-log(u))``, lowest id on an exact tie.

A kernel that computes the same scores in fp32 agrees with the oracle wherever the gap between the two best
scores of a draw exceeds its own rounding error. ``E32`` is that error measured for this file's inputs with
numpy float32 (the kernel's operation order with correctly rounded logs): the largest absolute difference from the
float64 scores over the 50 best tokens of every draw of every case below is 1.53e-6 (``predict(with_e32=True)``; the
largest is the sigma = 3 row of 128,256 entries at temperature 0.8, the other cases stay under 8e-7), and
tests/test_sampling_reference_cpu.py fails if a case exceeds ``E32 = 1.6e-6``. ``DELTA = 64 * E32 = 1.024e-4``
leaves room for native log intrinsics that are a few ULP off where ``u`` is close to 1 and the inner log is small.
A draw whose gap exceeds DELTA is *decided*.
"""

import dataclasses
import functools
import math

import numpy as np
import torch

E32 = 1.6e-6
DELTA = 64 * E32
UNDECIDED_CAP = 0.02   # largest share of undecided draws per case
MARGIN_MIN = 1e-2      # smallest top-p margin, as a share of the kept mass (> 128256 * 2^-24 = 7.6e-3)
LLAMA_VOCAB = 128256

_C_STEP = np.uint64(0x9E3779B97F4A7C15)
_C_TOKEN = np.uint64(0xD1B54A32D192ED03)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
H_MAX = (1 << 23) - 1

# Gumbel noise -log(-log(u)) over u in [2^-24, 1 - 2^-24]: a token more than G_SPAN below the best kept one
# cannot win whatever the uniforms are, so predict() may leave it out (exactly, not approximately)
G_MAX = -math.log(-math.log1p(-2.0 ** -24))
G_MIN = -math.log(-math.log(2.0 ** -24))
G_SPAN = G_MAX - G_MIN + 1e-9


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def hash64(seed, step, token):
    """uint64 hash of broadcastable integer arrays (int64 values wrap to uint64 as in the kernel)."""
    seed, step, token = _u64(seed), _u64(step), _u64(token)
    with np.errstate(over="ignore"):
        z = seed ^ (step * _C_STEP) ^ (token * _C_TOKEN)
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def uniform_from_h(h):
    return (np.asarray(h).astype(np.float64) + 0.5) * 2.0 ** -23


def uniform(seed, step, token):
    """The exact uniform (float64 holds it exactly, and so does fp32)."""
    return uniform_from_h(hash64(seed, step, token) >> np.uint64(41))


def row_f32(row):
    """bf16 torch row (or anything array-like) -> numpy float32."""
    if isinstance(row, torch.Tensor):
        return row.detach().cpu().float().numpy()
    return np.asarray(row, dtype=np.float32)


def scaled(row, temperature):
    """zz = fl32(z * fl32(1 / t)) as float32."""
    inv_t = np.float32(1.0) / np.float32(temperature)
    with np.errstate(invalid="ignore"):
        return (row_f32(row) * inv_t).astype(np.float32)


def _topk_mask(zz, top_k):
    mask = zz > -np.inf
    top_k = int(top_k)
    if 0 < top_k < zz.size:
        kth = np.partition(zz, zz.size - top_k)[zz.size - top_k]
        mask &= zz >= kth
    return mask


def levels(row, temperature, top_k):
    """Distinct values of the top-k set from the top, and their cumulative mass as a share of the set's mass."""
    zz = scaled(row, temperature).astype(np.float64)
    vals = zz[_topk_mask(zz, top_k)]
    if vals.size == 0:
        return vals, vals
    lv, inv = np.unique(vals, return_inverse=True)
    w = np.bincount(inv, weights=np.exp(vals - lv[-1]))[::-1]
    cum = np.cumsum(w)
    return lv[::-1], cum / cum[-1]


def kept_set(row, temperature, top_k, top_p):
    """-> (mask [vocab] bool, margin_hi, margin_lo): the kept set, and how far the top-p cut is from moving:
    ``cum[i] - p`` and ``p - cum[i - 1]`` for the cut level i, as shares of the top-k set's mass. Without a top-p
    cut both are inf; with the cut at the top level the lower one is inf (no mass above it whose sum could err)."""
    zz = scaled(row, temperature).astype(np.float64)
    mask = _topk_mask(zz, top_k)
    hi = lo = math.inf
    p = float(np.float32(top_p))
    if p < 1.0 and mask.any():
        lv, cum = levels(row, temperature, top_k)
        i = min(int(np.searchsorted(cum, p, side="left")), lv.size - 1)
        mask &= zz >= lv[i]
        hi = float(cum[i] - p)
        lo = float(p - cum[i - 1]) if i > 0 else math.inf
    return mask, hi, lo


def scores(row, temperature, top_k, top_p, seed, step):
    """One draw's perturbed scores [vocab] in float64: zz - log(-log(u)) on the kept set, -inf outside it."""
    zz = scaled(row, temperature).astype(np.float64)
    mask, _, _ = kept_set(row, temperature, top_k, top_p)
    u = uniform(seed, step, np.arange(zz.size))
    return np.where(mask, zz - np.log(-np.log(u)), -np.inf)


@dataclasses.dataclass
class Prediction:
    token: np.ndarray    # [n] the argmax token (lowest id on an exact tie)
    second: np.ndarray   # [n] the runner-up (= token where the kept set has one entry)
    gap: np.ndarray      # [n] best score - second best (inf with one entry)
    mask: np.ndarray     # [vocab] the kept set
    margin_hi: float
    margin_lo: float
    e32: float           # fp32_score_error of these draws (nan unless asked for)

    @property
    def undecided(self):
        return float(np.mean(self.gap <= DELTA))


def predict(row, temperature, top_k, top_p, seeds, steps, prune=True, with_e32=False):
    """The oracle's draws for n (seed, step) pairs on one row. ``prune`` leaves out kept tokens more than G_SPAN
    below the best one (they cannot win); ``with_e32`` also measures the float32 score error (module docstring)."""
    seeds, steps = np.asarray(seeds, dtype=np.int64), np.asarray(steps, dtype=np.int64)
    n = seeds.size
    zz32 = scaled(row, temperature)
    zz = zz32.astype(np.float64)
    mask, hi, lo = kept_set(row, temperature, top_k, top_p)
    token = np.zeros(n, dtype=np.int64)
    second = np.zeros(n, dtype=np.int64)
    gap = np.full(n, np.inf)
    e32 = 0.0 if with_e32 else math.nan
    cand = np.nonzero(mask & (zz >= zz[mask].max() - G_SPAN) if prune and mask.any() else mask)[0]
    if cand.size:
        zc, zc32 = zz[cand], zz32[cand]
        chunk = max(1, 3_000_000 // cand.size)
        for a in range(0, n, chunk):
            u = uniform(seeds[a:a + chunk, None], steps[a:a + chunk, None], cand[None, :])
            s = zc[None, :] - np.log(-np.log(u))
            rows = np.arange(s.shape[0])
            if with_e32:
                s32 = zc32[None, :] - np.log(-np.log(u.astype(np.float32)))
                assert s32.dtype == np.float32
                kth = np.partition(s, -min(50, cand.size), axis=1)[:, -min(50, cand.size)]
                e32 = max(e32, float(np.abs(s32.astype(np.float64) - s)[s >= kth[:, None]].max()))
            b = np.argmax(s, axis=1)
            best = s[rows, b]
            token[a:a + chunk] = cand[b]
            second[a:a + chunk] = cand[b]
            if cand.size > 1:
                s[rows, b] = -np.inf
                b2 = np.argmax(s, axis=1)
                second[a:a + chunk] = cand[b2]
                gap[a:a + chunk] = best - s[rows, b2]
    return Prediction(token, second, gap, mask, hi, lo, e32)


# ------------------------------------------------------------------------------------------------------------
# the decode-step advance


def advance_model(state, rows, block_size):
    """One decode-step advance on ``state`` (dict of CPU tensors: out, ids, pos, ctx, slots, bt [S, W], step,
    tokens [K, S], cnt [1], n_real [1]), in plain Python, from the header of csrc/kernels/decode_step.hip: the
    token row cnt[0] is written for every row while cnt[0] < K; rows < n_real take the token as their next id and
    grow position / context / step by one, their slot is looked up in the block table (-1 past its last column);
    rows >= n_real keep their inputs; cnt[0] grows by one. Returns a new dict."""
    s = {k: v.clone() for k, v in state.items()}
    k, n_real = int(s["cnt"][0]), int(s["n_real"][0])
    k_max, width = s["tokens"].shape[0], s["bt"].shape[1]
    for r in range(rows):
        t = int(s["out"][r])
        if k < k_max:
            s["tokens"][k, r] = t
        if r < n_real:
            s["ids"][r] = t
            p = int(s["pos"][r]) + 1
            s["pos"][r] = p
            s["ctx"][r] += 1
            s["step"][r] += 1
            b = p // block_size
            s["slots"][r] = int(s["bt"][r, b]) * block_size + p % block_size if b < width else -1
    s["cnt"][0] = k + 1
    return s


# ------------------------------------------------------------------------------------------------------------
# inputs


@dataclasses.dataclass
class Case:
    name: str
    row: torch.Tensor      # [vocab] bf16, CPU
    temperature: float
    top_k: int
    top_p: float           # as the kernel reads it: a float32 value
    seeds: np.ndarray      # [n] int64
    steps: np.ndarray      # [n] int64
    prune: bool = True
    margins: bool = True   # False: a degenerate top_p (0, 1e-6) whose cut is the top level by construction

    def predict(self, with_e32=False):
        return predict(self.row, self.temperature, self.top_k, self.top_p, self.seeds, self.steps, self.prune,
                       with_e32)


def _bf16(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16)


def _draws(n, salt):
    i = np.arange(n, dtype=np.int64)
    return i * 7919 + salt, (i * 5 + salt) % 11


def _scatter(vocab, heavy, filler, rng):
    """A row of ``filler`` with ``heavy`` at random places, the first and last entry among them."""
    row = np.array(filler, dtype=np.float32)
    at = rng.permutation(vocab - 2)[:len(heavy)] + 1
    if len(heavy) >= 2:
        at[0], at[-1] = 0, vocab - 1
    row[at] = heavy
    return _bf16(row)


def flat_topk_row(vocab, k, rng, tie=False):
    """Near-flat row for the top-k boundary at temperature 0.8 (sigma about 0.05 after it): k - 1 entries on the
    bf16 levels 0.5 + j * 2^-8 (j = 1..20), the k-th alone at 0.5, the (k + 1)-th alone one bf16 step below
    (0.5 - 2^-9) and the rest further down on 0.5 - j * 2^-9 (j >= 2): every kept token has mass about 1 / k and
    the first dropped one nearly as much. ``tie``: the k-th place is inside four equal entries at 0.5 (places
    k - 1 .. k + 2), all of which are kept."""
    k_top = min(k, vocab)
    top = 0.5 + rng.integers(1, 21, size=k_top - 1 - (1 if tie else 0)) * 2.0 ** -8
    mid = [0.5] * 4 if tie else [0.5]
    n_rest = vocab - len(top) - len(mid)
    rest = np.empty(0)
    if n_rest > 0:
        j = 2 + np.minimum(np.floor(np.abs(rng.normal(0.0, 12.0, size=n_rest))), 100)
        rest = 0.5 - j * 2.0 ** -9
        if not tie:
            rest[0] = 0.5 - 2.0 ** -9
    vals = np.concatenate([top, mid, rest])
    return _bf16(vals[rng.permutation(vocab)])


def ladder_row(vocab, temperature, rng, heavy=22):
    """``heavy`` tokens on distinct bf16 levels whose masses AFTER the temperature fall about linearly from 0.07
    to 0.02 of the total (every level carries at least 2e-2, so a midpoint between two cumulative masses is 1e-2
    from either), and a tail 25 / t and more below the top whose whole mass is under 2e-6."""
    q = np.linspace(0.07, 0.02, heavy)
    z = temperature * (np.log(q) - np.log(q[0]))
    tail = -temperature * (25.0 + rng.integers(0, 4, size=vocab))
    return _scatter(vocab, z[rng.permutation(heavy)], tail, rng)


def midpoint_p(row, temperature, top_k, target):
    """The float32 midpoint between two consecutive cumulative masses (steps of at least 2e-2 only) of the
    reference's top-k set that lies nearest to ``target``."""
    _, cum = levels(row, temperature, top_k)
    lower = np.concatenate([[0.0], cum[:-1]])
    mid = np.where(cum - lower >= 2e-2, (cum + lower) / 2, np.inf)
    return float(np.float32(mid[np.argmin(np.abs(mid - target))]))


def f2key(zz32):
    """Order-preserving uint32 key of a float32 array (larger float, larger key)."""
    u = np.asarray(zz32, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


RADIX_T = 0.7
_FILLER = (-6.0, -5.0)  # far below every threshold, yet 30 % of the row's mass: a floor that lets it in shows


def _radix_row(vocab, heavy, rng):
    return _scatter(vocab, np.asarray(heavy)[rng.permutation(len(heavy))], rng.uniform(*_FILLER, size=vocab), rng)


def radix_lowbits_row(vocab, rng):
    """64 consecutive bf16 levels 1 - j * 2^-8, one token each. Two bf16 values times one fp32 factor differ by at
    least 2^15 fp32 ULPs, so no two keys of a row differ in the lowest byte alone; consecutive levels in one
    binade are as close as keys get: at temperature 0.7 they are 0xB6DB apart, share the top byte always and the
    top 16 bits at about every fourth level, and their low bytes are filled by the fp32 product."""
    return _radix_row(vocab, 1.0 - np.arange(64) * 2.0 ** -8, rng)


def radix_lowbits_k(row, side):
    """A place k in 8..56 whose k-th largest key shares its top 16 bits with the (k + 1)-th ('below') or the
    (k - 1)-th ('above') and has a lowest byte other than 0x00 / 0xff."""
    key = np.sort(f2key(scaled(row, RADIX_T)))[::-1]
    for k in range(8, 57):
        other = key[k] if side == "below" else key[k - 2]
        if key[k - 1] >> 16 == other >> 16 and 0 < (key[k - 1] & 0xFF) < 0xFF:
            return k
    raise AssertionError("no such place")


def radix_sign_row(vocab, rng):
    """8 positive levels j * 2^-6 and 40 negative ones -j * 2^-8 over four binades: near-flat, and the 20th place is
    among the negatives, whose keys are the complemented bit patterns."""
    return _radix_row(vocab, np.concatenate([np.arange(1, 9) * 2.0 ** -6, -np.arange(1, 41) * 2.0 ** -8]), rng)


def radix_exponent_row(vocab, rng):
    """2^e and 1.5 * 2^e for e = -30 .. -3: 56 levels that differ in the exponent byte, all about zero."""
    e = 2.0 ** np.arange(-30, -2)
    return _radix_row(vocab, np.concatenate([e, 1.5 * e]), rng)


# (seed, step, token) triples whose uniform is the largest (h = 2^23 - 1) or the smallest (h = 0), found by
# hashing ids 0 .. 128255 (tests/test_sampling_reference_cpu.py re-derives each h). The first five are the triples
# whose top 24 hash bits are all ones, where the 24-bit mapping that this one replaced rounded to u = 1.0f.
EXTREME_MAX = ((256, 0, 99355), (412, 0, 74883), (512, 0, 108369), (519, 0, 91357), (560, 0, 20512),
               (1051, 0, 72755), (1095, 0, 123283), (1168, 0, 104201), (1197, 0, 4220))
EXTREME_MIN = ((0, 0, 0), (43, 0, 104312), (290, 0, 70018), (358, 0, 64362), (448, 0, 127874))
# (seed, step, token with the largest u, token with the smallest u)
EXTREME_BOTH = ((308, 0, 20490, 122383), (4331, 0, 3343, 83560), (4460, 0, 58807, 34195))


def extreme_case():
    """A peaked row (temperature 1): the maximum 10 at one token, 9 and 8.5 at two more, the rest 24 below the
    maximum, and every token of the triples above 20 below it. The noise lifts a token by at most G_MAX = 16.64
    and lowers the best one by at most -G_MIN = 2.82, so none of them can win; the draws are the triples' (seed,
    step) pairs."""
    row = np.full(LLAMA_VOCAB, -14.0, dtype=np.float32)
    special = [t for tr in EXTREME_MAX + EXTREME_MIN for t in tr[2:]] + [t for tr in EXTREME_BOTH for t in tr[2:]]
    row[special] = -10.0
    free = [t for t in (7, 60001, 128255, 1234, 99999, 31) if t not in special]
    row[free[0]], row[free[1]], row[free[2]] = 10.0, 9.0, 8.5
    pairs = sorted({tr[:2] for tr in EXTREME_MAX + EXTREME_MIN + EXTREME_BOTH})
    return Case("extreme", _bf16(row), 1.0, 0, 1.0, np.array([p[0] for p in pairs], dtype=np.int64),
                np.array([p[1] for p in pairs], dtype=np.int64), prune=False)


def _topk_cases():
    out = {}
    for vocab in (1000, 32000, LLAMA_VOCAB):
        for k in (2, 5, 50, 1000):
            def make(vocab=vocab, k=k):
                rng = np.random.default_rng(vocab * 31 + k)
                return Case(f"topk_v{vocab}_k{k}", flat_topk_row(vocab, k, rng), 0.8, k, 1.0, *_draws(512, vocab + k))
            out[f"topk_v{vocab}_k{k}"] = make

    def tie():
        rng = np.random.default_rng(77)
        return Case("topk_tie4", flat_topk_row(32000, 5, rng, tie=True), 0.8, 5, 1.0, *_draws(512, 77))
    out["topk_tie4"] = tie
    return out


def _radix_cases():
    def lowbits(side):
        row = radix_lowbits_row(32000, np.random.default_rng(5))
        return Case(f"radix_lowbits_{side}", row, RADIX_T, radix_lowbits_k(row, side), 1.0, *_draws(512, 5))

    def sign():
        return Case("radix_sign", radix_sign_row(32000, np.random.default_rng(6)), RADIX_T, 20, 1.0, *_draws(512, 6))

    def exponent():
        return Case("radix_exponent", radix_exponent_row(32000, np.random.default_rng(7)), RADIX_T, 24, 1.0,
                    *_draws(512, 7))
    return {"radix_lowbits_below": lambda: lowbits("below"), "radix_lowbits_above": lambda: lowbits("above"),
            "radix_sign": sign, "radix_exponent": exponent}


def _topp_cases():
    out = {}
    for vocab in (1024, LLAMA_VOCAB):
        for t in (0.5, 1.0, 1.7):
            for target in (0.3, 0.5, 0.9, 0.95):
                name = f"topp_v{vocab}_t{t}_p{target}"

                def make(vocab=vocab, t=t, target=target, name=name):
                    row = ladder_row(vocab, t, np.random.default_rng(vocab + int(t * 10)))
                    return Case(name, row, t, 0, midpoint_p(row, t, 0, target), *_draws(512, int(target * 100)))
                out[name] = make
    return out


def _ladder(vocab=32000, t=1.0, seed=11):
    return ladder_row(vocab, t, np.random.default_rng(seed))


def _combined_cases():
    def differ():  # the cut inside the top 10 of 22 levels: over the whole row the same p keeps other levels
        row = _ladder()
        return Case("kp_differ", row, 1.0, 10, midpoint_p(row, 1.0, 10, 0.8), *_draws(512, 21))

    def loose():  # p between the top 4's mass and the top 5's: the cut is the top-k floor itself
        row = _ladder()
        _, cum = levels(row, 1.0, 5)
        return Case("kp_loose", row, 1.0, 5, float(np.float32((cum[3] + 1.0) / 2)), *_draws(512, 22))

    def k_all(name, k):
        row = _ladder(1024)
        return Case(name, row, 1.0, k, midpoint_p(row, 1.0, 0, 0.5), *_draws(512, 23))

    def p_fixed(name, p, margins=True):
        return Case(name, _ladder(1024), 1.0, 0, float(np.float32(p)), *_draws(512, 24), margins=margins)

    def gauss():  # nothing filtered on a sigma = 3 row of the full vocabulary: the draw over 50,000 candidates
        row = _bf16(np.random.default_rng(12).normal(0.0, 3.0, size=LLAMA_VOCAB))
        return Case("gauss_unfiltered", row, 0.8, 0, 1.0, *_draws(256, 25))
    return {"kp_differ": differ, "kp_loose": loose,
            "k_eq_vocab": lambda: k_all("k_eq_vocab", 1024), "k_gt_vocab": lambda: k_all("k_gt_vocab", 1029),
            "k_zero": lambda: k_all("k_zero", 0), "p_one": lambda: p_fixed("p_one", 1.0),
            "p_zero": lambda: p_fixed("p_zero", 0.0, False), "p_tiny": lambda: p_fixed("p_tiny", 1e-6, False),
            "gauss_unfiltered": gauss}


def _masked_cases():
    def masked(vocab):
        row = np.full(vocab, -np.inf, dtype=np.float32)
        row[[5, vocab // 2 + 1, vocab - 1]] = (1.0, 0.5, 0.0)
        return Case(f"masked3_v{vocab}", _bf16(row), 0.8, 50, 1.0, *_draws(512, 31))

    def all_inf():
        return Case("masked_all", _bf16(np.full(1024, -np.inf, dtype=np.float32)), 0.8, 50, float(np.float32(0.9)),
                    *_draws(64, 32))
    return {"masked3_v1024": lambda: masked(1024), f"masked3_v{LLAMA_VOCAB}": lambda: masked(LLAMA_VOCAB),
            "masked_all": all_inf}


GROUPS = {"topk": _topk_cases(), "radix": _radix_cases(), "topp": _topp_cases(), "combined": _combined_cases(),
          "masked": _masked_cases(), "extreme": {"extreme": extreme_case}}
CASES = {name: make for group in GROUPS.values() for name, make in group.items()}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, with_e32=False):
    """The oracle's draws of a case, computed once per process and shared (do not modify)."""
    return case(name).predict(with_e32)
