"""
Not a test: the float64 oracle of ops.token_logprobs (token_logprobs_kernel, csrc/kernels/sampling.hip), its
tolerance, the kernel's geometry as constants, the designed input rows and the output-level mutants that
tests/test_token_logprobs_reference_cpu.py and tests/test_logprobs_kernel_gpu.py share. Plain numpy; nothing of
src/ops/reference.py is imported.

The oracle. Per row of bf16 logits z (given as bit patterns): lp_i = z_i - logsumexp(z) in float64. Tokens are
ordered by larger logit first, then lower id; -0.0 == +0.0. `rank` counts the entries strictly before the target,
the lists are the first top_n entries in that order with their logprobs. A target outside [0, vocab) gives -inf
and rank = vocab. Rows that hold +inf or NaN, or no finite entry, are OUTSIDE the numeric contract: the oracle is
not defined on them, and the kernel test only checks that every id it writes stays in [0, vocab).

The tolerance, per output element, derived and not tuned. The kernel computes (z_t - m) - logf(S) with
S = sum __expf(z - m) in fp32; write L = log S (0 <= L <= ln vocab, every term is <= 1 and the maximum's is 1), so
|lp| = |z_t - m| + L.
  * the sum: every term passes through N_add(vocab) rounded additions, each within 2^-24 relative, so S is within
    N_add * 2^-24 relative and L within N_add * 2^-24 absolute. N_add = 8 * ceil(vocab / 8192) sequential in a
    thread (8 entries per 16-byte group, one group per 8192-entry sweep of the 1024 threads), 6 in the wave's
    butterfly, 16 across the waves;
  * the exponential: __expf(x) is the hardware's 2^y at y = fp32(x * log2 e). The scaling moves e^x by about
    1.5 |x| 2^-24 relative (the product's rounding and the constant's own), weighted in S by |x| e^x <= 1/e = 0.37
    per term; the instruction adds its own error. No accuracy figure for the instruction is in the ROCm
    documentation or headers that ship with the toolchain, so c_exp = 4 is an ASSUMPTION (the 0.37 bounds a single
    term: over a row the scaling's worst case is 1.5 A 2^-24 with A the softmax-weighted mean of |z - m|, reached
    only if every rounding errs the same way; `spread()` reports A);
  * the logarithm: logf is assumed within 1 ulp (again no figure ships): 2^-23 L. Half of it fits the last term
    below, the other half is c_log = ceil(ln vocab) >= L;
  * z_t - m is rounded once (2^-24 |z_t - m|), the final subtraction once (2^-24 |lp|), with half an ulp of L that
    makes 2^-24 (2 |z_t - m| + 2 L) = 2^-23 (|z_t - m| + L).
        tol = (N_add + c_exp + c_log) * 2^-24 + 2^-23 * (|z_t - m| + L)
The CPU test checks on every case that a plain fp32 model of the sum (`model_lse`: numpy float32 additions in the
kernel's grouping, exponentials computed in float64 and rounded once) stays within tol / 4, and that tol <= 2e-5.

Geometry of the kernel, written out (NOT read from the source): 1024 threads = 16 waves of 64 lanes; a 256-bin
window of 16-bit keys below the maximum's, four bins per lane of wave 0; the walk gives wave w the slab
[w * slab, (w + 1) * slab), slab = ceil(vocab / 8 / 16) * 8, in iterations of 2048 entries = 4 sub-chunks of 64
lanes x 8 entries. A bf16 entry's 16-bit key is bits | 0x8000 for positive and ~bits for negative values (-0.0
counts as +0.0), so a LEVEL is one bf16 value and level B - D is the D-th value below B.
"""

from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

THREADS, WAVES, LANES = 1024, 16, 64
WINDOW = 256            # 16-bit keys below the maximum's that the histogram covers
SWEEP_SUM = 8192        # entries per sweep of the sum pass (x 4 in flight = 32768)
SWEEP_MAX = 65536       # entries per eight-deep sweep of row_argmax
WALK, SUB = 2048, 512   # the walk's iteration and its sub-chunk
C_EXP = 4.0             # assumption, see above
MAX_TOP = 20

MUTATIONS = ("tie_high", "negzero_below", "roundrobin", "lanemajor", "tie_displaces", "next_level", "id_order",
             "rank_both", "rank_none", "sum_drop_chunk", "rank_drop_chunk", "max_first_65536", "sum_first_32768",
             "no_max_sub", "top_lp_from_target")


# ------------------------------------------------------------------------------------------------ bf16 bit patterns
def f32(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_bits(x) -> np.ndarray:
    """Round-to-nearest-even of finite fp32 values to bf16 bit patterns."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def key16(bits) -> np.ndarray:
    b = np.asarray(bits, dtype=np.uint16).astype(np.int64)
    b = np.where(b == 0x8000, 0, b)
    return np.where(b & 0x8000, ~b & 0xffff, b | 0x8000)


def bits_of_key16(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.int64)
    return np.where(k & 0x8000, k & 0x7fff, ~k & 0xffff).astype(np.uint16)


def slab_of(vocab: int) -> int:
    return -(-(vocab // 8) // WAVES) * 8


def n_add(vocab: int) -> int:
    return 8 * -(-vocab // SWEEP_SUM) + 6 + WAVES


def tol_const(vocab: int) -> float:
    return (n_add(vocab) + C_EXP + math.ceil(math.log(vocab))) * 2.0 ** -24


def tol_of(vocab: int, lp) -> np.ndarray:
    """The bound for outputs whose true value is lp (|lp| = |z_t - m| + L); -inf outputs are compared exactly."""
    a = np.abs(np.asarray(lp, dtype=np.float64))
    return tol_const(vocab) + 2.0 ** -23 * np.where(np.isfinite(a), a, 0.0)


# ----------------------------------------------------------------------------------------------------- the oracle
def _lsm(z: np.ndarray):
    m = z.max()
    with np.errstate(divide="ignore", invalid="ignore"):
        big_l = math.log(np.exp(z - m).sum())
        return (z - m) - big_l, m, big_l


def _order(z: np.ndarray) -> np.ndarray:
    return np.lexsort((np.arange(z.size), -z))       # -z maps -0.0 and +0.0 to equal keys


def oracle(bits: np.ndarray, targets, top_n: int, mutation: str = None):
    """bits uint16 [R, V], targets [R] -> (lp f64 [R], rank i64 [R], top_lp f64 [R, top_n], top_id i64 [R, top_n]).
    `mutation` names one of MUTATIONS: the same outputs as a kernel with that defect would give them."""
    assert mutation is None or mutation in MUTATIONS
    bits = np.asarray(bits, dtype=np.uint16)
    rows, vocab = bits.shape
    lp = np.full(rows, -np.inf)
    rank = np.full(rows, vocab, dtype=np.int64)
    top_lp = np.zeros((rows, top_n))
    top_id = np.zeros((rows, top_n), dtype=np.int64)
    for r in range(rows):
        z = f32(bits[r]).astype(np.float64)
        t = int(targets[r])
        ok = 0 <= t < vocab
        lsm, _, _ = _lsm(z)
        if mutation is not None:
            lsm = _mutant_lsm(mutation, z, lsm, t if ok else None)
        zo = z
        if mutation == "negzero_below":
            zo = np.where(bits[r] == 0x8000, -5e-324, z)
        order = np.lexsort((-np.arange(vocab), -zo)) if mutation == "tie_high" else _order(zo)
        ids = order[:top_n]
        if mutation is not None and top_n > 0:
            ids = _mutant_ids(mutation, z, order, top_n)
        top_id[r] = ids
        top_lp[r] = lsm[ids]
        if ok:
            lp[r] = lsm[t]
            before = (zo > zo[t]) | ((zo == zo[t]) & ((np.arange(vocab) > t) if mutation == "tie_high"
                                                     else (np.arange(vocab) < t)))
            if mutation == "rank_both":
                before = (z >= z[t]) & (np.arange(vocab) != t)
            elif mutation == "rank_none":
                before = z > z[t]
            elif mutation == "rank_drop_chunk":
                per = before.reshape(-1, 8).sum(1)
                c = int(np.argmin(np.where(per > 0, per, vocab)))   # the chunk whose loss shows least
                before = before.copy()
                before[8 * c:8 * c + 8] = False
            rank[r] = int(before.sum())
            if mutation == "top_lp_from_target":
                top_lp[r] = lsm[t]
    return lp, rank, top_lp, top_id


def _mutant_lsm(mutation: str, z, lsm, t):
    vocab = z.size
    m = z.max()
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        if mutation == "sum_drop_chunk":                 # the chunk whose loss shows least
            mass = np.exp(z - m).reshape(-1, 8).sum(1)
            return (z - m) - math.log(mass.sum() - mass.min())
        if mutation == "sum_first_32768":
            return (z - m) - math.log(np.exp(z[:4 * SWEEP_SUM] - m).sum())
        if mutation == "max_first_65536":                # modelled in fp32: the terms above the wrong max overflow
            m2 = z[:SWEEP_MAX].max()
            s = np.exp(z - m2).astype(np.float32).sum(dtype=np.float32)
            return ((z - m2) - np.log(s.astype(np.float64)))
        if mutation == "no_max_sub":                     # modelled in fp32
            s = np.exp(z).astype(np.float32).sum(dtype=np.float32)
            return z - np.log(s.astype(np.float64))
    return lsm


def _mutant_ids(mutation: str, z, order, top_n: int):
    """The list of a kernel that places its threshold ties (or its threshold) wrongly."""
    vocab = z.size
    base = order[:top_n]
    if mutation == "id_order":
        return np.sort(base)
    if mutation not in ("roundrobin", "lanemajor", "tie_displaces", "next_level"):
        return base
    zt = z[order[top_n - 1]]
    above = order[z[order] > zt]
    ties = np.flatnonzero(z == zt)
    need = top_n - above.size
    if mutation == "next_level":
        rest = order[z[order] != zt]
        return rest[:top_n] if rest.size >= top_n else base
    if mutation == "tie_displaces":
        if above.size == 0 or ties.size < need + 1:
            return base
        picked = np.concatenate([above[:-1], ties[:need + 1]])
    else:
        slab = slab_of(vocab)
        w = ties // slab
        if mutation == "roundrobin":
            pos = np.array([np.count_nonzero(ties[:i] // slab == w[i]) for i in range(ties.size)])
            sel = np.lexsort((w, pos))
        else:
            o = ties - w * slab
            blk, q = o // WALK, o % WALK
            sel = np.lexsort((q % 8, q // SUB, (q % SUB) // 8, blk, w))
        picked = np.concatenate([above, ties[sel][:need]])
    return picked[np.lexsort((picked, -z[picked]))]


def differs(a, b, tol4) -> bool:
    """Do two results differ by an id, a rank, or a logprob by more than tol4 (a non-finite mismatch counts)?"""
    if not np.array_equal(a[1], b[1]) or not np.array_equal(a[3], b[3]):
        return True
    for x, y, t in ((a[0], b[0], tol4[0]), (a[2], b[2], tol4[1])):
        fin = np.isfinite(x) & np.isfinite(y)
        if not np.array_equal(np.isfinite(x), np.isfinite(y)) or np.any(np.abs(x[fin] - y[fin]) > t[fin]):
            return True
    return False


# ------------------------------------------------------------------------------------ the fp32 model and geometry
def model_lse(bits_row: np.ndarray) -> float:
    """L = log S with S summed in numpy float32 in the kernel's grouping: per thread its 16-byte group of every
    8192-entry sweep, entry by entry; a butterfly over the wave's 64 lanes; the 16 waves in order. Exponentials in
    float64, rounded once (the hardware exponential is c_exp's, not the model's)."""
    z = f32(bits_row).astype(np.float64)
    with np.errstate(divide="ignore"):
        e = np.exp(z - z.max()).astype(np.float32)
    sweeps = -(-z.size // SWEEP_SUM)
    e = np.concatenate([e, np.zeros(sweeps * SWEEP_SUM - z.size, np.float32)]).reshape(sweeps, THREADS, 8)
    acc = np.zeros(THREADS, np.float32)
    for k in range(sweeps):
        for j in range(8):
            acc = acc + e[k, :, j]
    v = acc.reshape(WAVES, LANES)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, np.arange(LANES) ^ o]
    s = np.float32(0)
    for w in range(WAVES):
        s = s + v[w, 0]
    return math.log(float(s))


def spread(bits_row: np.ndarray) -> float:
    """A: the softmax-weighted mean of |z - m| (the docstring's remark on c_exp)."""
    z = f32(bits_row).astype(np.float64)
    p = np.exp(z - z.max())
    d = np.where(p > 0, z.max() - z, 0.0)
    return float((p * d).sum() / p.sum())


def geometry(bits_row: np.ndarray, top_n: int) -> dict:
    """Which of the kernel's branches the row takes: the window bin of the top_n-th entry (None: fewer than top_n
    entries in the window, the radix fallback), whether the fallback's threshold is the key of -0.0 that gets
    patched, the filled low half of the threshold key, the entries above it and the ties per wave slab."""
    bits_row = np.asarray(bits_row, dtype=np.uint16)
    k = key16(bits_row)
    kmax = int(k.max())
    d = kmax - k
    whist = np.bincount(d[d < WINDOW], minlength=WINDOW)
    cum = np.cumsum(whist)
    g = {"whist": whist, "patch": False}
    if cum[-1] >= top_n:
        g["bin"] = int(np.searchsorted(cum, top_n))
        t16 = kmax - g["bin"]
    else:                                              # the radix select orders RAW keys: -0.0 one below +0.0
        g["bin"] = None
        raw = bits_row.astype(np.int64)
        k32 = np.where(raw & 0x8000, ~(raw << 16) & 0xffffffff, (raw << 16) | 0x80000000)
        t32 = int(np.sort(k32)[::-1][top_n - 1])
        g["patch"] = t32 == 0x7fffffff
        t16 = 0x8000 if g["patch"] else t32 >> 16
    g["t16"] = t16
    g["half"] = "zeros" if t16 & 0x8000 else "ones"
    g["above"] = int((k > t16).sum())
    ties = np.flatnonzero(k == t16)
    g["ties"] = ties
    g["slab_ties"] = np.bincount(ties // slab_of(bits_row.size), minlength=WAVES)
    return g


# ---------------------------------------------------------------------------------------------------- the families
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    family: str
    bits: np.ndarray          # uint16 [R, V]
    targets: np.ndarray       # int64 [R]
    top_n: int
    claims: tuple             # the mutations this case notices
    premise: tuple            # per row: a dict of expected geometry() entries (checked on the CPU)

    @property
    def vocab(self):
        return self.bits.shape[1]


K_B = 0xC100                  # the key of 8.0, the ladders' maximum
LADDER_WINDOW_D = (0, 1, 3, 4, 127, 128, 252, 255)
LADDER_FALLBACK_D = (256, 257, 5000)
VOCABS = (8, 24, 1000, 8192, 8200, 32776, 65544)

# vocab, top_n, D, a (entries above level B - D), t (entries at it), bulk
_LADDER = (
    (8, 5, 0, 0, 6, "in"), (8, 5, 3, 1, 6, "in"), (8, 8, 3, 3, 5, "in"), (24, 20, 1, 1, 19, "in"), (24, 20, 127, 19, 1, "in"),
    (1000, 1, 0, 0, 1, "in"), (1000, 5, 0, 0, 15, "far"), (1000, 5, 1, 1, 9, "in"), (1000, 20, 3, 1, 60, "far"),
    (8200, 5, 3, 3, 2, "in"), (1000, 5, 4, 4, 1, "in"), (8192, 20, 4, 1, 24, "in"), (8200, 20, 127, 19, 1, "far"),
    (1000, 5, 127, 1, 9, "in"), (8200, 5, 128, 4, 1, "in"), (1000, 20, 128, 1, 60, "far"),
    (32776, 20, 252, 19, 6, "in"), (1000, 5, 252, 1, 4, "far"), (8200, 20, 255, 1, 24, "in"),
    (65544, 5, 255, 4, 1, "far"),
    (1000, 5, 256, 1, 9, "far"), (8200, 20, 256, 19, 1, "far"), (1000, 20, 257, 1, 19, "far"),
    (32776, 5, 257, 4, 15, "far"), (8192, 5, 5000, 1, 4, "far"), (65544, 20, 5000, 19, 6, "far"),
    (24, 20, 5000, 1, 23, "far"),
)


def _scatter(vocab, rng, placed, bulk_bits, fixed=()):
    """A row: `fixed` = (position, bits) pairs, `placed` bits at random free positions, the rest from bulk_bits."""
    row = np.zeros(vocab, dtype=np.uint16)
    free = np.ones(vocab, dtype=bool)
    for p, b in fixed:
        row[p], free[p] = b, False
    spots = rng.permutation(np.flatnonzero(free))
    placed = np.asarray(placed, dtype=np.uint16)
    row[spots[:placed.size]] = placed
    rest = spots[placed.size:]
    row[rest] = bulk_bits[:rest.size]
    return row


def _ladder(idx, vocab, top_n, dist, a, t, bulk):
    rng = np.random.default_rng(7000 + idx)
    k_t = K_B - dist
    assert (a == 0) == (dist == 0) and a <= max(dist, 0) + (dist == 0) and a < top_n <= a + t and a + t <= vocab
    above = [K_B] + list(K_B - 1 - rng.permutation(dist - 1)[:a - 1]) if a else []
    n_bulk = vocab - a - t
    if bulk == "in":        # as in a real row: right below the threshold, across the window's lower edge
        bk = k_t - 1 - rng.integers(0, 300, n_bulk)
    else:                   # more than 256 levels below the maximum
        bk = min(k_t, K_B - WINDOW) - 1 - rng.integers(0, 2000, n_bulk)
    row = _scatter(vocab, rng, bits_of_key16(np.array(above + [k_t] * t)), bits_of_key16(bk))
    ties = np.flatnonzero(key16(row) == k_t)
    claims = ["next_level"] if vocab - t >= top_n else []
    if a:
        claims.append("top_lp_from_target")
    if t > top_n - a:
        claims.append("tie_high")
        if a:
            claims.append("tie_displaces")
    if a >= 19:
        claims.append("id_order")
    fallback = dist >= WINDOW
    prem = {"bin": None if fallback else dist, "patch": False, "half": "zeros", "above": a, "n_ties": t}
    return Case(f"ladder_v{vocab}_n{top_n}_D{dist}_a{a}_t{t}_{bulk}", "ladder", row[None], np.array([ties[-1]]),
                top_n, tuple(claims), (prem,))


def _neg_denormals(rng, n, lo=3, hi=200):
    return (0x8000 + rng.integers(lo, hi, n)).astype(np.uint16)


def _zero_cases():
    out = []
    pz, nz = 0x0000, 0x8000
    # the threshold on the positive side of zero: bin 3, the key's low half filled with zeros
    rng = np.random.default_rng(7100)
    v = 1000
    row = _scatter(v, rng, [5, 4, 3] + [2] * 4 + [pz] * 10 + [nz] * 10, _neg_denormals(rng, v))
    out.append(Case("zero_positive_side", "zero", row[None], np.array([int(np.flatnonzero(row == 2)[-1])]), 5,
                    ("tie_high", "next_level", "tie_displaces"),
                    ({"bin": 3, "half": "zeros", "above": 3, "n_ties": 4, "negzero_bin_empty": True},)))
    # the threshold exactly at +-0.0 (bin 5): -0.0 ties with +0.0, and -0.0 entries come first by id
    rng = np.random.default_rng(7101)
    v = 8200
    fixed = [(10, nz), (11, pz), (500, nz), (501, nz), (3000, pz), (8191, pz), (8192, nz), (8199, pz)]
    row = _scatter(v, rng, [5, 4, 3], _neg_denormals(rng, v), fixed)
    out.append(Case("zero_at_zero", "zero", row[None], np.array([501]), 5, ("tie_high", "negzero_below", "next_level"),
                    ({"bin": 5, "half": "zeros", "above": 3, "n_ties": 8, "negzero_bin_empty": True},)))
    # the threshold below zero: bin 8 = 6 levels down to -0.0's own (empty) bin, then bits 0x8001 and 0x8002
    rng = np.random.default_rng(7102)
    v = 1000
    fixed = [(20, nz), (21, pz), (22, nz), (600, pz), (601, nz), (999, pz)]
    row = _scatter(v, rng, [5, 4, 3, 2, 1] + [0x8001] * 2 + [0x8002] * 12, _neg_denormals(rng, v), fixed)
    out.append(Case("zero_negative_side", "zero", row[None], np.array([601]), 20,
                    ("tie_high", "negzero_below", "next_level", "tie_displaces"),
                    ({"bin": 8, "half": "ones", "above": 13, "n_ties": 12, "negzero_bin_empty": True},)))
    # through the fallback: the maximum 1.0 and 0.5, zeros, the bulk far below. Row 0: the 5th raw key is a +0.0's;
    # row 1: it is a -0.0's (0x7fffffff, patched to +0.0's); row 2: the threshold is -1.0 (low half ones)
    v = 1000
    rows, prem = [], []
    for i, (n_pz, n_nz) in enumerate(((4, 4), (2, 6), (1, 1))):
        rng = np.random.default_rng(7103 + i)
        extra = [0xbf80] * 6 if i == 2 else []
        rows.append(_scatter(v, rng, [0x3f80, 0x3f00] + extra, bits_of_key16(key16(0xc000) - rng.integers(0, 500, v)),
                             [(100 + 7 * j, nz if j % 2 == 0 else pz) for j in range(2 * min(n_pz, n_nz))]
                             + [(300 + 5 * j, nz if n_nz > n_pz else pz) for j in range(abs(n_nz - n_pz))]))
        prem.append({"bin": None, "patch": i == 1, "half": "ones" if i == 2 else "zeros",
                     "above": 4 if i == 2 else 2, "n_ties": 6 if i == 2 else 8})
    out.append(Case("zero_fallback", "zero", np.stack(rows), np.array([107, 305, 100]), 5,
                    ("tie_high", "negzero_below", "next_level"), tuple(prem)))
    return out


def _slab_row(seed, vocab, a, tie_pos):
    rng = np.random.default_rng(seed)
    k_t = K_B - 40
    above = [K_B] + list(K_B - 1 - rng.permutation(39)[:a - 1])
    return _scatter(vocab, rng, bits_of_key16(np.array(above)), bits_of_key16(k_t - 1 - rng.integers(0, 300, vocab)),
                    [(p, int(bits_of_key16(k_t))) for p in tie_pos])


def _slab_cases():
    out = []

    def add(name, seed, vocab, top_n, a, tie_pos, claims, slab_ties):
        row = _slab_row(seed, vocab, a, tie_pos)
        out.append(Case("slabs_" + name, "slabs", row[None], np.array([max(tie_pos)]), top_n, claims,
                        ({"bin": 40, "above": a, "n_ties": len(tie_pos), "slab_ties": slab_ties},)))

    def per_slab(vocab, pos):
        return tuple(np.bincount(np.array(pos) // slab_of(vocab), minlength=WAVES).tolist())

    # slab 64 at vocab 1000: the last index of wave 3's slab and the first of wave 4's; the ragged wave 15
    pos = [255, 256, 700, 900]
    add("edge_1000", 7200, 1000, 5, 3, pos, ("tie_high",), per_slab(1000, pos))
    pos = [961, 975, 990, 999]
    add("ragged_1000", 7201, 1000, 5, 3, pos, ("tie_high",), per_slab(1000, pos))
    # slab 520 at vocab 8200: wave 15 owns [7800, 8200)
    s = slab_of(8200)
    pos = [w * s + (37 * w) % min(s, 8200 - w * s) for w in range(WAVES)]
    add("each_8200", 7202, 8200, 20, 10, pos, ("tie_high", "tie_displaces"), (1,) * WAVES)
    pos = [3, 9, 17, 100, 200, 300, 400, 519] + [5 * s + o for o in (0, 8, 64, 65, 300, 511, 512, 519)]
    add("many_8200", 7203, 8200, 5, 1, pos, ("tie_high", "roundrobin"), per_slab(8200, pos))
    pos = [100, 519] + [5 * s + o for o in (0, 8, 64, 65, 300, 511, 512, 519)]
    add("split_8200", 7204, 8200, 5, 1, pos, ("tie_high",), per_slab(8200, pos))
    pos = [7800, 8191, 8192, 8199]
    add("ragged_8200", 7205, 8200, 5, 3, pos, ("tie_high",), per_slab(8200, pos))
    # slab 2056 at vocab 32776: one 2048-entry iteration and 8 entries of a second. Wave 2's slab starts at 4112:
    # index order meets lane 1 of sub-chunk 0 (offset 8) before lane 0 of sub-chunk 1 (offset 512)
    s = slab_of(32776)
    pos = [2 * s + o for o in (8, 16, 512, 1024 + 43, 1536, 2048, 2055)]
    add("lane_32776", 7206, 32776, 5, 3, pos, ("tie_high", "lanemajor"), per_slab(32776, pos))
    rng = np.random.default_rng(7207)
    pos = sorted((7 * s + rng.permutation(WALK)[:30]).tolist())
    add("lanes_32776", 7208, 32776, 20, 4, pos, ("tie_high", "lanemajor"), per_slab(32776, pos))
    return out


def _rank_cases():
    out = []
    hi, mid, lo = 0x4000, 0x3f80, 0x3f00
    for v in (1000, 8200):
        rng = np.random.default_rng(7300 + v)
        row = np.array([hi, mid, lo], dtype=np.uint16)[rng.integers(0, 3, v)]
        row[0] = row[v - 1] = row[v // 2] = mid
        out.append(Case(f"rank_ties_{v}", "rank", np.stack([row] * 3), np.array([0, v - 1, v // 2]), 5,
                        ("rank_both", "rank_none", "tie_high"), ()))
        flat = np.full((1, v), 0x3fc0, dtype=np.uint16)
        out.append(Case(f"rank_flat_{v}", "rank", flat, np.array([v - 1]), 0, ("rank_none", "rank_drop_chunk"), ()))
    v = 1000
    rng = np.random.default_rng(7301)
    row = np.where(rng.random(v) < 0.5, 0x0000, _neg_denormals(rng, v, 0x100, 0x4000)).astype(np.uint16)
    row[7], row[400], row[500], row[600] = 0x3f80, 0x8000, 0x8000, 0x8000
    out.append(Case("rank_negzero", "rank", row[None], np.array([500]), 5,
                    ("negzero_below", "rank_both", "rank_none"), ()))
    rng = np.random.default_rng(7302)
    row = bf16_bits(rng.standard_normal(v) * 4)
    dead = rng.random(v) < 0.9
    row[dead] = 0xff80
    rows = np.stack([row] * 3)
    out.append(Case("rank_minus_inf", "rank", rows, np.array([int(np.flatnonzero(dead)[40]), -1, v]), 5,
                    ("rank_both", "rank_none"), ()))
    return out


def _mass_cases():
    out = []
    for v in (8200, 32776, 65544):
        rng = np.random.default_rng(7400 + v)
        row = np.where(rng.random(v) < 0.5, 0x3f80, 0x3f7f).astype(np.uint16)
        claims = ("sum_drop_chunk",) + (("sum_first_32768",) if v > 4 * SWEEP_SUM else ())
        out.append(Case(f"mass_flat_{v}", "mass", row[None], np.array([v - 3]), 5, claims, ()))
    v = 65544                      # the maximum in the group past row_argmax's eight-deep sweep
    rng = np.random.default_rng(7401)
    row = bf16_bits(-45.0 + rng.random(v))
    row[v - 4] = bf16_bits(50.0)
    out.append(Case("mass_last_group_65544", "mass", row[None], np.array([v - 4]), 1, ("max_first_65536",), ()))
    v = 8200
    rng = np.random.default_rng(7402)
    row = bf16_bits(100.0 + 20.0 * rng.random((2, v)))
    out.append(Case("mass_loud_8200", "mass", row, np.array([17, v - 1]), 5, ("no_max_sub",), ()))
    return out


def _random_cases():
    rng = np.random.default_rng(7500)
    row = bf16_bits(rng.standard_normal((3, 8200)) * 4)
    return [Case("random_8200", "random", row, np.array([0, 8199, 4100]), 20, ("top_lp_from_target", "id_order"), ())]


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = [_ladder(i, *spec) for i, spec in enumerate(_LADDER)]
    out += _zero_cases() + _slab_cases() + _rank_cases() + _mass_cases() + _random_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case_names():
    return [c.name for c in cases()]


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """The oracle's outputs of a case and their tolerances (lp's, the lists'), computed once."""
    c = by_name(name)
    res = oracle(c.bits, c.targets, c.top_n)
    return res, (tol_of(c.vocab, res[0]), tol_of(c.vocab, res[2]))
