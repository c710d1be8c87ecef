"""Not a test: the float64 oracle of the decode GEMM (csrc/kernels/gemm_decode.hip), its tolerances, its seeded
input families and the case lists that test_gemm_decode_reference_cpu.py (which judges all of this on the CPU)
and test_gemm_decode_kernel_gpu.py (which judges the kernel by it) share.

Oracle. Plain float64 torch from the tensors exactly as the kernel receives them: y = x w^T; the split-K partials
y[by] over the K-chunks [by * tch // ny, (by + 1) * tch // ny), tch = K / kc (the kernel's split rule, restated in
slices() and not imported); the SiLU pairing w = [gate; up], silu(g r) * (u r); the row scale
r = (sum_t ssp[t, m] / K + eps)^-1/2; mode 3's h = bf16(resid + sum_by y[by]) with the per-tile row sums of
squares of h; mode 0's greedy candidates (per row and wr-column tile the maximum of the rounded outputs and the
lowest column that attains it); the grouped form's offsets, segments and gathered rows. The launcher's image rule
(the smallest of 16 / 32 / 64 / 128 rows that holds M and exists for the tile, 16 only with nt) is restated in
select_xr(); the geometry (GD_TILES, gd_tile_valid, ring_slots) comes from src/ops/decode_tiles.py, so a tile added
there gets its cases here without an edit.

Integer family (exact). x in {+-1}, w in +-{1..a} (a = 3 up to K = 512, 1 above; the SiLU modes change over at
K = 320, see below), resid in +-{1..4}: no zeros, so
leaving out or doubling any one product moves the exact result by >= 1. conditions() asserts per case that
sum_k |x w| < 2^24 for every output, that |y|, |h| <= 256 wherever a bf16 value is written and that ss < 2^24.
Every product and every partial sum in any order is then an integer that fp32 holds exactly, and every bf16 value
written is an integer of at most 9 bits, so the kernel has to equal the oracle (fp32 slabs, ss) and
RNE_bf16(oracle) (modes 0 and 3) bit for bit: the GPU test uses torch.equal. The ring sweep runs in mode 2, where
only the 2^24 bound applies. Cases that write bf16 keep K small: at most 1,280 with one slice, except the one tile
whose wrapped ring needs 7 x 256 = 1,792, and at most 9 chunks (2,304) when split; conditions() holds for each.

SiLU modes (1, 4, 6). g and u are exact integers; left are the row scale, the fast exp, a division, two
multiplies by r and the bf16 rounding. In units of 2^-23 (one fp32 ulp, relative): r costs 0.5 (the constant 1 / K)
+ 0.5 (t / K) + 0.5 (+ eps), halved by the square root, + 1 for rsqrtf (v_rsq_f32: 1 ulp) = 1.75; z = g r
another 0.5, and silu(z) = z sigma(z) moves by at most (1 + |z|) times the relative error of z:
2.25 (1 + |z|). u r: 2.25. __expf(-z) = exp2(-z log2 e): the rounded product and the rounded constant move the
argument by <= 1.5 * 2^-24 |z| log2 e, the result by 0.75 |z|, + 1 for v_exp_f32 (1 ulp), and the denominator
1 + E damps E's error by E / (1 + E) <= 1: 0.75 |z| + 1. The add 1 + E: 0.5. The division: 2.5 (the documented
bound of the fast fp32 divide; 0.5 where it is correctly rounded). The last multiply: 0.5. Sum:
3 (1 + |z|) + 6.75 <= 9.75 (1 + |z|), so c = C_SILU = 10 and y is accepted iff
|y - o| <= half a bf16 ulp at o + c 2^-23 (1 + |g r|) |o|. Mode 1 is the same with r = 1 exactly.
Below z = -88.72 the fast exp overflows and the kernel takes (z u r) e^z with the exponent lifted by 64 (silu_mul
in the kernel): two multiplies and an exact power of two in place of the add and the division, and an fma'd
argument that is off by <= 2^-18 + 1.5 * 2^-24 |z| log2 e, which is less than the 0.75 |z| already counted once
|z| > 88; the same c covers it. Mode 1 reaches z = -150 and so runs that branch down into bf16's subnormals; it
was added because of these cases (before, the quotient flushed to -0 where the oracle is up to 1e-35: up to 480
tol on up to 189 elements of a case).
An element is insensitive if a change of g or of u by +-1 moves the oracle by <= 4 tol (u = 0, g = 0, |g| or
|u| > 128, the minimum of silu); sensitivity() measures it with all four changes, the caps are 10 % of a case and
25 % of any row or column. Four tol are 2^-7 .. 2^-6 of |o| depending on o's mantissa, so |g| or |u| in 64 .. 128
already counts in part; measured with x = +-1 on 128 x 192 outputs at r = 1, the insensitive share is 6.0 / 4.5 /
3.9 / 5.8 % for +-{1,2,3} at K = 32 / 64 / 128 / 256 but 10.6 / 16.1 % at 384 / 512, and 9.6 / 8.2 / 7.4 / 7.3 /
9.0 % for +-1 at 256 / 384 / 512 / 1,024 / 1,280 but 11.0 / 12.9 % at 1,536 / 1,792 (26 / 19 / 14 % at 32 / 64 /
128). So the SiLU cases take a = 3 up to K = 320 and a = 1 above, and keep K <= 1,280: their longer ring is
min(S + 1, 1,280 / kc) chunks, which stops short of a wrap only for (32, 256) at 16 rows (S = 6; the ring sweep and
mode 0 wrap that ring). The caps on a 16-row column or a 48-column row are 4 and 12 elements, which a draw
misses by chance: SEEDS lists the cases whose numbered seed did.
The statistics are integer-valued tiles with one witness tile per row that holds 3/4 of the row's sum;
the witness rotates with the row over the tile indices 0, 1, NSL - 1, NSL, tiles - 2, tiles - 1 and a seeded one
(NSL = 256 / RR the kernel's slice count), so a dropped, doubled or clamped-in tile moves r by far more than tol.
The row sum is K^2 var(w) / 49 or twice that (more where many tiles need it), so that z = g r has a standard
deviation of about 5 - 7 (modes 4 and 6 stay far from the overflow of the fast exp) and few elements sit on the
minimum of silu.

Random family (one case per epilogue): bf16 randn x, randn / sqrt(K) w. An fp32 slab element is accepted within
E = (K + sk) 2^-24 sum_k |x w| (every product added one at a time: the worst any order can do), a bf16 output
within that plus half an ulp; through SiLU E is carried by the mean-value theorem (sup |silu'| < 1.1).

Case lists. Every (wr, kc, XR) that gd_tile_valid allows, three column tiles. An image is selected by M, so "M at
the top of the image and at 1" is M = XR and the smallest M that still selects XR (1 where no smaller image
exists, or 1 without nt for the 32-row image). The split epilogues (modes 3 and 6) take slices of one chunk and
longer slices (up to S + 1 chunks each, 17 in all, K bounded as above) alternately over the split counts and the
tiles instead of both for each: every split count, both slice lengths and both layouts appear for every wr, at a
quarter of the launches. Mode 4's statistics tile counts alternate between one chunk and the longer ring likewise.

Poison and sentinels are the GPU test's part: it places these tensors in NaN-filled and sentinel-filled buffers.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Optional

import torch

from src.ops.decode_tiles import GD_TILES, SSP_LD, gd_tile_valid, ring_slots

XRS = (16, 32, 64, 128)
NTILES = 3              # column tiles of every case: bx = 0, 1, 2 and N no power of two
EPS = 2.0 ** -16
C_SILU = 10.0
U23 = 2.0 ** -23
HALF_RING_BYTES = 76 * 1024
SILU_MODES = (1, 4, 6)
IMAGE_MS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)
IMAGE_TILES = ((64, 256), (64, 64), (128, 128))  # waves split K / columns / rows (by image) between them
SENT = 12352.0          # sentinel of the output buffers (a bf16 value no case produces)
SENT_I = -7777

VALID = tuple((wr, kc, xr) for wr, kc in GD_TILES for xr in XRS if gd_tile_valid(wr, kc, xr))


def select_xr(wr: int, kc: int, m: int, nt: bool) -> Optional[int]:
    """The activation image of a launch: the smallest that holds m rows and exists, 16 only with nt; None = the
    launch is refused."""
    for xr in XRS:
        if m <= xr and (xr != 16 or nt) and gd_tile_valid(wr, kc, xr):
            return xr
    return None


def slices(k: int, kc: int, sk: int):
    """[(k_lo, k_hi)] of the sk split-K slices."""
    tch = k // kc
    return [((by * tch // sk) * kc, ((by + 1) * tch // sk) * kc) for by in range(sk)]


def half_ring_slots(wr: int, kc: int, xr: int) -> int:
    """Ring depth of the half-LDS form, 0 = none (restated from gd_tiles.h with the launcher's LDS condition)."""
    slot = (wr + xr) * kc * 2
    s = min(ring_slots(wr, kc, xr), HALF_RING_BYTES // slot)
    red = (4 if xr < 64 and kc >= 128 else 1) * max(xr, 32) * wr * 4 + 2048
    return s if s >= 2 and xr <= 32 and max(s * slot, red) <= HALF_RING_BYTES else 0


def amax_ok(wr: int) -> bool:
    return wr % 8 == 0 and (wr // 8) & (wr // 8 - 1) == 0


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                 # ring | image | epi | grouped | random
    wr: int
    kc: int
    xr: Optional[int]         # the image the launcher has to select; None: the launch is refused
    mode: int
    sk: int = 1
    tch: int = 1              # K-chunks in all
    seed: int = 0
    rows: tuple = ()          # ((M, nt), ...): the launches
    amax: bool = False        # mode 0: also through gemm_decode_argmax
    half_ring: bool = False
    tiles: int = 0            # statistics tiles (modes 4, 6)
    family: str = "int"
    segs: int = 1             # grouped
    gather: bool = False
    counts: tuple = ()

    @property
    def k(self) -> int:
        return self.tch * self.kc

    @property
    def silu(self) -> bool:
        return self.mode in SILU_MODES

    @property
    def no(self) -> int:      # output columns per column tile
        return self.wr // 2 if self.silu else self.wr

    @property
    def n(self) -> int:
        return NTILES * self.no

    @property
    def amp(self) -> int:
        return 3 if self.k <= (320 if self.silu else 512) else 1

    @property
    def mx(self) -> int:
        return max(m for m, _ in self.rows)

    @property
    def rr(self) -> int:
        return max(32, self.xr)

    @property
    def refused(self) -> bool:
        return self.xr is None


# ---------------------------------------------------------------------------------------------- case lists

def _rows_for(wr, kc, xr, nts=(True, False)):
    """Launches that select image xr: M at the top of the image and the smallest M that still selects it."""
    top = next(((xr, nt) for nt in nts if select_xr(wr, kc, xr, nt) == xr), None)
    low = next(((m, nt) for m in range(1, xr + 1) for nt in nts if select_xr(wr, kc, m, nt) == xr), None)
    assert top is not None and low is not None
    return (top,) if top == low else (top, low)


def _tile_counts(xr):
    nsl = 256 // max(32, xr)
    return (1, 2, nsl, nsl + 1, 255, 256) if xr <= 32 else (1, 127, 128)


def _big(sk, s, kc):
    """Chunks of a split case whose slices run more than one chunk, bounded so that a bf16 output stays small."""
    return min(sk * (s + 1), 17, max(sk + 1, 1280 // kc))


def _silu_wrap(s, kc):
    """Chunks of the longer SiLU cases: a wrapped ring (S + 1), but K <= 1,280 (the sensitivity caps need it)."""
    return min(s + 1, 1280 // kc)


def _build():
    ring, image, epi, grouped, random = [], [], [], [], []
    for wr, kc, xr in VALID:
        s = ring_slots(wr, kc, xr)
        t = f"{wr}x{kc}-x{xr}"
        cfgs = [(1, n) for n in sorted({1, 2, s - 1, s, s + 1, 2 * s + 1}) if n >= 1] + [(2, 3), (3, 4), (3, 5)]
        for sk, tch in cfgs:
            ring.append(Case(f"ring-{t}-s{sk}t{tch}", "ring", wr, kc, xr, 2, sk, tch, rows=_rows_for(wr, kc, xr)))
        for tch in (1, s + 1):
            # the candidate entry point always loads nt: rows that select xr with nt
            epi.append(Case(f"epi0-{t}-t{tch}", "epi", wr, kc, xr, 0, 1, tch, amax=True,
                            rows=_rows_for(wr, kc, xr, (True,))))
        for tch in (1, _silu_wrap(s, kc)):
            epi.append(Case(f"epi1-{t}-t{tch}", "epi", wr, kc, xr, 1, 1, tch, rows=_rows_for(wr, kc, xr)))
        counts = _tile_counts(xr)
        for i, tc in enumerate(counts):
            tch = (1, _silu_wrap(s, kc))[i % 2]
            epi.append(Case(f"epi4-{t}-t{tch}-n{tc}", "epi", wr, kc, xr, 4, 1, tch, tiles=tc,
                            rows=_rows_for(wr, kc, xr)))
        # split cases: slices of one chunk and slices of several alternate over the split counts and the tiles
        vi = VALID.index((wr, kc, xr))
        for j, sk in enumerate((1, 2, 3, 4)):
            tch = (sk, _big(sk, s, kc))[(j + vi) % 2]
            epi.append(Case(f"epi6-{t}-s{sk}t{tch}", "epi", wr, kc, xr, 6, sk, tch,
                            tiles=counts[(j + vi) % len(counts)], rows=_rows_for(wr, kc, xr)))
        if wr in (32, 64, 128):
            for j, sk in enumerate((1, 2, 3, 4, 5, 8)):
                tch = (sk, _big(sk, s, kc))[(j + vi) % 2]
                epi.append(Case(f"epi3-{t}-s{sk}t{tch}", "epi", wr, kc, xr, 3, sk, tch, rows=_rows_for(wr, kc, xr)))
            hs = half_ring_slots(wr, kc, xr)
            if hs and select_xr(wr, kc, xr, True) == xr:
                for sk in (1, 2):
                    tch = _big(sk, hs, kc)
                    epi.append(Case(f"epi3h-{t}-s{sk}t{tch}", "epi", wr, kc, xr, 3, sk, tch, half_ring=True,
                                    rows=_rows_for(wr, kc, xr, (True,))))
        # grouped: groups that are empty and of 1, xr - 1 and xr rows; segments and gather alternate
        for j, mode in enumerate((0, 1)):
            v = (VALID.index((wr, kc, xr)) + j) % 4
            grouped.append(Case(f"grp{mode}-{t}", "grouped", wr, kc, xr, mode, 1, (1, _silu_wrap(s, kc))[v % 2],
                                rows=((xr, True),), segs=1 + v % 2, gather=v >= 2,
                                counts=(0, 1, xr - 1, xr, 0, 3)))
    for wr, kc in IMAGE_TILES:
        for m in IMAGE_MS:
            for nt in (True, False):
                image.append(Case(f"img-{wr}x{kc}-m{m}-{'nt' if nt else 'ld'}", "image", wr, kc,
                                  select_xr(wr, kc, m, nt), 2, 1, 2, rows=((m, nt),)))
    # magnitudes like the workload's: one case per epilogue at 33 rows (the 64-row image) and 8 chunks
    for mode, wr, kc, sk in ((0, 128, 128, 1), (1, 112, 128, 1), (2, 96, 128, 4), (3, 64, 128, 4), (4, 128, 64, 1),
                             (6, 64, 128, 2)):
        random.append(Case(f"rand{mode}-{wr}x{kc}", "random", wr, kc, 64, mode, sk, 8, rows=((33, True),),
                           tiles=5 if mode in (4, 6) else 0, amax=mode == 0, family="random"))
    out = []
    for i, c in enumerate(ring + image + epi + grouped + random):
        out.append(replace(c, seed=SEEDS.get(c.name, 1000 + i)))
    return out


# name -> seed where the numbered seed (1000 + position in the list) misses conditions() or a sensitivity cap: the
# first of seed + 5000 j that meets them (the caps on a 16-row column or a 48-column row are 4 and 12 elements)
SEEDS: dict = {'epi1-128x32-x64-t1': 7125,
 'epi1-48x256-x16-t1': 6501,
 'epi1-64x128-x16-t8': 6726,
 'epi1-96x128-x16-t1': 11803,
 'epi4-112x128-x16-t1-n255': 26859,
 'epi4-112x128-x16-t1-n8': 11857,
 'epi4-112x128-x16-t5-n2': 51856,
 'epi4-112x128-x16-t5-n256': 66860,
 'epi4-112x128-x16-t5-n9': 121858,
 'epi4-112x128-x32-t5-n256': 6874,
 'epi4-112x128-x32-t5-n9': 6872,
 'epi4-128x128-x16-t1-n255': 6909,
 'epi4-128x128-x16-t1-n8': 66907,
 'epi4-128x128-x16-t5-n2': 11906,
 'epi4-128x128-x16-t5-n256': 11910,
 'epi4-128x128-x16-t5-n9': 26908,
 'epi4-128x128-x32-t1-n255': 6931,
 'epi4-128x32-x64-t1-n128': 7129,
 'epi4-128x64-x32-t1-n1': 7037,
 'epi4-128x64-x32-t1-n8': 7039,
 'epi4-128x64-x32-t8-n2': 7038,
 'epi4-128x64-x32-t8-n9': 7040,
 'epi4-32x128-x16-t9-n9': 11602,
 'epi4-32x256-x16-t1-n1': 6442,
 'epi4-32x256-x16-t5-n2': 6443,
 'epi4-32x256-x16-t5-n256': 31447,
 'epi4-32x256-x16-t5-n9': 6445,
 'epi4-32x256-x32-t5-n9': 6467,
 'epi4-48x128-x16-t1-n1': 6677,
 'epi4-48x128-x16-t9-n9': 6680,
 'epi4-48x256-x16-t1-n1': 6503,
 'epi4-48x256-x16-t1-n255': 6507,
 'epi4-64x128-x16-t1-n8': 6729,
 'epi4-64x128-x16-t8-n2': 11728,
 'epi4-64x128-x16-t8-n256': 6732,
 'epi4-64x128-x16-t8-n9': 6730,
 'epi4-64x128-x32-t7-n2': 6750,
 'epi4-64x256-x16-t1-n8': 6544,
 'epi4-64x256-x16-t4-n256': 11547,
 'epi4-64x256-x16-t4-n9': 6545,
 'epi4-64x32-x64-t1-n128': 7095,
 'epi4-96x128-x16-t1-n255': 6809,
 'epi4-96x128-x32-t5-n2': 6820,
 'epi4-96x128-x32-t5-n256': 11824,
 'epi6-112x128-x16-s1t5': 46861,
 'epi6-112x128-x16-s2t2': 26862,
 'epi6-112x128-x16-s3t10': 116863,
 'epi6-112x128-x16-s4t4': 11864,
 'epi6-112x128-x32-s4t10': 16878,
 'epi6-128x128-x16-s3t10': 71913,
 'epi6-128x128-x16-s4t4': 16914,
 'epi6-128x128-x32-s4t10': 11936,
 'epi6-32x128-x128-s4t10': 6666,
 'epi6-32x128-x16-s1t9': 6605,
 'epi6-32x128-x16-s4t4': 6608,
 'epi6-32x128-x64-s3t10': 16648,
 'epi6-32x256-x16-s2t5': 6449,
 'epi6-32x256-x16-s3t3': 11450,
 'epi6-48x128-x16-s1t9': 41683,
 'epi6-48x128-x16-s3t10': 11685,
 'epi6-48x128-x32-s2t10': 11698,
 'epi6-48x256-x16-s2t2': 6510,
 'epi6-48x256-x32-s2t5': 11524,
 'epi6-64x128-x16-s1t8': 6733,
 'epi6-64x128-x32-s1t1': 6755,
 'epi6-64x128-x32-s2t10': 11756,
 'epi6-64x128-x32-s3t3': 6757,
 'epi6-64x128-x32-s4t10': 11758,
 'epi6-64x256-x16-s1t1': 11548,
 'epi6-64x256-x16-s2t5': 11549,
 'epi6-64x256-x16-s4t5': 6551,
 'epi6-64x256-x64-s2t5': 16586,
 'epi6-96x128-x16-s3t10': 46813,
 'epi6-96x128-x16-s4t4': 6814,
 'epi6-96x128-x32-s3t3': 6827,
 'epi6-96x128-x32-s4t10': 66828,
 'grp1-32x256-x16': 7158}

ALL = _build()
CASES = {c.name: c for c in ALL}
assert len(CASES) == len(ALL)
RING_CASES = [c.name for c in ALL if c.kind == "ring"]
IMAGE_CASES = [c.name for c in ALL if c.kind == "image"]
EPI_CASES = [c.name for c in ALL if c.kind == "epi"]
GROUPED_CASES = [c.name for c in ALL if c.kind == "grouped"]
RANDOM_CASES = [c.name for c in ALL if c.kind == "random"]
# launches that must raise the launcher's error: no image for that M, candidates on a wr / 8 that is no power of two
REFUSED_LAUNCHES = [c.name for c in ALL if c.refused]
REFUSED_AMAX = [c.name for c in ALL if c.amax and not amax_ok(c.wr)]


def case(name: str) -> Case:
    return CASES[name]


# ---------------------------------------------------------------------------------------------- inputs

def _signed(gen, shape, a):
    mag = torch.randint(1, a + 1, shape, generator=gen)
    return (mag * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).to(torch.bfloat16)


def witness_positions(tiles: int, rr: int, seeded: int):
    nsl = 256 // rr
    pos = []
    for p in (0, 1, nsl - 1, nsl, tiles - 2, tiles - 1, seeded % tiles):
        if 0 <= p < tiles and p not in pos:
            pos.append(p)
    return pos


def make_ssp(c: Case, rows: int, gen, unit: bool = False) -> torch.Tensor:
    """[tiles, SSP_LD] fp32 statistics of `rows` rows (the others NaN): integers, witness tile = 3/4 of the row."""
    var = 14.0 / 3.0 if c.amp == 3 else 1.0
    b0 = max(c.tiles, c.k // 4) if unit else max(c.tiles, round(c.k * c.k * var / 196))
    ssp = torch.full((c.tiles, SSP_LD), float("nan"), dtype=torch.float32)
    pos = witness_positions(c.tiles, c.rr, int(torch.randint(0, 1 << 20, (1,), generator=gen)))
    bm = torch.randint(1, 3, (rows,), generator=gen) * b0
    if c.tiles == 1:
        ssp[0, :rows] = (4 * bm).float()
        return ssp
    wt = torch.tensor(pos)[torch.arange(rows) % len(pos)]                 # [rows]
    t = torch.arange(c.tiles)[:, None]
    rank = t - (t > wt[None, :]).long()                                   # index among the other tiles
    other = bm[None, :] // (c.tiles - 1) + (rank < (bm % (c.tiles - 1))[None, :]).long()
    ssp[:, :rows] = torch.where(t == wt[None, :], 3 * bm[None, :], other).float()
    return ssp


@functools.lru_cache(maxsize=8)
def inputs(name: str) -> SimpleNamespace:
    """The case's tensors, seeded: x [mx, K], w [3 wr, K] (grouped: [E, 3 wr, K]), resid [mx, N], ssp; `parts`
    are the float64 split-K partials [sk, mx, 3 wr] of all rows (a launch of M rows is their first M)."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    i = SimpleNamespace(c=c)
    k, wrows = c.k, NTILES * c.wr
    if c.kind == "grouped":
        return _grouped_inputs(c, gen, i)
    mx = c.mx
    if c.family == "random":
        i.x = torch.randn(mx, k, generator=gen).to(torch.bfloat16)
        i.w = (torch.randn(wrows, k, generator=gen) / k ** 0.5).to(torch.bfloat16)
        i.resid = torch.randn(mx, c.n, generator=gen).to(torch.bfloat16)
    else:
        i.x = _signed(gen, (mx, k), 1)
        i.w = _signed(gen, (wrows, k), c.amp)
        i.resid = _signed(gen, (mx, c.n), 4)
        if c.amax:
            # ties by construction: inside every column tile the upper half of the columns repeats the lower half
            # (the tie crosses lanes) and column 8 i + 1 repeats column 8 i (the tie stays inside a lane)
            w = i.w.view(NTILES, c.wr, k)
            w[:, 1:c.wr // 2:8] = w[:, 0:c.wr // 2:8]
            w[:, c.wr // 2:] = w[:, :c.wr // 2]
    i.ssp = make_ssp(c, mx, gen, unit=c.family == "random") if c.tiles else None
    i.parts = partials(i.x.double(), i.w.double(), c.kc, c.sk)
    i.absum = i.x.double().abs() @ i.w.double().abs().T
    return i


def _grouped_inputs(c, gen, i):
    k, wrows = c.k, NTILES * c.wr
    groups = len(c.counts)
    e = groups // c.segs
    lead = 1
    tot = lead + sum(c.counts)
    r = tot + 2 + (tot % 2)                       # rows outside every group at both ends; even for k = 2
    i.offsets = torch.tensor([lead + sum(c.counts[:g]) for g in range(groups + 1)], dtype=torch.int32)
    i.w = _signed(gen, (e, wrows, k), c.amp)
    i.k = 2 if c.gather else 1
    if c.gather:
        i.rowmap = torch.randperm(r, generator=gen).to(torch.int32)   # sorted row j is token rowmap[j] // 2
        i.x = _signed(gen, (r // 2, k), 1)
        xs = i.x[(i.rowmap // 2).long()]
    else:
        i.rowmap = None
        i.x = xs = _signed(gen, (r, k), 1)
    i.r = r
    i.y = torch.zeros(r, wrows, dtype=torch.float64)
    i.absum = torch.zeros(r, wrows, dtype=torch.float64)
    i.inside = torch.zeros(r, dtype=torch.bool)
    for g in range(groups):
        lo, hi = int(i.offsets[g]), int(i.offsets[g + 1])
        wg = i.w[g // c.segs].double()
        i.y[lo:hi] = xs[lo:hi].double() @ wg.T
        i.absum[lo:hi] = xs[lo:hi].double().abs() @ wg.abs().T
        i.inside[lo:hi] = True
    i.xs = xs
    return i


# ---------------------------------------------------------------------------------------------- oracle

def partials(x: torch.Tensor, w: torch.Tensor, kc: int, sk: int) -> torch.Tensor:
    """[sk, M, rows of w] float64: slice by of x w^T."""
    return torch.stack([x[:, lo:hi] @ w[:, lo:hi].T for lo, hi in slices(x.shape[1], kc, sk)])


def half_ulp_bf16(o: torch.Tensor) -> torch.Tensor:
    """Half the spacing of bf16 at |o| (float64), the subnormal spacing below the smallest normal."""
    _, e = torch.frexp(o.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(o), (e - 1).clamp_min(-126) - 8)


def row_scale(ssp: torch.Tensor, m: int, k: int) -> torch.Tensor:
    return (ssp[:, :m].double().sum(0) / k + EPS) ** -0.5


def silu_mul(g, u, r):
    """(o, z, tol) of silu(g r) * (u r), r [M] or 1."""
    r = r[:, None] if torch.is_tensor(r) else r
    z = g * r
    o = z / (1 + torch.exp(-z)) * (u * r)
    return o, z, half_ulp_bf16(o) + C_SILU * U23 * (1 + z.abs()) * o.abs()


def sensitivity(g, u, r) -> torch.Tensor:
    """True where every change of g or of u by +-1 moves the oracle by more than 4 tol."""
    o, _, tol = silu_mul(g, u, r)
    ok = torch.ones_like(o, dtype=torch.bool)
    for dg, du in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        ok &= (silu_mul(g + dg, u + du, r)[0] - o).abs() > 4 * tol
    return ok


def slab6_layout(parts: torch.Tensor, wr: int) -> torch.Tensor:
    """Mode 6's slab [sk, M, 2 N]: tile-local columns, gate at bx wr + j, up at bx wr + wr / 2 + j."""
    sk, m, w2 = parts.shape
    n, no = w2 // 2, wr // 2
    g = parts[:, :, :n].reshape(sk, m, n // no, no)
    u = parts[:, :, n:].reshape(sk, m, n // no, no)
    return torch.cat([g, u], 3).reshape(sk, m, w2)


def finish(c: Case, parts: torch.Tensor, m: int, resid=None, ssp=None) -> SimpleNamespace:
    """The epilogue of mode c.mode on the float64 partials [sk, >= m, 3 wr], for a launch of m rows."""
    parts = parts[:, :m]
    y = parts.sum(0)
    e = SimpleNamespace(y=y, parts=parts)
    if c.mode == 0:
        e.yb = y.to(torch.bfloat16)
        v = e.yb.double().view(m, NTILES, c.wr)
        e.amax_val = v.max(2).values
        first = (v == e.amax_val[:, :, None]).to(torch.int32).argmax(2)   # the first of the maxima
        e.amax_col = first + torch.arange(NTILES) * c.wr
    elif c.mode == 3:
        e.h64 = resid[:m].double() + y
        e.h = e.h64.to(torch.bfloat16)
        e.ss = e.h.double().pow(2).view(m, NTILES, c.wr).sum(2).T.contiguous()   # [tile, m]
    elif c.silu:
        e.g, e.u = y[:, : c.n], y[:, c.n:]
        e.r = row_scale(ssp, m, c.k) if c.mode in (4, 6) else 1.0
        e.o, e.z, e.tol = silu_mul(e.g, e.u, e.r)
        if c.mode == 6:
            e.slab6 = slab6_layout(parts, c.wr)
    return e


def expected(name: str, m: int) -> SimpleNamespace:
    i = inputs(name)
    return finish(i.c, i.parts, m, getattr(i, "resid", None), i.ssp)


def random_bounds(c: Case, i: SimpleNamespace, e: SimpleNamespace, m: int) -> SimpleNamespace:
    """The random family's tolerances for a launch of m rows (module docstring)."""
    t = SimpleNamespace()
    k = c.k
    big = (k + c.sk) * 2.0 ** -24 * i.absum[:m]                       # on y = sum of the slices
    t.parts = torch.stack([(k + c.sk) * 2.0 ** -24 * (i.x[:m, lo:hi].double().abs() @ i.w[:, lo:hi].double().abs().T)
                           for lo, hi in slices(k, c.kc, c.sk)])
    if c.mode == 0:
        t.y = big + half_ulp_bf16(e.y.abs() + big)
    elif c.mode == 3:
        t.h = big + 2.0 ** -24 * e.h64.abs() + half_ulp_bf16(e.h64.abs() + big)
    elif c.silu:
        r = e.r[:, None] if torch.is_tensor(e.r) else e.r
        eg, eu = big[:, : c.n] * r, big[:, c.n:] * r                  # on z and on u r
        s = (e.z / (1 + torch.exp(-e.z))).abs()
        prop = 1.1 * eg * (e.u * r).abs() + s * eu + 1.1 * eg * eu
        t.o = prop + C_SILU * U23 * (1 + e.z.abs() + eg) * (e.o.abs() + prop) + half_ulp_bf16(e.o.abs() + prop)
    return t


def conditions(name: str) -> dict:
    """Asserts the integer family's exactness conditions on a case; returns the figures."""
    i = inputs(name)
    c = i.c
    assert c.family == "int"
    for t in (i.x, i.w):
        v = t.double()
        assert bool((v == v.round()).all()) and bool((v != 0).all()), f"{name}: a zero or a fraction in an operand"
    fig = {"absum": float(i.absum.max())}
    assert fig["absum"] < 2 ** 24, name
    y = i.y if c.kind == "grouped" else i.parts.sum(0)
    if c.mode == 0:
        fig["y"] = float(y.abs().max())
        assert fig["y"] <= 256, f"{name}: |y| reaches {fig['y']}"
    if c.mode == 3:
        assert bool((i.resid != 0).all())
        e = finish(c, i.parts, c.mx, i.resid)
        fig["h"], fig["ss"] = float(e.h64.abs().max()), float(e.ss.max())
        assert fig["h"] <= 256 and fig["ss"] < 2 ** 24, f"{name}: |h| {fig['h']}, ss {fig['ss']}"
    if c.tiles:
        s = i.ssp[:, : c.mx].double()
        assert bool((s == s.round()).all()) and float(s.sum(0).max()) < 2 ** 24
        assert bool(torch.isnan(i.ssp[:, c.mx:]).all())
    return fig
