"""Not a test: the float64 oracles of the per-token row kernels (csrc/kernels/norm_act.hip: RMSNorm plain, fused add
and slab, the row sums of squares, the embedding gather, SiLU * up, the RMSNorm row scale; csrc/kernels/rope_cache.hip:
RoPE + paged KV write from bf16 rows and from fp32 slabs, the block movers), their tolerances, their seeded input
families and the named case lists that test_rowwise_reference_cpu.py (which judges all of this on the CPU) and
test_rowwise_kernel_gpu.py (which judges the kernels by it) share.

Every oracle value is float64 torch from the tensors exactly as the kernel receives them. Four ways of judging:

1. Bit-exact outputs (torch.equal on the bit patterns).
   * The residual after an add. The kernels do one fp32 add (the slab forms sk sequential fp32 adds, s = 0 .. sk - 1,
     onto the residual, resp. onto 0 for RoPE) and round to bf16 (round to nearest even). An add cannot be contracted
     into anything, so fp32 CPU arithmetic in that order (resid32 + x32, then .to(bfloat16)) reproduces the bits:
     added(), slab_sum().
   * V written without a row scale (a 16-byte copy), V from slabs (slab_sum from 0, rounded), the embedding gather,
     every block mover, q under rot_q = False.
   * The fp32 sums of squares on the integer family: integers |x| <= 15, sum x^2 < 2^24, so every partial sum in any
     order, with or without fused multiply-adds, is an integer that fp32 holds exactly. norm_act.hip and
     rope_cache.hip are built with the compiler's default contraction, so no judgement here assumes unfused
     arithmetic.
   * RoPE on the exact-table family: cos / sin entries in {0, +-1, +-1/2, +-2}, q / k integers of magnitude <= 4,
     row scales that are powers of two: every product, sum and scaled sum is a multiple of 1/8 below 32, exact in
     fp32 and representable in bf16 whatever the contraction. V under a power-of-two row scale likewise.

2. Rounded outputs behind rsqrtf / v_exp_f32 / v_rcp_f32 (the y of the three norm kernels, SiLU * up, RoPE with the
   real table). o is the float64 oracle, S the float64 sum of the magnitudes of its terms, delta = c 2^-23 S. The
   kernel has to lie in [RNE_bf16(o - delta), RNE_bf16(o + delta)] (bracket(); rounding is monotone, so these are
   exactly the bf16 values that a result within delta of o can round to); where the two ends agree the element is
   decided and the kernel equals RNE_bf16(o); elsewhere the ends are the two neighbours of o, except where a
   difference cancels (RoPE: S >> |o|) and delta spans more than one bf16 step. rne_bf16() rounds the
   float64 value in one step (torch's double -> float -> bfloat16 would round twice). At most 1 % of a case's
   elements may be undecided (UNDECIDED_CAP; the CPU file asserts it per case by name). Values are compared as
   numbers, so -0 equals +0. The reported err / tol is |y - o| / (half a bf16 ulp at o + delta).

   c per op, in units of 2^-23 (one fp32 ulp, relative; a correctly rounded operation costs 0.5). Neither the ROCm
   headers (__clang_hip_math.h: rsqrtf = __ocml_rsqrt_f32, __expf(x) = v_exp_f32(log2e * x)) nor any document
   installed with them states the accuracy of v_rsq_f32, v_exp_f32 and v_rcp_f32; 1 ulp each is ASSUMED (C_HW), the
   value the decode GEMM's derivation already uses.
   * Norms, c = 2 NC + 5 with NC = ceil(hidden / 2048) chunks per thread (c_norm()). The sum of squares: a thread
     adds its 8 NC squares one at a time (8 NC roundings; without fusing the rounded squares cost one more in all),
     the wave butterfly 6, the four wave sums 3: 8 NC + 10 roundings of positive partial sums, each at most 2^-24 of
     the total = 4 NC + 5 units. / hidden: 0.5 (correctly rounded division, the compiler's default), + eps: 0.5.
     The inverse square root halves that: 2 NC + 3. rsqrtf: 1. x * inv and * w: 0.5 each. S = |o|.
   * RoPE, c = 2 (C_ROPE), S = |a cos| + |b sin| (times the row scale): unfused, the two products cost 0.5 S
     together and the difference 0.5 |o| <= 0.5 S; fused, less. The row scale: 0.5 more. 1.5, rounded up. The slab
     form's a and b are slab_sum(), reproduced bit for bit, so they enter as exact fp32 inputs.
   * SiLU, c = 10 (C_SILU, the decode GEMM's), S = (1 + |z|) |o|, z = g r: the product g r 0.5, carried through
     z sigma(z) by (1 + |z|): 0.5 (1 + |z|); the scaled exp argument 0.75 |z|, v_exp_f32 1, damped by E / (1 + E)
     <= 1; the add 0.5; the bare reciprocal 1 (a true division, as in the decode GEMM: 2.5); the multiply by it
     0.5; u r 0.5; the last multiply 0.5: <= 6.25 (1 + |z|) either way. From z = -87.34 down (e^-z >= 2^126) the
     kernel takes the denominator as exp2(t - 64) (1 + e == e there) and multiplies by 2^-64 at the end: the same
     count without the add, the subtraction and the power of two exact.

3. fp32 statistics on the non-integer families: |got - o| <= D 2^-24 o with D = 8 ceil(hidden / 2048) + 10 roundings
   as above (sumsq_tol()). rs of rms_row_scale: relative D 2^-25 + (0.5 + 0.5) 2^-24 / 2 + C_HW 2^-23 (rs_tol()).
   On the integer family ss is exact, so rs must be within C_HW 2^-23 rs of the float64 value of
   rsqrt(fl32(fl32(ss / h) + eps)) (rs_exact()).

4. Poison and sentinels are the GPU file's part: every input a view of a NaN-filled buffer, every output a view of a
   sentinel-filled one that must be bit-identical outside the specified region.

Families (norms, statistics). w is bf16 randn everywhere (so that y takes many values). The plain forms (rms_norm,
row_sumsq, rms_row_scale without x) read resid, the adding forms resid and x.
* int: x = +-1, resid = +-{3, 4}, row r times (1, 2, 3)[r mod 3]: no element and no sum is 0 (a chunk of zeros could
  leave the statistics unseen), neighbouring rows differ, |resid + x| <= 15 and sum of squares <= 225 * 16384 < 2^24.
* random: resid and the target resid + x are randn with every magnitude raised by 0.4 (no chunk so weak that losing
  it moves fewer than 8 roundings at hidden 16384), row r scaled by ROW_AMP so that neighbouring rows have different
  statistics. small: the same times 0.01: row variance about 1e-4, eps = 1e-5 is 10 % of it.
* biased: resid = +-M 2^k with an even 8-bit mantissa M in 128 .. 254, x = +-2^(k-1) with the same sign, half an ulp
  of resid (257 = 256 + 1 among them): resid + x is a tie that rounds to even, back to resid, always towards 0, so
  the statistics of the unrounded sum are 0.4 - 0.8 % larger. (Powers of two alone would make y a pure function of
  w's 8-bit mantissa and blind to small changes of the scale.)
Slabs of the int and biased families are x times integer weights that add up to 1 (SLAB_WEIGHTS, every partial sum
exact); of the others fp32 randn parts and a last slab that closes the sum on resid + x in fp32.

Sensitivity (the CPU file, per case by name). changed() counts the decided elements whose expectation a mutation
moves so far that neither of the mutated bracket's values equals it. Leaving a 16-byte chunk out of the statistics
only changes the row's scale, by a factor that grows with the chunk's sum of squares, and the set of elements that
a larger factor moves across a rounding boundary contains the set of a smaller one: so the chunk with the smallest
sum of squares is the hardest and the only one checked (weakest_chunk()). Mutations that apply to a family only:
eps = 0 to `small`, the unrounded statistics to `biased`, a neighbour's scale to cases of more than one row, the
single row-scale application of SiLU to cases with a row scale.

SiLU ladder. Gates: every integer in [-110, 110] with ups {1, -2^20, 2^40, 2^-20}; every bf16 value in [-92, -87],
+-0 and +-the two largest finite bf16 with ups {+-1, +-2^20, +-2^40, 2^-20}; a pair is kept if the oracle is 0 or a
bf16 normal in [2^-120, 2^120] (so the band below -87 is populated by up = +-1 and 2^20, the far end by 2^40). The
pairs fill the head of row LADDER_ROW of a case's [3, inter] block, the rest is the random family (gates randn * 4):
the bound's (1 + |z|) makes 2 - 5 % of the elements at |z| ~ 100 undecided, and the cap of 1 % holds for the case.
For the largest gates (1 + |z|) |o| exceeds every bf16 value, so the bracket only asks for a finite result there.
Through the row scale: every bf16 gate in [-37, -29] in every row, with r = 3, 2.875, 3.125 (z from -116 to -83).

Measured on one MI355X (worst err / tol over the case lists; undecided share: the largest of any case, from the
oracle alone): see docs/performance.md, "Row kernels oracle".
"""

from __future__ import annotations

import functools
from dataclasses import dataclass
from types import SimpleNamespace

import torch

U23 = 2.0 ** -23
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))   # the kernels take eps as a float
C_HW = 1.0              # assumed accuracy of v_rsq_f32 / v_exp_f32 / v_rcp_f32 in ulp
C_ROPE = 2.0
C_V = 1.0               # V under a row scale that is no power of two: one multiply (0.5), rounded up; S = |v r|
C_SILU = 10.0
UNDECIDED_CAP = 0.01
MIN_CHANGED = 8
SSP_LD = 128
SENT = 12352.0          # sentinel of bf16 / fp32 output buffers (no case produces it)
INT_ROW_MUL = (1, 2, 3)
ROW_AMP = (1.0, 1.5, 0.75, 1.25, 0.5, 2.0, 1.75, 0.625)
BF16_MAX = float(torch.finfo(torch.bfloat16).max)


# ---------------------------------------------------------------------------------------------- rounding, judging

def half_ulp_bf16(o: torch.Tensor) -> torch.Tensor:
    """Half the spacing of bf16 at |o| (float64), the subnormal spacing below the smallest normal."""
    _, e = torch.frexp(o.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(o), (e - 1).clamp_min(-126) - 8)


def rne_bf16(o: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (ties to even) in one rounding, as float64."""
    sp = 2 * half_ulp_bf16(o)
    return torch.round(o / sp) * sp


def bracket(o, s, c):
    """(lo, hi): the bf16 values the kernel may return for oracle o, magnitude sum s and constant c."""
    d = c * U23 * s
    return rne_bf16(o - d), rne_bf16(o + d)


def judge(y: torch.Tensor, o, s, c) -> SimpleNamespace:
    """y (any float dtype) against the bracket: ok [elementwise], undecided share, worst err / tol."""
    y = y.double()
    lo, hi = bracket(o, s, c)
    ok = (y >= lo) & (y <= hi)
    tol = half_ulp_bf16(o) + c * U23 * s
    return SimpleNamespace(ok=ok, undecided=float((lo != hi).double().mean()), ratio=float(((y - o).abs() / tol).max()),
                           lo=lo, hi=hi)


def changed(o, s, o_mut, s_mut, c) -> torch.Tensor:
    """Per element: the expectation is decided and the mutated oracle's bracket does not contain it."""
    lo, hi = bracket(o, s, c)
    lom, him = bracket(o_mut, s_mut, c)
    return (lo == hi) & ((lo < lom) | (lo > him))


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------- norms, statistics

def nc_of(hidden: int) -> int:
    """16-byte chunks per thread of the 256-thread row kernels."""
    return (hidden // 8 + 255) // 256


def c_norm(hidden: int) -> float:
    return 2.0 * nc_of(hidden) + 5.0


def sum_depth(hidden: int) -> int:
    return 8 * nc_of(hidden) + 10


def sumsq_tol(ss: torch.Tensor, hidden: int) -> torch.Tensor:
    return sum_depth(hidden) * 2.0 ** -24 * ss


def rs_tol(rs: torch.Tensor, hidden: int) -> torch.Tensor:
    return rs * (sum_depth(hidden) * 2.0 ** -25 + 2.0 ** -24 + C_HW * U23)


def added(resid: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """bf16(resid + x): one fp32 add, one rounding."""
    return (resid.float() + x.float()).to(torch.bfloat16)


def slab_sum(slab: torch.Tensor, start=None) -> torch.Tensor:
    """fp32: start (bf16 / fp32 / None = 0) + slab[0] + slab[1] + ... in that order."""
    acc = torch.zeros_like(slab[0]) if start is None else start.float().clone()
    for s in range(slab.shape[0]):
        acc = acc + slab[s]
    return acc


def sumsq(h: torch.Tensor) -> torch.Tensor:
    return h.double().pow(2).sum(-1)


def norm_y(h: torch.Tensor, w: torch.Tensor, ss: torch.Tensor, hmean: float, eps: float = EPS32):
    """(o, S) of h * rsqrt(ss / hmean + eps) * w; ss [rows] float64."""
    var = ss / hmean if hmean else torch.full_like(ss, float("inf"))
    o = h.double() * ((var + eps) ** -0.5)[:, None] * w.double()[None, :]
    return o, o.abs()


def rs_exact(ss: torch.Tensor, hidden: int) -> torch.Tensor:
    """float64 rsqrt of the fp32 argument the kernel forms from an exact fp32 ss."""
    var = ss.float() / torch.tensor(float(hidden), dtype=torch.float32)
    return (var + torch.tensor(EPS, dtype=torch.float32)).double() ** -0.5


def weakest_chunk(h: torch.Tensor) -> torch.Tensor:
    """[rows]: the sum of squares of each row's 16-byte chunk with the smallest one."""
    return h.double().pow(2).view(h.shape[0], -1, 8).sum(-1).min(-1).values


@dataclass(frozen=True)
class RowCase:
    name: str
    op: str            # norm | rs | sumsq
    hidden: int
    rows: int
    family: str
    sk: int = 1
    strided: bool = False
    seed: int = 0

    @property
    def exact_stats(self) -> bool:
        return self.family == "int"


def _nc_sizes(top: int):
    out = [8]
    for nc in range(1, top + 1):
        for h in (2048 * (nc - 1) + 8, 2048 * (nc - 1) + 16, 2048 * nc):
            if h not in out:
                out.append(h)
    return out


NORM_HIDDENS = _nc_sizes(8)
RS_HIDDENS = _nc_sizes(4)
SUMSQ_HIDDENS = (8, 2040, 2048, 2056, 8192)
SUMSQ_ROWS = (1, 7, 128)
NORM_REFUSED_HIDDEN = 16392
RS_REFUSED_HIDDEN = 8200
SUMSQ_REFUSED_ROWS = 129
FAMILIES = ("int", "random", "small", "biased")
EMBED_VOCAB = 11


def _row_cases():
    out = []
    i = 0
    for h in NORM_HIDDENS:
        for fam in FAMILIES:
            if fam == "biased" and h < 2048:
                continue   # 8 or 16 elements cannot show a 0.4 % scale change on 8 decided elements
            sk = (2, 5)[i % 2] if fam == "biased" else (1, 2, 5)[i % 3]   # biased, one slab: dropping it is no change
            out.append(RowCase(f"norm-h{h}-{fam}", "norm", h, (1, 3)[i % 2], fam, sk, (i // 2) % 2 == 1, 2000 + i))
            i += 1
    for h in RS_HIDDENS:
        for fam in FAMILIES:
            out.append(RowCase(f"rs-h{h}-{fam}", "rs", h, (3, 1)[i % 2], fam, 1, (i // 2) % 2 == 1, 2000 + i))
            i += 1
    for h in SUMSQ_HIDDENS:
        for r in SUMSQ_ROWS:
            for fam in ("int", "random", "biased"):
                out.append(RowCase(f"sumsq-h{h}-r{r}-{fam}", "sumsq", h, r, fam, 1, i % 2 == 1, 2000 + i))
                i += 1
    return out


ROW_ALL = _row_cases()
ROW_CASES = {c.name: c for c in ROW_ALL}
NORM_CASES = [c.name for c in ROW_ALL if c.op == "norm"]
RS_CASES = [c.name for c in ROW_ALL if c.op == "rs"]
SUMSQ_CASES = [c.name for c in ROW_ALL if c.op == "sumsq"]
# every weight has magnitude >= 3: without or with twice any slab the biased family's sum is resid + t x with
# |t| >= 2 (x is half an ulp of resid, and only t in {-1, 0, 1} rounds back to the residual)
SLAB_WEIGHTS = {1: (1,), 2: (4, -3), 5: (3, -4, 5, -6, 3)}


def _signed(gen, shape, a):
    mag = torch.randint(1, a + 1, shape, generator=gen)
    return (mag * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).to(torch.bfloat16)


def _floored(gen, shape):
    """randn with every magnitude raised by 0.4: no 16-byte chunk is so weak that the statistics could lose it unseen."""
    z = torch.randn(shape, generator=gen)
    return torch.sign(z) * (z.abs() + 0.4)


def _family_pair(fam: str, gen, rows: int, hidden: int):
    """(x, resid) bf16 [rows, hidden] of a family; the random families draw resid and the target resid + x floored."""
    shape = (rows, hidden)
    if fam == "int":
        mul = torch.tensor([INT_ROW_MUL[r % 3] for r in range(rows)])[:, None]
        x = _signed(gen, shape, 1)
        mag = torch.randint(3, 5, shape, generator=gen) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
        return (x.long() * mul).to(torch.bfloat16), (mag * mul).to(torch.bfloat16)
    if fam == "biased":
        half = 2 ** (torch.randint(0, 3, shape, generator=gen) + (torch.arange(rows) % 3)[:, None])   # half an ulp
        mant = 2 * torch.randint(64, 128, shape, generator=gen)                                      # even, 8 bits
        sg = torch.randint(0, 2, shape, generator=gen) * 2 - 1
        return (sg * half).to(torch.bfloat16), (sg * mant * 2 * half).to(torch.bfloat16)
    amp = row_amp(fam, rows)
    resid = (_floored(gen, shape) * amp).to(torch.bfloat16)
    target = _floored(gen, shape) * amp * 2 ** 0.5
    return (target - resid.float()).to(torch.bfloat16), resid


def row_amp(fam: str, rows: int) -> torch.Tensor:
    return torch.tensor([ROW_AMP[r % len(ROW_AMP)] for r in range(rows)])[:, None] * (0.01 if fam == "small" else 1.0)


@functools.lru_cache(maxsize=4)
def row_inputs(name: str) -> SimpleNamespace:
    """The case's tensors: x, resid [rows, hidden] bf16, w [hidden] bf16; norm: slab [sk, rows, hidden] fp32; sumsq:
    table [EMBED_VOCAB, hidden] bf16 and ids [rows] int64 (repeats, the first and the last table row)."""
    c = ROW_CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    i = SimpleNamespace(c=c)
    i.x, i.resid = _family_pair(c.family, gen, c.rows, c.hidden)
    i.w = torch.randn(c.hidden, generator=gen).to(torch.bfloat16)
    if c.op == "norm":
        if c.family in ("int", "biased"):
            i.slab = torch.stack([i.x.float() * k for k in SLAB_WEIGHTS[c.sk]])
        else:   # random parts, the last one closes the sum on resid + x (in fp32: slab_sum() is the truth)
            parts = [torch.randn(c.rows, c.hidden, generator=gen) * row_amp(c.family, c.rows) for _ in range(c.sk - 1)]
            i.slab = torch.stack(parts + [i.x.float() - sum(parts)]) if parts else i.x.float()[None].clone()
    if c.op == "sumsq":
        i.table = _family_pair(c.family, gen, EMBED_VOCAB, c.hidden)[1]
        ids = torch.randint(0, EMBED_VOCAB, (c.rows,), generator=gen)
        ids[0] = EMBED_VOCAB - 1 if c.seed % 2 else 0
        if c.rows > 2:
            ids[1], ids[2], ids[-1] = 0, EMBED_VOCAB - 1, ids[0]
        i.ids = ids
    return i


def norm_expected(name: str, form: str, **mut) -> SimpleNamespace:
    """form: plain (rms_norm of resid) | add (fused_add_rms_norm) | slab (fused_add_rms_norm_slab) | rs_add | rs_plain
    (rms_row_scale with and without x). -> h (the bf16 residual after the op, the input for plain), o, S, c, and
    ss, rs, rs_tol for the rs forms. Mutations: drop_weakest, hdelta, eps, unrounded, shift_rows, slabs (indices)."""
    i = row_inputs(name)
    c = i.c
    e = SimpleNamespace()
    if form == "plain":
        e.h, exact = i.resid, i.resid.double()
    elif form in ("add", "rs_add"):
        e.h, exact = added(i.resid, i.x), i.resid.double() + i.x.double()
    elif form == "rs_plain":
        e.h, exact = i.resid, i.resid.double()
    else:
        slab = i.slab[list(mut["slabs"])] if "slabs" in mut else i.slab
        e.h = slab_sum(slab, i.resid).to(torch.bfloat16)
        exact = i.resid.double() + slab.double().sum(0)
    ss = exact.pow(2).sum(-1) if mut.get("unrounded") else sumsq(e.h)
    if mut.get("drop_weakest"):
        ss = ss - weakest_chunk(e.h)
    if mut.get("shift_rows"):
        ss = ss.roll(1)
    e.ss = ss
    hmean = c.hidden + mut.get("hdelta", 0)
    eps = mut.get("eps", EPS32)
    e.o, e.s = norm_y(e.h, i.w, ss, hmean, eps)
    e.c = c_norm(c.hidden)
    var = ss / hmean if hmean else torch.full_like(ss, float("inf"))
    e.rs = (var + eps) ** -0.5
    e.rs_tol = rs_tol(e.rs, c.hidden)
    if c.exact_stats and not mut:
        e.rs = rs_exact(ss, c.hidden)
        e.rs_tol = C_HW * U23 * e.rs
    return e


def sumsq_expected(name: str, op: str, unrounded: bool = False) -> SimpleNamespace:
    """op: row (row_sumsq of resid) | embed (table[ids]) | add (residual_add_sumsq). -> h (bf16 rows written or read),
    ss [rows] float64, tol [rows] (0 on the integer family)."""
    i = row_inputs(name)
    c = i.c
    e = SimpleNamespace()
    e.h = {"row": lambda: i.resid, "embed": lambda: i.table[i.ids], "add": lambda: added(i.resid, i.x)}[op]()
    e.ss = (i.resid.double() + i.x.double()).pow(2).sum(-1) if unrounded else sumsq(e.h)
    e.tol = torch.zeros_like(e.ss) if c.exact_stats else sumsq_tol(e.ss, c.hidden)
    return e


# ---------------------------------------------------------------------------------------------- SiLU * up

def silu_mul(g, u, r=1.0):
    """(o, S, z) of silu(g r) * (u r); r [rows] or a number."""
    r = r[:, None].double() if torch.is_tensor(r) else r
    z = g.double() * r
    o = z / (1 + torch.exp(-z)) * (u.double() * r)
    return o, (1 + z.abs()) * o.abs(), z


SILU_INTERS = (8, 2040, 2048, 2056, 3072)   # 2056 and 3072: gridDim.y = 2 at one chunk per lane
SILU_PERS = tuple(range(9))
SILU_ROWS = 3
LADDER_UPS = (1.0, -1.0, 2.0 ** 20, -2.0 ** 20, 2.0 ** 40, -2.0 ** 40, 2.0 ** -20)
LADDER_UPS_WIDE = (1.0, -2.0 ** 20, 2.0 ** 40, 2.0 ** -20)
LADDER_RS = (3.0, 2.875, 3.125)
LADDER_ROW = 1          # the row of a 'ladder' case that holds the ladder


def _bf16_values(lo: float, hi: float) -> torch.Tensor:
    """Every bf16 value in [lo, hi] (same sign, nonzero), ascending."""
    a = torch.tensor([lo, hi]).to(torch.bfloat16).view(torch.int16).tolist()
    v = torch.arange(min(a), max(a) + 1, dtype=torch.int16).view(torch.bfloat16)
    return v.double().sort().values


def _ladder_pairs(gates: torch.Tensor, ups, rs):
    g = gates.repeat_interleave(len(ups))
    u = torch.tensor(ups, dtype=torch.float64).repeat(gates.numel())
    keep = torch.ones_like(g, dtype=torch.bool)
    for r in rs:
        o = silu_mul(g, u, r)[0].abs()
        keep &= (o == 0) | ((o >= 2.0 ** -120) & (o <= 2.0 ** 120))
    return g[keep].to(torch.bfloat16), u[keep].to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def ladder(kind: str):
    """(gate, up) bf16 [n] of the gate ladder ('ladder': r = 1) or of the one reached through LADDER_RS
    ('ladder_rs')."""
    if kind == "ladder":
        top = torch.tensor([BF16_MAX]).to(torch.bfloat16)
        big = torch.cat([top, (top.view(torch.int16) - 1).view(torch.bfloat16)]).double()
        wide = _ladder_pairs(torch.arange(-110, 111, dtype=torch.float64), LADDER_UPS_WIDE, (1.0,))
        band = _ladder_pairs(torch.cat([_bf16_values(-92.0, -87.0), torch.tensor([0.0, -0.0], dtype=torch.float64),
                                        big, -big]), LADDER_UPS, (1.0,))
        return torch.cat([wide[0], band[0]]), torch.cat([wide[1], band[1]])
    return _ladder_pairs(_bf16_values(-37.0, -29.0), LADDER_UPS, LADDER_RS)


@dataclass(frozen=True)
class SiluCase:
    name: str
    inter: int
    per: int
    family: str        # random | ladder | ladder_rs
    scaled: bool       # a row scale is passed
    seed: int = 0


def _silu_cases():
    out = []
    i = 0
    for inter in SILU_INTERS:
        for per in SILU_PERS:
            for fam in ("random", "ladder", "ladder_rs"):
                if fam != "random" and inter < 2040:
                    continue
                scaled = fam == "ladder_rs" or (fam == "random" and i % 2 == 0)
                out.append(SiluCase(f"silu-i{inter}-p{per}-{fam}", inter, per, fam, scaled, 4000 + i))
                i += 1
    return out


SILU_ALL = _silu_cases()
SILU_CASES = {c.name: c for c in SILU_ALL}


@functools.lru_cache(maxsize=4)
def silu_inputs(name: str) -> SimpleNamespace:
    """gate, up [SILU_ROWS, inter] bf16 and r [SILU_ROWS] fp32 or None; n_ladder: the leading elements (row-major)
    that hold the ladder."""
    c = SILU_CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    shape = (SILU_ROWS, c.inter)
    g = (torch.randn(shape, generator=gen) * 4).to(torch.bfloat16)
    u = torch.randn(shape, generator=gen).to(torch.bfloat16)
    i = SimpleNamespace(c=c, n_ladder=0, r=None)
    if c.family == "random":
        if c.scaled:
            i.r = (0.5 + 1.5 * torch.rand(SILU_ROWS, generator=gen)).float()
    else:
        lg, lu = ladder(c.family)
        n = lg.numel()
        assert n <= c.inter, "the ladder has to fit into one row"
        i.n_ladder = n
        if c.scaled:      # the ladder in every row: each row reaches it at its own r
            g[:, :n], u[:, :n] = lg, lu
            i.r = torch.tensor(LADDER_RS, dtype=torch.float32)
        else:
            g[LADDER_ROW, :n], u[LADDER_ROW, :n] = lg, lu
    i.gate, i.up = g, u
    return i


def silu_expected(name: str, swap: bool = False, once: bool = False) -> SimpleNamespace:
    i = silu_inputs(name)
    r = i.r if i.r is not None else 1.0
    g, u = (i.up, i.gate) if swap else (i.gate, i.up)
    e = SimpleNamespace(c=C_SILU)
    e.o, e.s, e.z = silu_mul(g, u, r)
    if once:
        e.o = e.o / i.r[:, None].double()
        e.s = e.s / i.r[:, None].double()
    return e


# ---------------------------------------------------------------------------------------------- RoPE + KV write

ROPE_HEADS = ((1, 1), (8, 1), (4, 4), (8, 8), (32, 8))   # (8, 8) at head_dim 128: exactly one pass of 256 items
ROPE_TOKENS = 6
ROPE_BLOCKS = 5
MAX_POS = 64
ROPE_THETA = 10000.0
EXACT_PAIRS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.5, 2.0), (2.0, -0.5), (0.0, -1.0), (-0.5, 0.5), (1.0, 1.0),
               (-2.0, 1.0), (0.5, -1.0), (-1.0, -2.0))


def rope_items(d: int, hq: int, hkv: int, rot_q: bool) -> int:
    """Work items of one token's workgroup (256 threads per pass)."""
    return ((hq if rot_q else 0) + hkv) * (d // 16) + hkv * (d // 8)


@dataclass(frozen=True)
class RopeCase:
    name: str
    d: int
    hq: int
    hkv: int
    block_size: int
    family: str        # exact | real
    rot_q: bool = True
    scaled: bool = False
    wide: bool = False
    sk: int = 0        # > 0: the slab form
    seed: int = 0

    @property
    def width(self) -> int:
        return (self.hq + 2 * self.hkv) * self.d


def _rope_cases():
    out = []
    i = 0
    for d in (64, 128):
        for hq, hkv in ROPE_HEADS:
            for bs in (16, 32):
                for fam in ("exact", "real"):
                    t = f"d{d}-h{hq}x{hkv}-b{bs}-{fam}"
                    out.append(RopeCase(f"rope-{t}-q", d, hq, hkv, bs, fam, True, False, i % 2 == 0, 0, 6000 + i))
                    out.append(RopeCase(f"rope-{t}-k", d, hq, hkv, bs, fam, False, i % 2 == 1, i % 4 < 2, 0,
                                        6100 + i))
                    out.append(RopeCase(f"ropeslab-{t}", d, hq, hkv, bs, fam, True, False, False, (1, 2, 5)[i % 3],
                                        6200 + i))
                    i += 1
    return out


ROPE_ALL = _rope_cases()
ROPE_CASES_BY_NAME = {c.name: c for c in ROPE_ALL}
ROPE_CASES = [c.name for c in ROPE_ALL if not c.sk]
ROPE_SLAB_CASES = [c.name for c in ROPE_ALL if c.sk]


def exact_table(d: int) -> torch.Tensor:
    """[MAX_POS, d] fp32, cos | sin from EXACT_PAIRS: row p, dim j takes pair (3 p + j) mod 11, so rows p and p +- 1
    (and p +- 2, 3) differ in every dim."""
    p = torch.arange(MAX_POS)[:, None]
    j = torch.arange(d // 2)[None, :]
    pairs = torch.tensor(EXACT_PAIRS, dtype=torch.float32)[(3 * p + j) % len(EXACT_PAIRS)]
    return torch.cat([pairs[..., 0], pairs[..., 1]], 1).contiguous()


def real_table(d: int) -> torch.Tensor:
    half = d // 2
    inv = 1.0 / (ROPE_THETA ** (torch.arange(0, half, dtype=torch.float64) / half))
    f = torch.outer(torch.arange(MAX_POS, dtype=torch.float64), inv)
    return torch.cat([f.cos(), f.sin()], -1).float()


@functools.lru_cache(maxsize=4)
def rope_inputs(name: str) -> SimpleNamespace:
    """qkv [T, width] bf16 (or slab [sk, T, width] fp32), positions, slots [T] int64, table [MAX_POS, d] fp32,
    r [T] fp32 or None. Slots: the first and the last of block 0, the first and the last of the last block, -1, one
    inside a middle block; positions 0, MAX_POS - 1 and four distinct others."""
    c = ROPE_CASES_BY_NAME[name]
    gen = torch.Generator().manual_seed(c.seed)
    i = SimpleNamespace(c=c, r=None)
    t, bs = ROPE_TOKENS, c.block_size
    i.slots = torch.tensor([0, bs - 1, (ROPE_BLOCKS - 1) * bs, ROPE_BLOCKS * bs - 1, -1, 2 * bs + 3])
    i.positions = torch.tensor([0, MAX_POS - 1, 7, 8, 31, 40])
    i.table = exact_table(c.d) if c.family == "exact" else real_table(c.d)
    if c.sk:
        if c.family == "exact":
            # integer slabs whose sequential sums are exact and end in +-{1..4}
            tot = _signed(gen, (t, c.width), 4).float()
            parts = [torch.randint(-8, 9, (t, c.width), generator=gen).float() for _ in range(c.sk - 1)]
            i.slab = torch.stack(parts + [tot - sum(parts)]) if parts else tot[None]
        else:
            i.slab = torch.randn(c.sk, t, c.width, generator=gen) / c.sk ** 0.5
        i.rows = slab_sum(i.slab)                       # fp32 [T, width]: what the rotation receives
    else:
        i.qkv = _signed(gen, (t, c.width), 4) if c.family == "exact" else \
            torch.randn(t, c.width, generator=gen).to(torch.bfloat16)
        i.rows = i.qkv.float()
        if c.scaled:
            i.r = (2.0 ** torch.randint(-2, 2, (t,), generator=gen).float()) if c.family == "exact" else \
                (0.5 + torch.rand(t, generator=gen)).float()
    return i


def rotate(x: torch.Tensor, cs: torch.Tensor, scale=None, swap_halves=False, flip_sin=False):
    """x [T, H, D] float64, cs [T, D] float64 -> (o, S) [T, H, D]."""
    half = x.shape[-1] // 2
    cos, sin = cs[:, None, :half], cs[:, None, half:]
    if flip_sin:
        sin = -sin
    a, b = x[..., :half], x[..., half:]
    if swap_halves:
        a, b = b, a
    o = torch.cat([a * cos - b * sin, b * cos + a * sin], -1)
    s = torch.cat([(a * cos).abs() + (b * sin).abs(), (b * cos).abs() + (a * sin).abs()], -1)
    if scale is not None:
        o, s = o * scale[:, None, None], s * scale[:, None, None]
    return o, s


def rope_expected(name: str, **mut) -> SimpleNamespace:
    """q (o, S) [T, hq, D] and whether q is rotated; the K cache (o, S) and the V cache (float64) with a `written`
    mask, all [blocks, hkv, block_size, D]. v_exact: V is a copy or an exactly rounded sum (bit-exact judgement),
    else it is a scaled value under the bracket with c = 0.5 (one multiply). Mutations: swap_halves, flip_sin,
    pos_shift, slot_shift (tokens), head_shift (kv heads), scale_q, unscaled_v, slabs (indices)."""
    i = rope_inputs(name)
    c = i.c
    t, d = ROPE_TOKENS, c.d
    rows = i.rows
    if "slabs" in mut:
        rows = slab_sum(i.slab[list(mut["slabs"])]) if mut["slabs"] else torch.zeros_like(i.rows)
    rows = rows.double()
    q = rows[:, : c.hq * d].view(t, c.hq, d)
    k = rows[:, c.hq * d:(c.hq + c.hkv) * d].view(t, c.hkv, d)
    v = rows[:, (c.hq + c.hkv) * d:c.width].view(t, c.hkv, d)
    pos = (i.positions + mut.get("pos_shift", 0)).clamp(0, MAX_POS - 1)
    cs = i.table.double()[pos]
    r = i.r.double() if i.r is not None else None
    kw = dict(swap_halves=mut.get("swap_halves", False), flip_sin=mut.get("flip_sin", False))
    e = SimpleNamespace(rot_q=c.rot_q, c=C_ROPE)
    e.q, e.qs = rotate(q, cs, None, **kw) if c.rot_q else (q, q.abs())
    if mut.get("scale_q"):      # the row scale wrongly applied to q as well (rot_q = False: to the unrotated q)
        e.q, e.qs = e.q * r[:, None, None], e.qs * r[:, None, None]
    ko, ks = rotate(k, cs, r, **kw)
    vo = v * r[:, None, None] if r is not None and not mut.get("unscaled_v") else v
    e.v_exact = r is None or c.family == "exact"
    shape = (ROPE_BLOCKS, c.hkv, c.block_size, d)
    e.k, e.ks, e.v = (torch.zeros(shape, dtype=torch.float64) for _ in range(3))
    e.written = torch.zeros(shape, dtype=torch.bool)
    slots = i.slots.roll(mut.get("slot_shift", 0))
    hs = mut.get("head_shift", 0)
    for tok in range(t):
        s = int(slots[tok])
        if s < 0:
            continue
        b, off = s // c.block_size, s % c.block_size
        e.k[b, :, off], e.ks[b, :, off], e.v[b, :, off] = ko[tok].roll(hs, 0), ks[tok].roll(hs, 0), vo[tok].roll(hs, 0)
        e.written[b, :, off] = True
    return e


# ---------------------------------------------------------------------------------------------- block movers

@dataclass(frozen=True)
class MoverCase:
    name: str
    planes: int
    blocks: int
    slab: int          # elements of one (plane, block)


MOVER_ALL = [MoverCase(f"move-p{p}-s{s}", p, 7, s) for p in (1, 6) for s in (8, 8 * 300)]
MOVER_CASES = {c.name: c for c in MOVER_ALL}
COPY_PAIRS = ((0, 3), (6, 1), (4, 5))        # disjoint (src, dst); the first and the last block among them
MOVE_IDS = ((6, 0, 3), (3, 5, 1, 0, 6, 2, 4))   # a permuted subset with both ends, a full permutation


def mover_pool(name: str) -> torch.Tensor:
    """[planes, blocks, slab] bf16 whose 16-bit patterns count up (all finite, every chunk different)."""
    c = MOVER_CASES[name]
    n = c.planes * c.blocks * c.slab
    return (torch.arange(n, dtype=torch.int32) % 32000 + 128).to(torch.int16).view(torch.bfloat16).view(
        c.planes, c.blocks, c.slab)


def copied(pool: torch.Tensor, pairs) -> torch.Tensor:
    out = pool.clone()
    for s, d in pairs:
        out[:, d] = pool[:, s]
    return out


def gathered(pool: torch.Tensor, ids) -> torch.Tensor:
    """[n, planes, slab]."""
    return pool[:, list(ids)].transpose(0, 1).contiguous()


def scattered(pool: torch.Tensor, ids, buf: torch.Tensor) -> torch.Tensor:
    out = pool.clone()
    out[:, list(ids)] = buf.transpose(0, 1)
    return out


