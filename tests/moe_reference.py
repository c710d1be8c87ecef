"""Not a test: the float64 oracles of the mixture-of-experts kernels (csrc/kernels/moe.hip: topk_softmax,
moe_route<8|16>, moe_align, moe_gather, moe_combine, moe_combine_residual), their tolerances, their seeded input
families and the named case lists that test_moe_reference_cpu.py (which judges all of this on the CPU) and
test_moe_kernel_gpu.py (which judges the kernels by it) share.

Every oracle value is float64 torch from the tensors exactly as the kernel receives them.

Selection rule (both routing kernels, ref.topk_softmax, topk() here): slot k holds the k-th largest logit, and among
equal logits the lowest expert index comes first. -inf entries are equal to one another and are taken lowest index
first once the finite ones are used up. A row with a NaN has no order that a comparison could state: there the ids
only have to be K distinct values in [0, E), and the weights (NaN in the oracle) are not judged.

Ids are always compared with torch.equal, slot order included, on every row without a NaN. Nothing is excluded.

Routing weights (fp32), tolerance. Units of 2^-23 (one fp32 ulp, relative; a correctly rounded operation costs
0.5); the per-operation bounds are those of gemm_decode_reference's SiLU section and rowwise_reference's C_HW.
With d_e = g_e - max (<= 0), p_e the softmax and z = sum_e exp(d_e):
  * the subtraction g_e - max: 0.5 ulp of d, so 0.5 |d| in exp(d);
  * __expf(d) = exp2(d log2 e): the rounded product and the rounded constant, 0.75 |d|; v_exp_f32: 1 (C_HW);
    together a(d) = 1.25 |d| + 1 for one exponential;
  * z: every term carries a(d_e), weighted by its share p_e: sum_e p_e a(d_e) = 1.25 D + 1 with D = sum_e p_e |d_e|;
    E - 1 adds of positive partial sums, 0.5 each;
  * exp(d_k) / z: 2.5 (the documented bound of the fast fp32 divide; 0.5 where it is correctly rounded).
  renorm off:  c_k = a(d_k) + 1.25 D + 1 + 0.5 (E - 1) + 2.5 = 1.25 (|d_k| + D) + 0.5 (E - 1) + 4.5.
  renorm on:   w_k = p_k / sum_j p_j. The computed z is one number and cancels, left are per pick a(d_j) + 2.5 (its
               own divide), weighted by the renormalised shares w_j in the sum, K - 1 adds and one more divide:
               c_k = 1.25 (|d_k| + D_K) + 0.5 (K - 1) + 9.5 with D_K = sum_j w_j |d_j| over the picks.
  Mixtral (E = 8, K = 2, |d| about 1): c about 10.5 without and 12.5 with renormalisation: 1.3e-6 / 1.5e-6 relative,
  against the 1e-4 / 2e-3 absolute that test_kernels_gpu.py asks for. c is multiplied by 1 + 2^-10 for the
  second-order terms (c 2^-23 < 2^-14 at every |d| < 200). The tolerance is c 2^-23 w + 2^-126: the absolute floor is
  the smallest normal fp32, because v_exp_f32 flushes a subnormal result to 0 and the quotient of a normal by z > 1
  may be flushed likewise; a renormalised weight is exp(d_k) / sum_j exp(d_j) <= exp(d_k) (the first pick has
  d = 0), so what is flushed is below 2^-126 there too. The constant was fixed before any kernel output was seen;
  the measured worst err / tol is in docs/performance.md, "MoE kernels oracle".

Route, exact family. x in {+-1}, wg in {+-2^-s}, s = floor(log2(H) / 2) (the logits of random signs have a standard
deviation of sqrt(H) 2^-s, between 1 and 1.5). Every product is +-2^-s and every partial sum in any order is an
integer multiple of 2^-s below H 2^-s: exact in fp32 with or without fused multiply-adds. The logit's one rounding to
bf16 (RNE) is therefore the same in the kernel and in route_logits(), which rounds the float64 sum. conditions()
asserts sum |x w| 2^s = H < 2^24 and no zero in x or wg. Leaving out or doubling one product moves a logit by 2^-s
(>= 2^-6: a weight moves by about 1 %, tolerance 1e-6).
  * designed (T <= 3): the logits of every row are chosen and then realised in signs. Columns fall into classes
    j mod 4; row t of x is x_0 times a Walsh sign per class, wg_e = 2^-s x_0 v_e with m_{e,c} = (H / 4 - u_{e,c}) / 2
    signs flipped at seeded places of class c, so that logit[t, e] = 2^-s sum_c walsh[t, c] u[e, c] = 4 l[t, e] 2^-s
    (T = 1: one class, 2 l 2^-s). Per row the levels l fall with the rank by seeded gaps of 1 .. 3 except one gap of 0:
    between ranks K - 1 and K (K < E: the tie straddles the cut), between the last two ranks (K = E), between the
    first two (K = 1). The ranks go to the experts by a seeded permutation, mended so that for K >= 2 and E >= 3 the
    first pick has a higher index than the second (slots in index order would differ), and for E in {7, 9} with
    K >= 2 the first pick is expert E - 1 (a clamped router row past E, equal to row E - 1, would be taken next).
    Every row of every designed case therefore decides a tie, and breaking it the other way changes the ids.
  * random (any T): seeded signs. Ties across the cut are frequent but not in every row; used for H = 8 at T = 3
    (8 columns cannot realise three chosen rows) and for the T = 257 case through ops.moe_route, which takes the
    GEMM + topk_softmax path: both paths are tied to one oracle and so to one another.

Topk families ([T, E] bf16 logits).
  * tied: every logit one of {-2, -1, 0, 1}; row 0 all equal. Most rows tie across the cut.
  * ladder: E distinct values (step 1/4 up to E = 8, 1/16 above), permuted per row; row 0 rises with the index, so
    its picks come in falling index order.
  * wide: half the values 0, -1/4, -1/2, .., the other half -86, -86.5, .. (steps of 1 below -128), permuted per
    row: d crosses -87.3, where the fast exp's result turns subnormal and is flushed.
  * nonfinite: the tied family with, by row mod 6, some -inf / fewer than K finite / all -inf / some NaN / all NaN /
    untouched. Held by the kernel only since the selection takes the lowest untaken index when nothing compares
    greater; before, such a row wrote id -1 and moe_align then counted into cnt[-1].

Combine families. exact: ys in +-{1, 2, 3}, resid in +-{1 .. 4}, w[t, k] = DYADIC[(t + 3 k + seed) mod 8] from
+-{1/4, 1/2, 1, 2} (neighbouring tokens never share a weight row). Every term and partial sum is a multiple of 1/4 of
magnitude <= 8 * 2 * 3 + 4 = 52: exact in fp32 in any order, fused or not, and representable in bf16 (208 quarter
steps), so the kernel must equal the oracle bit for bit; squares are multiples of 1/16 and 16 ss < 2^24, so ssp is
exact as well (conditions()). random: randn ys and resid, softmax w: a bf16 output is accepted inside
[RNE(o - delta), RNE(o + delta)], delta = (K + 1) 2^-24 S, S = sum_k |w y| (+ |resid|): K products and K adds of at
most half an ulp of a partial sum below S each (rowwise_reference.judge with c = (K + 1) / 2). The rows after that
rounding are not bit-defined, so ssp is judged against the sum of squares of the rows the kernel wrote, within
rowwise_reference.sumsq_tol (the rows themselves are judged by the bracket, so nothing escapes between the two).

Align is judged by properties (check_align), not by an expected array: the order inside an expert's group follows the
order of LDS atomics and is free.

Sensitivity (the CPU file, per case by name): CLAIMS[name] lists the mutations that have to change the expectation
beyond tolerance in at least MIN_CHANGED rows or elements, in every row or element of a case that holds fewer. The
claims are rules over the case's parameters (claims_of()), written down where each rule is needed:
  * E = 1 claims no routing mutation but the leak without renormalisation (its output is the constant (0, 1));
  * renormalisation skipped / applied needs K < E (the K = E weights already add up to 1);
  * K = 1 with renormalisation has the constant weight 1: only the ids can show anything.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace

import torch

from tests import rowwise_reference as rr

U23 = rr.U23
C_HW = rr.C_HW
C_DIV = 2.5
FLOOR = 2.0 ** -126
SECOND_ORDER = 1 + 2.0 ** -10
MIN_CHANGED = 8
SENT = rr.SENT
SENT_I = -77777            # sentinel of int32 output buffers
SSP_LD = rr.SSP_LD
ROUTE_MAX_E = 16
ROUTE_MAX_T = 256          # ops.moe_route fuses up to here
INF = float("inf")
NAN = float("nan")


# ---------------------------------------------------------------------------------------------- topk

def topk(logits: torch.Tensor, k: int, renorm: bool, tie: str = "low", order: str = "value") -> SimpleNamespace:
    """logits [T, E] (bf16 or float64) -> ids [T, K] int32, w [T, K] float64, tol [T, K], nan_row [T].
    tie = 'high' and order = 'index' are the mutations of the selection rule."""
    g = logits.double()
    t, e = g.shape
    if tie == "low":
        idx = torch.sort(g, dim=-1, descending=True, stable=True).indices
    else:
        idx = e - 1 - torch.sort(g.flip(-1), dim=-1, descending=True, stable=True).indices
    ids = idx[:, :k]
    if order == "index":
        ids = ids.sort(-1).values
    p = torch.softmax(g, -1)
    mx = g.max(-1, keepdim=True).values
    d = (g - mx).abs()
    d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))      # -inf entries: exp(-inf) = 0 exactly
    pk, dk = p.gather(-1, ids), d.gather(-1, ids)
    if renorm:
        w = pk / pk.sum(-1, keepdim=True)
        c = 1.25 * (dk + (w * dk).sum(-1, keepdim=True)) + 0.5 * (k - 1) + 2 * (C_HW + C_DIV) + C_DIV
    else:
        w = pk
        c = 1.25 * (dk + (p * d).sum(-1, keepdim=True)) + 0.5 * (e - 1) + 2 * C_HW + C_DIV
    tol = SECOND_ORDER * c * U23 * w.abs() + FLOOR
    return SimpleNamespace(ids=ids.int(), w=w, tol=tol, nan_row=torch.isnan(g).any(-1), c=c)


def judge_routing(ids: torch.Tensor, w: torch.Tensor, e: SimpleNamespace, num_experts: int) -> SimpleNamespace:
    """Kernel (ids int32 [T, K], w fp32 [T, K]) against the oracle e: errors (list of str) and the worst err / tol."""
    ids, w = ids.cpu().long(), w.cpu().double()
    errs = []
    k = ids.shape[1]
    srt = ids.sort(-1).values
    if not bool(((ids >= 0) & (ids < num_experts)).all()):
        errs.append(f"ids outside [0, {num_experts}): {ids[((ids < 0) | (ids >= num_experts)).any(-1)][:3].tolist()}")
    if k > 1 and not bool((srt[:, 1:] != srt[:, :-1]).all()):
        errs.append("ids repeat within a row")
    clean = ~e.nan_row
    if not torch.equal(ids[clean], e.ids.long()[clean]):
        bad = (ids != e.ids.long()).any(-1) & clean
        r = int(bad.nonzero()[0])
        errs.append(f"{int(bad.sum())} rows of ids differ; row {r}: got {ids[r].tolist()}, want {e.ids[r].tolist()}")
    fin = torch.isfinite(e.w).all(-1)
    ratio = 0.0
    if bool(fin.any()):
        r = ((w[fin] - e.w[fin]).abs() / e.tol[fin])
        r = torch.where(torch.isnan(r), torch.full_like(r, INF), r)
        ratio = float(r.max())
        if ratio > 1:
            errs.append(f"weights: worst err/tol {ratio:.3g}")
    return SimpleNamespace(errs=errs, ratio=ratio)


def rows_changed(e: SimpleNamespace, m: SimpleNamespace) -> torch.Tensor:
    """[T] bool: the mutated expectation m differs from e beyond both tolerances (ids, or a weight)."""
    ids_m = m.ids[:, : e.ids.shape[1]]
    dw = (e.w - m.w[:, : e.w.shape[1]]).abs() > e.tol + m.tol[:, : e.w.shape[1]]
    return (e.ids != ids_m).any(-1) | dw.any(-1)


def enough(changed: torch.Tensor) -> bool:
    """At least MIN_CHANGED rows / elements, or all of a case that holds fewer."""
    n = changed.numel()
    return n > 0 and int(changed.sum()) >= min(MIN_CHANGED, n)


TOPK_T = (1, 255, 256, 257)
TOPK_E = (1, 2, 8, 63, 64, 65, 128, 256)
TOPK_FAMILIES = ("tied", "ladder", "wide", "nonfinite")
TIED_VALUES = (-2.0, -1.0, 0.0, 1.0)


@dataclass(frozen=True)
class TopkCase:
    name: str
    t: int
    e: int
    k: int
    renorm: bool
    family: str
    seed: int


def _topk_cases():
    out = []
    i = 0
    for e in TOPK_E:
        for k in sorted({1, min(2, e), min(e, 8), e}):
            for fam in TOPK_FAMILIES:
                t = TOPK_T[i % 4]
                out.append(TopkCase(f"topk-t{t}-e{e}-k{k}-{'rn' if (i // 4) % 2 else 'raw'}-{fam}", t, e, k,
                                    (i // 4) % 2 == 1, fam, 9000 + i))
                i += 1
            i += 1      # shift the rotation so that every family meets every T and both renorm settings
    return out


TOPK_ALL = _topk_cases()
TOPK_CASES = {c.name: c for c in TOPK_ALL}
TOPK_REFUSED_E = 257


def _permuted(values: torch.Tensor, t: int, gen) -> torch.Tensor:
    perm = torch.rand(t, values.numel(), generator=gen).argsort(-1)
    return values[perm]


@functools.lru_cache(maxsize=8)
def topk_inputs(name: str) -> torch.Tensor:
    """[T, E] bf16 logits."""
    c = TOPK_CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    t, e = c.t, c.e
    tied = torch.tensor(TIED_VALUES, dtype=torch.float64)[torch.randint(0, len(TIED_VALUES), (t, e), generator=gen)]
    if c.family in ("tied", "nonfinite"):
        g = tied
        if c.family == "tied":
            g[0] = g[0, 0]
        else:
            for r in range(t):
                kind = (r + c.seed) % 6
                some = torch.rand(e, generator=gen) < 0.4
                some[int(torch.randint(0, e, (1,), generator=gen))] = True
                if kind == 0:
                    g[r, some] = -INF
                elif kind == 1:
                    g[r, torch.randperm(e, generator=gen)[c.k // 2:]] = -INF     # k // 2 < K finite entries
                elif kind == 2:
                    g[r] = -INF
                elif kind == 3:
                    g[r, some] = NAN
                elif kind == 4:
                    g[r] = NAN
    elif c.family == "ladder":
        vals = (torch.arange(e, dtype=torch.float64) - e // 2) * (0.25 if e <= 8 else 0.0625)
        g = _permuted(vals, t, gen)
        g[0] = vals
    else:
        hi = (e + 1) // 2
        lo = torch.arange(e - hi, dtype=torch.float64)
        vals = torch.cat([-0.25 * torch.arange(hi, dtype=torch.float64),
                          torch.where(lo < 84, -86.0 - 0.5 * lo, -128.0 - (lo - 84))])
        g = _permuted(vals, t, gen)
    out = g.to(torch.bfloat16)
    assert torch.equal(out.double().nan_to_num(7.0), g.nan_to_num(7.0)), "the family's values are bf16 values"
    return out


def topk_expected(name: str, **mut) -> SimpleNamespace:
    """Mutations: tie='high', order='index', flip_renorm=True."""
    c = TOPK_CASES[name]
    renorm = c.renorm != bool(mut.pop("flip_renorm", False))
    return topk(topk_inputs(name), c.k, renorm, **mut)


# ---------------------------------------------------------------------------------------------- route

ROUTE_T = (1, 3)
ROUTE_H = (8, 2040, 2048, 2056, 4096)
ROUTE_E = (1, 7, 8, 9, 16)
ROUTE_REFUSED_E = 17
REFUSED_H = 12
WALSH = ((1, 1, 1, 1), (1, 1, -1, -1), (1, -1, 1, -1))


def route_shift(h: int) -> int:
    return int(math.log2(h)) // 2


def route_em(e: int) -> int:
    """The kernel's compile-time expert count."""
    return 8 if e <= 8 else 16


@dataclass(frozen=True)
class RouteCase:
    name: str
    t: int
    h: int
    e: int
    k: int
    renorm: bool
    strided: bool
    gen: str            # designed | random
    seed: int


def _route_cases():
    out = []
    i = 0
    for h in ROUTE_H:
        for e in ROUTE_E:
            for k in sorted({1, min(2, e), e}):
                t = ROUTE_T[i % 2]
                renorm = (i // 2) % 2 == 1
                strided = (i // 4) % 2 == 1
                gen = "random" if (h == 8 and t == 3) else "designed"
                out.append(RouteCase(f"route-t{t}-h{h}-e{e}-k{k}-{'rn' if renorm else 'raw'}-"
                                     f"{'strided' if strided else 'contig'}", t, h, e, k, renorm, strided, gen,
                                     9500 + i))
                i += 1
    return out


ROUTE_ALL = _route_cases()
ROUTE_FALLBACK = RouteCase("route-t257-h2048-e8-k2-rn-fallback", 257, 2048, 8, 2, True, False, "random", 9499)
ROUTE_CASES = {c.name: c for c in ROUTE_ALL + [ROUTE_FALLBACK]}
ROUTE_FUSED_CASES = [c.name for c in ROUTE_ALL]


def _levels(e: int, k: int, top: int, gen) -> torch.Tensor:
    """[E] falling integer levels by rank with the one gap of 0 that the selection rule has to decide."""
    if e == 1:
        return torch.zeros(1, dtype=torch.long)
    gaps = torch.randint(1, 4, (e - 1,), generator=gen)
    gaps[0 if k == 1 else (k - 1 if k < e else e - 2)] = 0
    lv = torch.cat([torch.zeros(1, dtype=torch.long), -gaps.cumsum(0)])
    lv = lv + min(top, int(-lv[-1]) // 2)
    return lv.clamp_min(-top)


def _assign(lv: torch.Tensor, e: int, k: int, gen) -> torch.Tensor:
    """[E]: the level of each expert: a seeded permutation of the ranks, mended as the docstring says."""
    perm = torch.randperm(e, generator=gen)             # perm[r]: the expert of rank r
    if k >= 2 and e >= 3:
        if e in (7, 9):
            j = int((perm == e - 1).nonzero()[0])
            perm[0], perm[j] = perm[j].clone(), perm[0].clone()
        else:
            grp = (lv == lv[1]).nonzero().flatten()
            grp = grp[grp != 0]
            j = int(grp[perm[grp].argmin()])
            if int(perm[0]) < int(perm[j]):
                perm[0], perm[j] = perm[j].clone(), perm[0].clone()
    out = torch.empty(e, dtype=torch.long)
    out[perm] = lv
    return out


@functools.lru_cache(maxsize=8)
def route_inputs(name: str) -> SimpleNamespace:
    """x [T, H] bf16 in {+-1}, wg [E, H] bf16 in {+-2^-s}, s."""
    c = ROUTE_CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    s = route_shift(c.h)
    sign = lambda *shape: (torch.randint(0, 2, shape, generator=gen) * 2 - 1).double()   # noqa: E731
    if c.gen == "random":
        x, v = sign(c.t, c.h), sign(c.e, c.h)
    else:
        assert c.t in (1, 3)
        ncls = 1 if c.t == 1 else 4
        n_c = c.h // ncls
        top = c.h // 2 - 1 if c.t == 1 else (n_c - 1) // 3     # T = 1: both signs of product stay present
        assert top >= 1, "too few columns to realise the chosen rows"
        lev = torch.stack([_assign(_levels(c.e, c.k, top, gen), c.e, c.k, gen) for _ in range(c.t)])    # [T, E]
        if c.t == 1:
            u = 2 * lev[0][:, None]                                                                   # [E, 1]
        else:
            l3 = lev.sum(0) % 2
            l0, l1, l2 = lev
            u = torch.stack([l0 + l1 + l2 + l3, l0 + l1 - l2 - l3, l0 - l1 + l2 - l3, l0 - l1 - l2 + l3], 1)
        assert bool((u.abs() <= n_c).all()) and bool(((n_c - u) % 2 == 0).all())
        cls = torch.arange(c.h) % ncls
        v = torch.ones(c.e, c.h, dtype=torch.float64)
        for e in range(c.e):
            for q in range(ncls):
                cols = (cls == q).nonzero().flatten()
                m = int(n_c - u[e, q]) // 2
                v[e, cols[torch.randperm(n_c, generator=gen)[:m]]] = -1.0
        x0 = sign(c.h)
        walsh = torch.tensor(WALSH, dtype=torch.float64)[: c.t, :ncls]
        x = x0[None, :] * walsh[:, cls]
        v = v * x0[None, :]
    return SimpleNamespace(c=c, s=s, x=x.to(torch.bfloat16), wg=(v * 2.0 ** -s).to(torch.bfloat16))


def route_logits(x: torch.Tensor, wg: torch.Tensor, drop=None, double=None) -> torch.Tensor:
    """[T, E] float64 holding bf16 values: x wg^T in float64, rounded once (RNE). drop / double: [T] expert and
    column of the one product per row that is left out / counted twice."""
    prod = x.double()[:, None, :] * wg.double()[None, :, :]                 # [T, E, H]
    for sel, f in ((drop, 0.0), (double, 2.0)):
        if sel is not None:
            e, j = sel
            r = torch.arange(prod.shape[0])
            prod[r, e, j] = prod[r, e, j] * f
    return rr.rne_bf16(prod.sum(-1))


def route_expected(name: str, **mut) -> SimpleNamespace:
    """Mutations: drop / double (one product of the last pick's logit per row, chosen so that the logit falls by
    2^-s), leak (the clamped router rows E .. EM - 1 enter unmasked), tie, order, flip_renorm."""
    i = route_inputs(name)
    c = i.c
    renorm = c.renorm != bool(mut.pop("flip_renorm", False))
    kind = next((m for m in ("drop", "double") if mut.pop(m, False)), None)
    leak = mut.pop("leak", False)
    sel = {}
    if kind:
        base = topk(route_logits(i.x, i.wg), c.k, renorm)
        e_sel = base.ids[:, -1].long()
        prod = i.x.double() * i.wg.double()[e_sel]                           # [T, H]
        want = prod > 0 if kind == "drop" else prod < 0
        assert bool(want.any(-1).all())
        sel[kind] = (e_sel, want.double().argmax(-1))
    g = route_logits(i.x, i.wg, **sel)
    if leak:
        g = torch.cat([g, g[:, -1:].expand(-1, route_em(c.e) - c.e)], 1)
    return topk(g, c.k, renorm, **mut)


# ---------------------------------------------------------------------------------------------- align

ALIGN_N = (0, 1, 1023, 1024, 1025, 4099)
ALIGN_E = (1, 8, 9, 256)
ALIGN_DISTS = ("uniform", "one", "ends_empty", "null", "distinct")
ALIGN_REFUSED_E = 257
ALIGN_K = {1023: 3, 1024: 4, 1025: 5}      # 'distinct': tokens of K slots with K distinct experts (else K = 1)


@dataclass(frozen=True)
class AlignCase:
    name: str
    n: int
    e: int
    dist: str
    seed: int


ALIGN_ALL = [AlignCase(f"align-n{n}-e{e}-{d}", n, e, d, 9800 + 31 * a + 7 * b + q)
             for a, n in enumerate(ALIGN_N) for b, e in enumerate(ALIGN_E) for q, d in enumerate(ALIGN_DISTS)
             if not (d == "ends_empty" and e < 3)]
ALIGN_CASES = {c.name: c for c in ALIGN_ALL}


def align_ids(name: str) -> torch.Tensor:
    """[n] int32 expert ids; 'null': every assignment in the last group (expert parallelism: groups = E, all
    remote)."""
    c = ALIGN_CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    if c.dist == "uniform":
        ids = torch.randint(0, c.e, (c.n,), generator=gen)
    elif c.dist == "one":
        ids = torch.full((c.n,), c.e // 2)
    elif c.dist == "null":
        ids = torch.full((c.n,), c.e - 1)
    elif c.dist == "ends_empty":
        ids = torch.randint(1, c.e - 1, (c.n,), generator=gen)
    else:
        k = min(ALIGN_K.get(c.n, 1), c.e)
        ids = torch.rand(c.n // k if k else 0, c.e, generator=gen).argsort(-1)[:, :k].reshape(-1)
        assert ids.numel() == c.n
    return ids.int()


def check_align(offsets, sorted_idx, pos, ids, num_experts: int) -> list:
    """The contract of moe_align as a list of violations (empty: holds). offsets [E + 1], sorted, pos [n]."""
    offsets, sorted_idx, pos, ids = (t.cpu().long() for t in (offsets, sorted_idx, pos, ids))
    n = ids.numel()
    errs = []
    want = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(ids, minlength=num_experts).cumsum(0)])
    if not torch.equal(offsets, want):
        errs.append("offsets are not the exclusive cumsum of the expert histogram")
    if not torch.equal(sorted_idx.sort().values, torch.arange(n)):
        errs.append("sorted is no permutation of 0 .. n - 1")
        return errs
    group = torch.bucketize(torch.arange(n), want[1:], right=True)          # the expert whose range holds j
    if not torch.equal(ids[sorted_idx], group):
        errs.append("an entry of sorted lies in another expert's range")
    if not (bool(((pos >= 0) & (pos < n)).all()) and torch.equal(pos[sorted_idx], torch.arange(n))):
        errs.append("pos is not the inverse of sorted")
    return errs


def align_model(ids: torch.Tensor, num_experts: int):
    """One valid answer (the stable one), for the CPU file and for hand-made wrong answers."""
    ids = ids.long()
    srt = torch.sort(ids, stable=True).indices
    pos = torch.empty_like(srt)
    pos[srt] = torch.arange(ids.numel())
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(ids, minlength=num_experts).cumsum(0)])
    return off.int(), srt.int(), pos.int()


# ---------------------------------------------------------------------------------------------- gather

GATHER_T = 9
GATHER_E = 8


@dataclass(frozen=True)
class GatherCase:
    name: str
    h: int
    k: int
    source: str         # align | hand
    seed: int


GATHER_ALL = [GatherCase(f"gather-h{h}-k{k}-{src}", h, k, src, 9900 + 10 * a + 2 * b + q)
              for a, h in enumerate((8, 2048, 2056)) for b, k in enumerate((1, 2, 4)) for q, src in
              enumerate(("align", "hand"))]
GATHER_CASES = {c.name: c for c in GATHER_ALL}


def gather_inputs(name: str) -> SimpleNamespace:
    """x [GATHER_T, H] bf16 whose 16-bit patterns count up (every chunk different); ids [T * K] for the 'align'
    source (the sorted order then comes from an align), sorted [T * K] for 'hand' (the reversal, rotated by 2)."""
    c = GATHER_CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    n = GATHER_T * c.k
    x = (torch.arange(GATHER_T * c.h, dtype=torch.int32) % 32000 + 128).to(torch.int16).view(torch.bfloat16).view(
        GATHER_T, c.h)
    i = SimpleNamespace(c=c, x=x, ids=torch.randint(0, GATHER_E, (n,), generator=gen).int())
    i.sorted = torch.arange(n - 1, -1, -1).roll(2).int() if c.source == "hand" else None
    return i


def gathered(x: torch.Tensor, sorted_idx: torch.Tensor, k: int, mod: bool = False) -> torch.Tensor:
    """xs[j] = x[sorted[j] // K]; mod: the mutation sorted[j] % K."""
    s = sorted_idx.cpu().long()
    return x[(s % k) if mod else (s // k)]


# ---------------------------------------------------------------------------------------------- combine

COMBINE_T = (1, 5, 128)
COMBINE_K = (1, 2, 4, 8)
COMBINE_H = (8, 2040, 2048, 2056, 4104)
COMBINE_REFUSED_T = 129
DYADIC = (0.25, -0.5, 1.0, -2.0, -0.25, 0.5, -1.0, 2.0)


@dataclass(frozen=True)
class CombineCase:
    name: str
    t: int
    k: int
    h: int
    family: str         # exact | random
    strided: bool       # the residual form's resid
    seed: int


def _combine_cases():
    out = []
    i = 0
    for h in COMBINE_H:
        for k in COMBINE_K:
            t = (1, 5)[i % 2]
            out.append(CombineCase(f"combine-t{t}-k{k}-h{h}-exact", t, k, h, "exact", (i // 2) % 2 == 1, 9950 + i))
            i += 1
        i += 1
    for k in COMBINE_K:
        out.append(CombineCase(f"combine-t128-k{k}-h8-exact", 128, k, 8, "exact", k in (2, 8), 9990 + k))
    out.append(CombineCase("combine-t128-k2-h2048-exact", 128, 2, 2048, "exact", True, 9989))
    out.append(CombineCase("combine-t5-k2-h2056-random", 5, 2, 2056, "random", True, 9988))
    out.append(CombineCase("combine-t9-k8-h4104-random", 9, 8, 4104, "random", False, 9987))
    return out


COMBINE_ALL = _combine_cases()
COMBINE_CASES = {c.name: c for c in COMBINE_ALL}


def _ints(gen, shape, a):
    mag = torch.randint(1, a + 1, shape, generator=gen)
    return (mag * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).to(torch.bfloat16)


@functools.lru_cache(maxsize=4)
def combine_inputs(name: str) -> SimpleNamespace:
    """ys [T K, H] bf16, resid [T, H] bf16, w [T, K] fp32, pos [T K] int32 (a seeded permutation without a fixed
    point wherever T K > 1)."""
    c = COMBINE_CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    n = c.t * c.k
    i = SimpleNamespace(c=c)
    if c.family == "exact":
        i.ys, i.resid = _ints(gen, (n, c.h), 3), _ints(gen, (c.t, c.h), 4)
        idx = (torch.arange(c.t)[:, None] + 3 * torch.arange(c.k)[None, :] + c.seed) % len(DYADIC)
        i.w = torch.tensor(DYADIC, dtype=torch.float32)[idx]
    else:
        i.ys = torch.randn(n, c.h, generator=gen).to(torch.bfloat16)
        i.resid = torch.randn(c.t, c.h, generator=gen).to(torch.bfloat16)
        i.w = torch.softmax(torch.randn(c.t, c.k, generator=gen), -1).float()
    perm = torch.randperm(n, generator=gen)
    i.pos = perm.int()
    if n > 1:           # a cyclic shift of a permutation's values along its own order has no fixed point
        inv = torch.empty(n, dtype=torch.long)
        inv[perm] = torch.arange(n)
        i.pos = perm[(inv + 1) % n].int()
    return i


def combine_expected(name: str, residual: bool, **mut) -> SimpleNamespace:
    """o [T, H] float64 (before the rounding), s = sum of the magnitudes of its terms, h = RNE_bf16(o) as float64, ss
    [T] = the sum of squares of h (mutation unrounded: of o), exact (bool), c for rowwise_reference.judge.
    Mutations: drop / double (the last term of every row), shift_pos, shift_w (the next token's), unrounded."""
    i = combine_inputs(name)
    c = i.c
    pos, w = i.pos.long().view(c.t, c.k), i.w.double()
    if mut.get("shift_pos"):
        pos = pos.roll(-1, 0)
    if mut.get("shift_w"):
        w = w.roll(-1, 0)
    terms = w[:, :, None] * i.ys.double()[pos]                               # [T, K, H]
    if mut.get("drop"):
        terms = terms[:, :-1]
    if mut.get("double"):
        terms = torch.cat([terms, terms[:, -1:]], 1)
    e = SimpleNamespace(exact=c.family == "exact", c=(c.k + 1) / 2.0)
    e.o, e.s = terms.sum(1), terms.abs().sum(1)
    if residual:
        e.o, e.s = e.o + i.resid.double(), e.s + i.resid.double().abs()
    e.h = rr.rne_bf16(e.o)
    e.ss = (e.o if mut.get("unrounded") else e.h).pow(2).sum(-1)
    e.ss_tol = torch.zeros_like(e.ss) if e.exact else rr.sumsq_tol(e.ss, c.h)
    return e


def elements_changed(e: SimpleNamespace, m: SimpleNamespace) -> torch.Tensor:
    """[T, H] bool: the mutated expectation's bracket does not hold the original's rounded value (exact: differs)."""
    if e.exact:
        return e.h != m.h
    return rr.changed(e.o, e.s, m.o, m.s, e.c)


# ---------------------------------------------------------------------------------------------- exactness premises

def conditions(name: str) -> None:
    """Asserts the premises under which the case is compared bit for bit."""
    if name in ROUTE_CASES:
        i = route_inputs(name)
        x, wg = i.x.double(), i.wg.double() * 2.0 ** i.s
        assert bool((x.abs() == 1).all()) and bool((wg.abs() == 1).all()), f"{name}: a zero or non-unit factor"
        assert i.c.h < 2 ** 24, name                                         # sum |x w| in units of 2^-s
        assert 0 <= i.s <= 6 and 1.0 <= math.sqrt(i.c.h) * 2.0 ** -i.s <= 2.0, name
    elif name in COMBINE_CASES and COMBINE_CASES[name].family == "exact":
        i = combine_inputs(name)
        c = i.c
        assert bool((i.ys.double() != 0).all()) and bool((i.resid.double() != 0).all()), name
        assert bool((i.ys.double() == i.ys.double().round()).all()), name
        w4 = i.w.double() * 4
        assert bool((w4 == w4.round()).all()) and bool((w4 != 0).all()), name
        assert bool((i.w[1:] != i.w[:-1]).all()) and (c.t == 1 or bool((i.w[0] != i.w[-1]).all())), name
        bound = (i.w.double().abs()[:, :, None] * i.ys.double().abs()[i.pos.long().view(c.t, c.k)]).sum(1) \
            + i.resid.double().abs()
        assert float(bound.max()) <= 256 and float(bound.max()) * 4 < 256, f"{name}: a sum leaves bf16's 8 bits"
        for residual in (False, True):
            e = combine_expected(name, residual)
            assert torch.equal(e.h, e.o), name                               # nothing is rounded away
            assert float(e.ss.max()) * 16 < 2 ** 24, f"{name}: ss leaves fp32's integers"
    else:
        raise KeyError(name)


# ---------------------------------------------------------------------------------------------- claims

def claims_of(c) -> tuple:
    """The mutations a case has to notice (rules over its parameters; see the docstring)."""
    if isinstance(c, TopkCase):
        out = []
        if c.family == "tied" and c.e >= 2:
            out.append("tie_high")
        if c.family == "ladder" and c.k >= 2:
            out.append("index_order")
        if c.family in ("tied", "ladder") and c.k < c.e:
            out.append("renorm_skipped" if c.renorm else "renorm_applied")
        return tuple(out)
    if isinstance(c, RouteCase):
        out = []
        if c.e >= 2 and (c.gen == "designed" or not (c.k == 1 and c.renorm)):
            out += ["drop", "double"]
        if c.e >= 2 and (c.gen == "designed" or c.t >= 255):
            out.append("tie_high")
        if c.k >= 2 and c.e >= 3 and (c.gen == "designed" or c.t >= 255):
            out.append("index_order")
        if c.k < c.e:
            out.append("renorm_skipped" if c.renorm else "renorm_applied")
        if c.e < route_em(c.e) and (not c.renorm or (c.gen == "designed" and c.k >= 2 and c.e >= 2)):
            out.append("leak")
        return tuple(out)
    if isinstance(c, CombineCase):
        out = ["drop", "double"]
        if c.t >= 2:
            out += ["shift_pos", "shift_w"]
        if c.family == "random":
            out.append("unrounded")
        return tuple(out)
    raise TypeError(c)


CLAIMS = {c.name: claims_of(c) for c in TOPK_ALL + ROUTE_ALL + [ROUTE_FALLBACK] + COMBINE_ALL}
ROUTING_MUTATIONS = {"tie_high": dict(tie="high"), "index_order": dict(order="index"),
                     "renorm_skipped": dict(flip_renorm=True), "renorm_applied": dict(flip_renorm=True),
                     "drop": dict(drop=True), "double": dict(double=True), "leak": dict(leak=True)}
