"""Not a test: the float64 oracle of paged attention, the tolerance derived from the kernels' rounding steps, and
the seeded input families that test_attention_reference_cpu.py (conditions on the inputs) and
test_attention_kernel_gpu.py (the kernels) share.

Oracle. `oracle()` is causal paged attention with GQA in float64 on the inputs exactly as a kernel receives them
(bf16 q, paged bf16 caches, block tables, the arguments of src/ops/reference.attention). Per output element it
returns o = sum_j p_j v_j, a = sum_j p_j |v_j| and, for the fused paths, the score-slack term below.
`fused_step()` models the fused decode prologue (fp32 slabs summed, scaled by rsqrt(sum of the statistics tiles /
hidden + eps), RoPE at ctx - 1, q and the new k / v rounded to bf16 where the kernel rounds them, the caches after
the step: slot -1 writes nothing, the row still attends to its new token); `rope_q()` models the prefill kernel's
RoPE-on-load with q_scale, rounded to bf16 at the same point.

Tolerance (derived, not tuned). The kernels convert fp32 to bf16 with v_cvt_pk_bf16_f32 (round to nearest even,
common.h: pack2 / f2bf). bf16 keeps 8 significant bits: half an ulp is 2^-9 of the binade's upper end and up to
u = 2^-8 of the value itself (just above a power of two). The places where the kernels round:
  1. P is rounded to bf16 before the PV MFMA while l sums the unrounded p: the numerator moves by at most
     sum_j u p_j |v_j|, the denominator not at all: |err| <= u a. (The lazy rescale keeps p <= 2^8, and a relative
     error does not care; bf16 x bf16 products are exact in the MFMA's fp32 accumulator.)
  2. The output is rounded once: |err| <= u |o|.
  3. fp32 accumulation over n keys (<= n 2^-24 relative, n <= 2,049 here: 2^-13), v_exp_f32 (about 1 ulp of fp32)
     and the fp32 scale constant (score (1 + 2^-23): p moves by < 1e-5 relative at a score range of 90 log2 units)
     are orders of magnitude below 1. and 2.
Hence |err| <= 2^-8 (|o| + a) to first order, and tol = 2^-8 (|o| + a) + 1e-6; the 1e-6 floor (outputs that are
exactly 0 in the oracle and 1e-8 in fp32) is the only chosen number. The formula was set with the two steps at 2^-9
each, which would make it twice the bound; with u = 2^-8 it is the bound itself, and the measurements agree: the
flat family (p = 1 exactly, so only step 2 acts, and a = |o|) reaches err / tol = 0.47 of a possible 0.5, and the
witness family (equal p, all rounded the same way) 0.91 of a possible 1. Step 3 is what is left of the margin.

Fused paths only (decode prologue, prefill RoPE-on-load). The oracle rotates in float64, the kernel in fp32; where
the exact value lies within fp32 error of a rounding midpoint the two round a q or k element to neighbouring bf16
values, one ulp <= 2^-7 |x| apart. If every element of q moved so, the score of key j would move by at most
2 eps_j, eps_j = 2^-8 scale sum_d |q_d k_jd|, its p_j by the factor exp(+-2 eps_j), and o by at most
slack = 2 sum_j p_j eps_j (|v_j| + |o|), which is added to tol. (The step's new key can move as well, which doubles
its own eps; a flip needs the exact value within 2^-20 relative of a midpoint, about one element in 2^12, so the
all-elements bound covers it amply.) That bound is loose: at these inputs it is as large as the old tolerance. The
oracle therefore also marks the elements that CAN flip (exact value within 2^-20 mag of a midpoint, mag as below;
flip_move()) and evaluates the same expression with the true ulp of only those elements of q, of the new key and of
the new value: `flip`, zero for most rows. The GPU tests assert both tol (with slack) and the tighter base + flip,
and the sensitivity conditions are proved against the tighter one. The new k / v rows written to the cache are
checked the same way: a kernel value y is accepted iff |y - x| <= half an ulp + 2^-20 mag, x the float64 value
before rounding and mag the sum of the magnitudes of the rotation's two products (fp32 error of <= sk + 12
operations: the slab sum, the statistics sum, v_rsq_f32, the scale, the rotation).

Input families (every case complete and seeded; block ids scattered; table entries past a context name a block
full of NaN, and so are the rows past the context inside its last block):
  flat       q = 0, K random, V[key j] = amp(seq, kv head) e_el(j) with distinct bf16-exact amps <= 0.75 and
             el(j) = j mod 128, but c + 64 for key c of chunk c (flat_element: a dropped chunk would otherwise leave a
             context of whole chunks unchanged): o_d = amp count_d / ctx exactly. A key dropped, counted twice,
             taken from another pair or mis-weighted in a merge shows in one element.
  staircase  q = u, K[j] = level(j) u, u = +-1 on 16 dims, scale = ln 2 / 16: every score is level(j) log2 units,
             every p a power of two. Levels are constant over 32-key tiles and step by +9, +7, +9, +7, -20 between a
             wave's consecutive tiles (128 keys apart in decode, 32 in prefill): both sides of the lazy-rescale
             threshold of 8, and a drop. The net step is positive, so the top levels sit in the last chunks. V as
             in flat; the output is a ratio of sums of powers of two.
  witness    a random base plus witness keys W that hold nearly all the weight in equal shares: the group's q rows
             carry 6 u on u's 16 dims, the witness K rows are exactly u. Decode: first and last key (the step's
             new token), and for at most three chunk edges (first, last, one seeded) both sides of the edge and of
             the block edges 16 keys either side. Prefill: keys 0, pos0 - 1, pos0, ctx - 1 and the rows' own
             positions on both sides of every 32-row edge. Witness V rows are distinct +-0.75 sign patterns.
  random     bf16 randn q and K, V = 0.25 randn clamped to +-0.75.
Why the caps: dropping a key of weight w moves an element by about 0.75 w while tol is about 2^-8 0.75, a ratio
of 256 w; the >= 4x sensitivity that the CPU test demands therefore needs w >= 1/64, which neither the 92 edge
keys of a 2,048-key context nor a witness at every prefill row can have. And V magnitudes stay <= 0.75 because at
a one-key context |o| = a = |v|, so tol = 2^-7 |v| must stay below a quarter of the old 2.5e-2.
"""

from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import torch

from src.ops import reference as ref
from src.ops.decode_tiles import SSP_LD

D, HID, EPS = 128, 1024, 1e-5
BF16 = torch.bfloat16
F64 = torch.float64
FAMILIES = ("flat", "staircase", "witness", "random")
LN2 = math.log(2.0)
V_MAX = 0.75
Q_BOOST = 6.0
# distinct bf16-exact amplitudes in [0.125, 0.75], largest first
AMPS = [0.75 - k / 256 for k in range(65)] + [0.5 - (k + 1) / 512 for k in range(128)] + \
       [0.25 - (k + 1) / 1024 for k in range(128)]
STEPS = (9, 7, 9, 7, -20)
STALE_K, STALE_V = 1.0, -1.5   # a new token's cache row before the fused step writes it


def bf(x: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16, round to nearest even (through fp32: exact unless within 2^-24 of a midpoint)."""
    return x.float().to(BF16)


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _u0() -> torch.Tensor:
    u = torch.zeros(D, dtype=F64)
    u[:16] = torch.tensor([1, -1, 1, 1, -1, 1, -1, -1, 1, 1, -1, 1, -1, -1, -1, 1], dtype=F64)
    return u


U0 = _u0()


# ------------------------------------------------------------------------------------------------ oracle
def _terms(q, kc, vc, bt_row, qlen, ctx, hq, hkv, scale):
    """One sequence in float64: e [hq, qlen, ctx] (exp of the causally masked scores minus the row max), v and k
    [ctx, hq, D] (kv heads repeated over their groups), q [qlen, hq, D]."""
    g = hq // hkv
    qs = q.double().reshape(qlen, hq, D)
    k = ref.gather_kv(kc, bt_row, ctx).double().repeat_interleave(g, dim=1)
    v = ref.gather_kv(vc, bt_row, ctx).double().repeat_interleave(g, dim=1)
    sc = torch.einsum("qhd,khd->hqk", qs, k) * scale
    qpos = torch.arange(ctx - qlen, ctx)[:, None]
    kpos = torch.arange(ctx)[None, :]
    vis = (kpos <= qpos)[None]
    sc = sc.masked_fill(~vis, float("-inf"))
    e = torch.exp(sc - sc.max(-1, keepdim=True).values)
    return e, v, qs, k


def _finish(e, v, keep=None):
    if keep is not None:
        e = e * keep.double()[None, None, :]
    l = e.sum(-1)
    p = e / l.clamp_min(1e-300)[..., None]
    o = torch.einsum("hqk,khd->qhd", p, v)
    a = torch.einsum("hqk,khd->qhd", p, v.abs())
    return p, o, a


def oracle(q, kc, vc, bt, cu_q, ctx_lens, hq, hkv, scale, slack=False, keep=None, moves=None):
    """float64 causal paged attention. Returns (o, a, slack, flip) [T, hq, D]; slack (the all-elements bound of the
    module docstring) and flip are zero unless slack is asked for. flip is the same bound restricted to the elements
    that can in fact round the other way: moves = (dq [T, hq, D], dk [n, hkv, D], dv [n, hkv, D]), the size of the
    possible move of every q element and of every element of each sequence's LAST key / value row (0 = cannot
    flip; flip_move()). keep: per sequence a bool [ctx] (False = the key does not exist), for the sensitivity
    checks."""
    t = q.shape[0]
    g = hq // hkv
    o = torch.zeros(t, hq, D, dtype=F64)
    a = torch.zeros_like(o)
    sl = torch.zeros_like(o)
    fl = torch.zeros_like(o)
    for s in range(len(ctx_lens)):
        b0, b1 = int(cu_q[s]), int(cu_q[s + 1])
        qlen, ctx = b1 - b0, int(ctx_lens[s])
        if qlen == 0:
            continue
        e, v, qs, k = _terms(q[b0:b1, : hq * D], kc, vc, bt[s], qlen, ctx, hq, hkv, scale)
        p, o[b0:b1], a[b0:b1] = _finish(e, v, None if keep is None else keep[s])
        if not slack:
            continue
        oa = o[b0:b1].abs()

        def bound(pe):  # sum_j pe_j (|v_j| + |o|)
            return torch.einsum("hqk,khd->qhd", pe, v.abs()) + pe.sum(-1).t()[..., None] * oa
        sl[b0:b1] = 2 * bound(p * (torch.einsum("qhd,khd->hqk", qs.abs(), k.abs()) * (scale * 2.0 ** -8)))
        if moves is not None:
            dq = moves[0][b0:b1]
            eps = torch.einsum("qhd,khd->hqk", dq, k.abs())
            dk = moves[1][s].repeat_interleave(g, dim=0)                              # [hq, D]
            eps[:, :, ctx - 1] += torch.einsum("qhd,hd->hq", qs.abs() + dq, dk)
            fl[b0:b1] = 2 * bound(p * eps * scale)
            fl[b0:b1] += p[:, :, ctx - 1].t()[..., None] * moves[2][s].repeat_interleave(g, dim=0)[None]
    return o, a, sl, fl


def flip_move(x, delta):
    """Where the float64 x lies within delta of a bf16 rounding midpoint: the distance of the two candidates (one
    ulp), else 0."""
    ax = x.abs().clamp_min(2.0 ** -126)
    u = torch.exp2(torch.floor(torch.log2(ax)) - 7)
    fr = ax / u - torch.floor(ax / u)
    return torch.where((fr - 0.5).abs() * u <= delta, u, torch.zeros_like(u))


def tolerance(o, a, slack=None):
    t = 2.0 ** -8 * (o.abs() + a) + 1e-6
    return t if slack is None else t + slack


def drop_ratios(c, s, sets=None, keys=None, rows=None):
    """Sequence s of case c with each key set of `sets` (bool [B, ctx]) removed: max over the elements of the
    given q rows (default all) of |o_without - o| / tol, one figure per set; or, with `keys`, one figure per
    single key, judged on one q row each (default row 0). Leave-out form of the same sums
    (numerator and denominator minus the set's share); test_attention_reference_cpu checks it against oracle(keep=)."""
    q, kc, vc = c.oracle_inputs()
    b0, b1 = int(c.cu[s]), int(c.cu[s + 1])
    ctx = c.ctxs[s]
    e, v, qs, k = _terms(q[b0:b1, : c.hq * D], kc, vc, c.bt[s], b1 - b0, ctx, c.hq, c.hkv, c.scale)
    tol = c.expected().tight[b0:b1]
    o = c.expected().o[b0:b1]
    num = torch.einsum("hqk,khd->qhd", e, v)
    den = e.sum(-1).t()
    out = []
    if sets is None:  # single keys, each judged on one q row (default row 0): vectorised
        keys = torch.as_tensor(keys)
        r = torch.zeros_like(keys) if rows is None else torch.as_tensor(rows)
        for i in range(0, len(keys), 256):
            kk, rr = keys[i:i + 256], r[i:i + 256]
            ej = e[:, rr, kk].t()                                   # [B, hq]
            n2 = num[rr] - ej[..., None] * v[kk]
            d2 = den[rr] - ej
            o2 = torch.where(d2[..., None] > 1e-12 * den[rr][..., None], n2 / d2.clamp_min(1e-300)[..., None],
                             torch.zeros_like(n2))
            out += ((o2 - o[rr]).abs() / tol[rr]).amax((1, 2)).tolist()
        return out
    if rows is None:
        rows = [slice(None)] * len(sets)
    for m, r in zip(sets, rows):
        em = e[:, r] * m.double()[None, None, :]
        n2 = num[r] - torch.einsum("hqk,khd->qhd", em, v)
        d2 = den[r] - em.sum(-1).t()
        # a row that loses every visible key has no output: the kernels write 0 for it
        o2 = torch.where(d2[..., None] > 1e-12 * den[r][..., None], n2 / d2.clamp_min(1e-300)[..., None],
                         torch.zeros_like(n2))
        out.append(float(((o2 - o[r]).abs() / tol[r]).max()))
    return out


# ------------------------------------------------------------------------------------------------ families
def levels(ctx: int, stride: int) -> torch.Tensor:
    """Staircase level of every key: tiles of 32 keys; a wave's consecutive tiles (`stride` tiles apart) step by
    STEPS, the tiles of one step differ by one level each (the waves of a decode chunk merge distinct maxima)."""
    t = torch.arange(ctx) // 32
    step, w = t // stride, t % stride
    base = [8]
    for i in range(int(step.max()) if ctx else 0):
        base.append(base[-1] + STEPS[i % len(STEPS)])
    return torch.tensor(base)[step] + w


def flat_element(j: torch.Tensor) -> torch.Tensor:
    """The element that key j's V row lights: j mod 128, except that key c of chunk c goes to element c + 64, so
    that whole chunks are not interchangeable (with j mod 128 alone a context of whole chunks would give the same
    output without any one of them)."""
    el = j % D
    return torch.where(el == (j // D) % D, (el + 64) % D, el)


def top_tiles(ctx: int, stride: int):
    """Key masks [B, ctx] of the 32-key tiles whose level is within one of the context's highest."""
    lv = levels(ctx, stride)
    t = torch.arange(ctx) // 32
    tiles = sorted({int(x) for x in t[lv >= lv.max() - 1]})
    return torch.stack([t == x for x in tiles])


def decode_witnesses(ctx: int, seed: int):
    w = {0, ctx - 1}
    edges = list(range(128, ctx, 128))
    pick = set(edges[:1] + edges[-1:])
    if len(edges) > 2:
        pick.add(edges[1 + seed % (len(edges) - 2)])
    for e in pick:
        w.update(x for x in (e - 17, e - 16, e - 1, e, e + 15, e + 16) if 0 <= x < ctx)
    return sorted(w)


def prefill_witnesses(qlen: int, ctx: int):
    pos0 = ctx - qlen
    w = {0, max(pos0 - 1, 0), pos0, ctx - 1}
    for i in range(32, qlen, 32):
        w.update((pos0 + i - 1, pos0 + i))
    return sorted(w)


def _logical(family, n, qlens, ctxs, g, hkv, seed, stride):
    """Per-sequence q [qlen, hq, D], K / V [ctx, hkv, D] (bf16-exact values in float64), witnesses, closed form."""
    gen = _gen(seed)
    hq = g * hkv
    qs, ks, vs, wit, closed = [], [], [], [], []
    for s in range(n):
        qlen, ctx = qlens[s], ctxs[s]
        pos0 = ctx - qlen
        q = torch.randn(qlen, hq, D, generator=gen).to(BF16).double()
        k = torch.randn(ctx, hkv, D, generator=gen).to(BF16).double()
        v = (0.25 * torch.randn(ctx, hkv, D, generator=gen)).clamp(-V_MAX, V_MAX).to(BF16).double()
        w, cf = [], None
        if family in ("flat", "staircase"):
            amp = torch.tensor([AMPS[(s * hkv + h) % len(AMPS)] for h in range(hkv)], dtype=F64)
            v = torch.zeros(ctx, hkv, D, dtype=F64)
            j = torch.arange(ctx)
            el = flat_element(j)
            v[j, :, el] = amp[None, :].expand(ctx, hkv)
            if family == "flat":
                q = torch.zeros_like(q)
                wt = torch.ones(ctx, dtype=F64)
            else:
                lv = levels(ctx, stride)
                q = U0.expand(qlen, hq, D).clone()
                k = lv.double()[:, None, None] * U0.expand(ctx, hkv, D)
                wt = None
            # closed form: o[row i, element d] = amp * sum_{j <= pos0 + i, el(j) = d} w_j / sum_{j <= pos0 + i} w_j
            cf = torch.zeros(qlen, hq, D, dtype=F64)
            for i in range(qlen):
                nvis = pos0 + i + 1
                if wt is None:
                    lvv = lv[:nvis]
                    wv = torch.ldexp(torch.ones(nvis, dtype=F64), (lvv - lvv.max()))
                else:
                    wv = wt[:nvis]
                cnt = torch.zeros(D, dtype=F64).index_add_(0, el[:nvis], wv)
                cf[i] = (cnt / wv.sum())[None, :] * amp.repeat_interleave(g)[:, None]
        elif family == "witness":
            w = decode_witnesses(ctx, seed + s) if stride == 4 else prefill_witnesses(qlen, ctx)
            q[..., :16] = Q_BOOST * U0[:16]
            wi = torch.tensor(w)
            k[wi] = U0.expand(len(w), hkv, D)
            pat = torch.where(torch.rand(len(w), hkv, D, generator=gen) < 0.5, -V_MAX, V_MAX).double()
            flat = pat.transpose(0, 1).reshape(hkv, len(w), D)
            for h in range(hkv):
                assert len({tuple(r.tolist()) for r in flat[h]}) == len(w), "witness V rows must be distinct"
            v[wi] = pat
        qs.append(q)
        ks.append(k)
        vs.append(v)
        wit.append(w)
        closed.append(cf)
    return qs, ks, vs, wit, closed


def _page(ks, vs, ctxs, hkv, bs, cols, seed):
    """Scattered block ids; entries past a context name the NaN block; rows past a context are NaN too."""
    gen = _gen(seed + 7919)
    n = len(ctxs)
    need = [(c + bs - 1) // bs for c in ctxs]
    cols = max(cols, max(need))
    total = sum(need) + 1
    perm = torch.randperm(total, generator=gen).tolist()
    poison = perm.pop()
    bt = torch.full((n, cols), poison, dtype=torch.int32)
    kc = torch.full((total, hkv, bs, D), float("nan"), dtype=BF16)
    vc = torch.full((total, hkv, bs, D), float("nan"), dtype=BF16)
    for s, nb in enumerate(need):
        ids = torch.tensor([perm.pop() for _ in range(nb)], dtype=torch.int32)
        bt[s, :nb] = ids
        pos = torch.arange(ctxs[s])
        blk = ids.long()[pos // bs]
        kc[blk, :, pos % bs] = ks[s].to(BF16)
        vc[blk, :, pos % bs] = vs[s].to(BF16)
    return kc, vc, bt, poison


class Case(SimpleNamespace):
    def oracle_inputs(self):
        """(q, k cache, v cache) as the attention proper sees them: after the fused prologue / the RoPE-on-load."""
        if self.fused is not None:
            f = fused_step(self)
            return f.q, f.k_att, f.v_att
        if self.cs is not None:
            return rope_q(self)[0], self.kc, self.vc
        return self.q, self.kc, self.vc

    def expected(self):
        """o, a, slack, flip of the case and its two tolerances (tol: the all-elements slack; tight: only the
        elements that can flip; both the plain tolerance where nothing is fused), computed once."""
        if self._exp is None:
            q, kc, vc = self.oracle_inputs()
            moves = None
            if self.fused is not None:
                moves = fused_step(self).moves
            elif self.cs is not None:
                z = torch.zeros(self.n, self.hkv, D, dtype=F64)
                moves = (rope_q(self)[1], z, z)
            fz = moves is not None
            o, a, sl, fl = oracle(q, kc, vc, self.bt, self.cu, self.ctxs, self.hq, self.hkv, self.scale, slack=fz,
                                  moves=moves)
            self._exp = SimpleNamespace(o=o, a=a, slack=sl, flip=fl, base=tolerance(o, a),
                                        tol=tolerance(o, a, sl if fz else None),
                                        tight=tolerance(o, a, fl if fz else None))
        return self._exp


def make_case(name, family, qlens, ctxs, g, hkv, bs=16, max_ctx=None, seed=0, stride=4):
    n, hq = len(ctxs), g * hkv
    qs, ks, vs, wit, closed = _logical(family, n, qlens, ctxs, g, hkv, seed, stride)
    kc, vc, bt, poison = _page(ks, vs, ctxs, hkv, bs, (max_ctx or 0) // bs, seed)
    cu = torch.zeros(n + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(qlens), 0)
    q = torch.cat(qs).reshape(-1, hq * D).to(BF16)
    return Case(name=name, family=family, n=n, g=g, hq=hq, hkv=hkv, bs=bs, qlens=list(qlens), ctxs=list(ctxs),
                q=q, kc=kc, vc=vc, bt=bt, cu=cu, poison=poison, max_ctx=max_ctx or bt.shape[1] * bs,
                scale=LN2 / 16 if family == "staircase" else 1 / math.sqrt(D), witnesses=wit, stride=stride,
                closed=None if closed[0] is None else torch.cat(closed), fused=None, cs=None, q_scale=None,
                logical=(qs, ks, vs), _exp=None, _fs=None)


# ------------------------------------------------------------------------------------------------ fused decode
def _rot(x, cs, sign=1.0):
    """neox rotation of x [..., 128] by the table rows cs [..., 128] (cos | sin), float64; sign -1 undoes it.
    Also returns the magnitudes |a cos| + |b sin| of the two products of every element."""
    co, si = cs[..., :64], sign * cs[..., 64:]
    a, b = x[..., :64], x[..., 64:]
    y = torch.cat([a * co - b * si, b * co + a * si], -1)
    mag = torch.cat([(a * co).abs() + (b * si).abs(), (b * co).abs() + (a * si).abs()], -1)
    return y, mag


def add_fused(c, sk=2, tiles=4, padded=(), seed=0):
    """The decode case as the fused kernel gets it: fp32 split-K slabs, statistics tiles, the RoPE table and slots,
    built backwards (un-rotated, un-scaled) from the case's q rows and its last key, so that the prologue arrives at
    them again. Before the step the new token's row holds stale values: finite, as the engine's zeroed pool
    guarantees (the kernel loads that row for the masked keys past the context), and far from the real ones."""
    gen = _gen(seed + 104729)
    n, hq, hkv = c.n, c.hq, c.hkv
    qs, ks, vs = c.logical
    cs = ref.rope_cos_sin(4096, D, 500000.0)
    ssv = (torch.rand(n, generator=gen) + 0.5) * HID
    wt = torch.rand(tiles, generator=gen) + 0.5
    ssp = torch.zeros(tiles, SSP_LD)
    ssp[:, :n] = (wt / wt.sum())[:, None] * ssv[None, :]
    rn = _row_scale(ssp, n)
    tgt = torch.stack([torch.cat([qs[s][0], ks[s][-1], vs[s][-1]]) for s in range(n)])   # [n, hq + 2 hkv, D]
    table = cs.double()[torch.tensor(c.ctxs) - 1][:, None, :]
    pre = tgt.clone()
    pre[:, : hq + hkv] = _rot(tgt[:, : hq + hkv], table, -1.0)[0]
    pre = pre.reshape(n, -1) / rn[:, None]
    fr = torch.rand(sk, generator=gen) + 0.5
    slab = ((fr / fr.sum())[:, None, None] * pre[None]).float()
    real = torch.tensor([int(c.bt[i, (x - 1) // 16]) * 16 + (x - 1) % 16 for i, x in enumerate(c.ctxs)])
    slots = real.clone()
    slots[list(padded)] = -1
    kc0, vc0 = c.kc.clone(), c.vc.clone()
    kc0[real // 16, :, real % 16] = STALE_K
    vc0[real // 16, :, real % 16] = STALE_V
    c.fused = SimpleNamespace(slab=slab, ssp=ssp, cs=cs, real=real, slots=slots, kc0=kc0, vc0=vc0, sk=sk, tiles=tiles,
                              pos=torch.tensor(c.ctxs) - 1)
    c._exp = c._fs = None
    return c


def _row_scale(ssp, n):
    inv_n = float(torch.tensor(1.0) / torch.tensor(float(HID)))   # the launcher's fp32 1 / hidden
    return 1.0 / torch.sqrt(ssp.double()[:, :n].sum(0) * inv_n + float(torch.tensor(EPS)))


def fused_step(c):
    """float64 model of the fused decode prologue. q bf16 [n, hq D]; the caches the step attends to (every row's
    new token in place) and the caches it leaves (slot -1 wrote nothing); the new k / v before rounding with their
    fp32 error allowance."""
    if c._fs is not None:
        return c._fs
    f, n, hq, hkv = c.fused, c.n, c.hq, c.hkv
    x = (f.slab.double().sum(0) * _row_scale(f.ssp, n)[:, None]).reshape(n, hq + 2 * hkv, D)
    table = f.cs.double()[f.pos][:, None, :]
    rot, mag = _rot(x[:, : hq + hkv], table)
    k64, v64 = rot[:, hq:], x[:, hq + hkv:]
    q = bf(rot[:, :hq]).reshape(n, hq * D)

    def write(kc, vc, slots):
        ok = slots >= 0
        kc[slots[ok] // 16, :, slots[ok] % 16] = bf(k64[ok])
        vc[slots[ok] // 16, :, slots[ok] % 16] = bf(v64[ok])
        return kc, vc
    k_att, v_att = write(f.kc0.clone(), f.vc0.clone(), f.real)
    k_aft, v_aft = write(f.kc0.clone(), f.vc0.clone(), f.slots)
    kd, vd = 2.0 ** -20 * mag[:, hq:], 2.0 ** -20 * v64.abs()
    moves = (flip_move(rot[:, :hq], 2.0 ** -20 * mag[:, :hq]), flip_move(k64, kd), flip_move(v64, vd))
    c._fs = SimpleNamespace(q=q, k_att=k_att, v_att=v_att, k_after=k_aft, v_after=v_aft, k64=k64, v64=v64,
                            k_delta=kd, v_delta=vd, moves=moves)
    return c._fs


def rounds_to(y, x, delta):
    """True where bf16 y is a correct rounding of some value within delta of the float64 x."""
    big = torch.maximum(y.double().abs(), x.abs()).clamp_min(2.0 ** -126)
    half_ulp = torch.exp2(torch.floor(torch.log2(big)) - 8)
    return (y.double() - x).abs() <= half_ulp + delta


# ------------------------------------------------------------------------------------------------ prefill RoPE
def add_rope(c, q_scale=False, seed=0):
    c.cs = ref.rope_cos_sin(4096, D, 500000.0)
    if q_scale:
        c.q_scale = (torch.rand(c.q.shape[0], generator=_gen(seed + 15485863)) + 0.5).float()
    c._exp = None
    return c


def rope_q(c):
    """The prefill kernel's RoPE-on-load: q rows rotated at position ctx - qlen + i (clamped to the table), scaled
    by q_scale, rounded to bf16 once. Returns (q bf16 [T, hq D], the possible move of every element [T, hq, D])."""
    pos = torch.cat([torch.arange(ctx - ql, ctx) for ql, ctx in zip(c.qlens, c.ctxs)])
    table = c.cs.double()[pos.clamp_max(c.cs.shape[0] - 1)][:, None, :]
    y, mag = _rot(c.q.double().reshape(-1, c.hq, D), table)
    if c.q_scale is not None:
        y, mag = y * c.q_scale.double()[:, None, None], mag * c.q_scale.double()[:, None, None]
    return bf(y).reshape(-1, c.hq * D), flip_move(y, 2.0 ** -20 * mag)


# ------------------------------------------------------------------------------------------------ the GPU lists
BOUNDARY = [1, 15, 16, 17, 127, 128, 129, 255, 256, 257]
BATCH32 = [777, 2, 128, 129, 640, 641] + [3 + (97 * i) % 770 for i in range(26)]
# config -> g, hkv, contexts, static bound, padded rows of the fused variant. "multi" is 4 sequences x 8 kv heads: at
# a bound of 2,048 a 256-CU device still cuts it into one-chunk parts (512 tasks <= 2 x CUs), so "multi4k" repeats
# it at a bound of 4,096, where the parts are 4 chunks long.
DECODE_CONFIGS = {
    "b1x4": (1, 4, BOUNDARY, None, (0, 6)),
    "b2x4": (2, 4, BOUNDARY, None, (0, 6)),
    "b4x8": (4, 8, BOUNDARY, None, (0, 6)),
    "b8x1": (8, 1, BOUNDARY, None, (0, 6)),
    "few": (8, 1, [130, 1024, 1025, 2048], 2048, (0,)),
    "multi": (4, 8, [640, 1023, 1025, 2048], 2048, ()),
    "multi4k": (4, 8, [640, 1023, 1025, 2048], 4096, (2,)),
    "batch32": (4, 8, BATCH32, None, (1, 3)),
}
DECODE_CASES = [f"{fam}-{cfg}" for cfg in DECODE_CONFIGS for fam in FAMILIES]
# fused variants: (config, split-K slabs, statistics tiles); the default of the list above is (2, 4)
FUSED_VARIANTS = [("b1x4", 1, 130), ("b1x4", 3, 256), ("b4x8", 3, 4), ("b8x1", 4, 130)]
FUSED_CASES = [f"{c}+fused" for c in DECODE_CASES] + \
              [f"{fam}-{cfg}+fused-sk{sk}-t{t}" for cfg, sk, t in FUSED_VARIANTS for fam in ("flat", "random")]
TWO_LAUNCH_CTXS = [1, 64, 65, 300, 2049]
TWO_LAUNCH_CASES = [f"{fam}-2l-g{g}-bs{bs}" for fam in ("flat", "witness") for g in (4, 16) for bs in (16, 32)]
# (256, 391) puts the short list exactly on the launcher's max_q_len <= 256 threshold, (257, 257) one past it
PREFILL_PAIRS = [(1, 1), (37, 37), (129, 129), (128, 300), (64, 1000), (33, 161), (256, 391), (257, 257), (257, 700)]
PREFILL_KINDS = (("flat", ""), ("staircase", ""), ("witness", ""), ("random", "+cs"), ("random", "+cs+qs"))
PREFILL_CASES = [f"{fam}-pf-{size}-g{g}{fz}" for size in ("small", "large") for g in (1, 4, 8)
                 for fam, fz in PREFILL_KINDS]
ALL_CASES = DECODE_CASES + FUSED_CASES + TWO_LAUNCH_CASES + PREFILL_CASES


def _seed(name: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


@functools.lru_cache(maxsize=2)
def case(name: str) -> Case:
    """The named case of the lists above (the last two stay cached); tests must not write to its tensors."""
    base, _, fz = name.partition("+")
    fam, _, rest = base.partition("-")
    if rest.startswith("pf-"):
        _, size, g = rest.split("-")
        pairs = [p for p in PREFILL_PAIRS if size == "large" or p[0] <= 256]
        c = make_case(name, fam, [p[0] for p in pairs], [p[1] for p in pairs], int(g[1:]), 2, seed=_seed(base),
                      stride=1)
        c.max_q_len = max(c.qlens)
        if fz:
            add_rope(c, q_scale=fz.endswith("qs"), seed=_seed(name))
        return c
    if rest.startswith("2l-"):
        _, g, bs = rest.split("-")
        return make_case(name, fam, [1] * 5, TWO_LAUNCH_CTXS, int(g[1:]), 2, bs=int(bs[2:]), seed=_seed(base))
    g, hkv, ctxs, max_ctx, padded = DECODE_CONFIGS[rest]
    c = make_case(name, fam, [1] * len(ctxs), ctxs, g, hkv, max_ctx=max_ctx, seed=_seed(base))
    if fz:
        parts = fz.split("-")
        sk, tiles = (int(parts[1][2:]), int(parts[2][1:])) if len(parts) == 3 else (2, 4)
        add_fused(c, sk=sk, tiles=tiles, padded=padded, seed=_seed(name))
    return c
