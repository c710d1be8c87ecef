"""The per-token row kernels (csrc/kernels/norm_act.hip, csrc/kernels/rope_cache.hip) element by element against the
float64 oracles of tests/rowwise_reference.py on its case lists, through the public wrappers of src/ops: RMSNorm
(plain, fused add, slab) at the bottom, one chunk past the bottom and the top of every chunks-per-thread count, the row
scale likewise, the three sums of squares, SiLU * up at every chunks-per-lane count with the gate ladder across the
fast exp's overflow, RoPE + KV write at both head sizes from bf16 rows and from fp32 slabs, and the block movers.
test_rowwise_reference_cpu.py proves for every case used here that a single wrong term changes the expectation.

Bit-exact outputs (residuals after an add, copies, sums of squares and RoPE on the exact families) are compared
with torch.equal; rounded outputs have to be one of the bracket's bf16 values (the oracle's rounding wherever the
derived error cannot cross a rounding boundary); fp32 statistics stay within their summation bound. Every input is
a view of a NaN-filled buffer, every output a view of a sentinel-filled one that must be bit-identical outside the
specified region; in-place ops run once on fresh copies. A launch that the binding has to refuse must raise. Each
test prints its worst err / tol."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from tests import rowwise_reference as rr  # noqa: E402

NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), "HIP extension must be built for GPU tests"
    return torch.device("cuda:0")


def _place(t, dev, strided=False, fill=NAN):
    """t (>= 1-D, rows of its last dim) as a view of a buffer filled with `fill`: guard rows before and after, and with
    `strided` (2-D only) a longer row stride with guard columns."""
    flat = t.reshape(-1, t.shape[-1])
    rows, cols = flat.shape
    buf = torch.full((rows + 2, cols + (8 if strided else 0)), fill, dtype=t.dtype, device=dev)
    v = buf[1:1 + rows, :cols]
    v.copy_(flat)
    assert strided == (not v.is_contiguous()) or rows == 1
    return v if strided else v.view(t.shape)


def _vec(t, dev, fill=NAN):
    """A 1-D tensor as a contiguous slice of a longer one."""
    buf = torch.full((t.numel() + 16,), fill, dtype=t.dtype, device=dev)
    v = buf[8:8 + t.numel()]
    v.copy_(t)
    return v


class _Out:
    """An output [rows, cols] as a view of a sentinel-filled buffer (guard rows, with `strided` guard columns);
    untouched() is true when everything outside the view still holds the sentinel."""

    def __init__(self, rows, cols, dtype, dev, strided=False, value=rr.SENT):
        self.value = value
        self.buf = torch.full((rows + 2, cols + (8 if strided else 0)), value, dtype=dtype, device=dev)
        self.t = self.buf[1:1 + rows, :cols]

    def untouched(self):
        c = self.buf.clone()
        c[1:1 + self.t.shape[0], : self.t.shape[1]] = self.value
        return rr.same_bits(c, torch.full_like(c, self.value))


def _bracketed(label, y, o, s, c):
    j = rr.judge(y.cpu(), o, s, c)
    bad = ~j.ok
    if bool(bad.any()):
        k = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.numel()} elements outside the bracket; first at flat "
                             f"index {k}: got {float(y.cpu().double().flatten()[k]):.9g}, oracle "
                             f"{float(o.flatten()[k]):.9g}, allowed {float(j.lo.flatten()[k]):.9g} / "
                             f"{float(j.hi.flatten()[k]):.9g}; worst err/tol {j.ratio:.3f}")
    return j.ratio


def _equal(label, got, want):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, label
    if not rr.same_bits(got, want):
        d = rr.bits(got) != rr.bits(want)
        k = int(d.flatten().nonzero()[0])
        raise AssertionError(f"{label}: {int(d.sum())} of {d.numel()} elements differ; first at flat index {k}: got "
                             f"{float(got.flatten()[k]):.9g}, want {float(want.flatten()[k]):.9g}")


# ---------------------------------------------------------------------------------------------- norms

@pytest.mark.parametrize("name", rr.NORM_CASES)
def test_rms_norm_forms(dev, name):
    c = rr.ROW_CASES[name]
    i = rr.row_inputs(name)
    w = _vec(i.w, dev)
    worst = 0.0
    for form in ("plain", "add", "slab"):
        e = rr.norm_expected(name, form)
        out = _Out(c.rows, c.hidden, torch.bfloat16, dev, c.strided)
        res = _Out(c.rows, c.hidden, torch.bfloat16, dev)          # the binding wants a contiguous residual
        res.t.copy_(i.resid)
        if form == "plain":
            ops.rms_norm(_place(i.resid, dev, c.strided), w, rr.EPS, out=out.t)
        elif form == "add":
            ops.fused_add_rms_norm(_place(i.x, dev, c.strided), res.t, w, rr.EPS, out=out.t)
        else:
            ops.fused_add_rms_norm_slab(_place(i.slab, dev), res.t, w, rr.EPS, out=out.t)
        torch.cuda.synchronize()
        tag = f"{name} {form}"
        assert out.untouched() and res.untouched(), f"{tag}: guard rows or columns written"
        _equal(f"{tag} residual", res.t, i.resid if form == "plain" else e.h)
        worst = max(worst, _bracketed(tag, out.t, e.o, e.s, e.c))
    print(f"{name}: c = {rr.c_norm(c.hidden):.0f}, worst err/tol {worst:.3f}")


def test_norms_refuse_wide_rows(dev):
    h = rr.NORM_REFUSED_HIDDEN
    x = torch.zeros(1, h, dtype=torch.bfloat16, device=dev)
    w = torch.ones(h, dtype=torch.bfloat16, device=dev)
    out = torch.empty_like(x)
    with pytest.raises(RuntimeError):
        ops.rms_norm(x, w, rr.EPS, out=out)
    with pytest.raises(RuntimeError):
        ops.fused_add_rms_norm(x, x.clone(), w, rr.EPS, out=out)
    with pytest.raises(RuntimeError):
        ops.fused_add_rms_norm_slab(torch.zeros(1, 1, h, device=dev), x.clone(), w, rr.EPS, out=out)
    h = rr.RS_REFUSED_HIDDEN
    x = torch.zeros(1, h, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError):
        ops.rms_row_scale(x, None, rr.EPS)
    with pytest.raises(RuntimeError):
        ops.rms_row_scale(x, x.clone(), rr.EPS)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", rr.RS_CASES)
def test_rms_row_scale(dev, name):
    c = rr.ROW_CASES[name]
    i = rr.row_inputs(name)
    worst = 0.0
    for form in ("rs_plain", "rs_add"):
        e = rr.norm_expected(name, form)
        res = _Out(c.rows, c.hidden, torch.bfloat16, dev, c.strided)
        res.t.copy_(i.resid)
        rs = _Out(1, c.rows, torch.float32, dev, True)
        x = _place(i.x, dev, not c.strided) if form == "rs_add" else None
        ops.rms_row_scale(res.t, x, rr.EPS, out=rs.t[0])
        torch.cuda.synchronize()
        tag = f"{name} {form}"
        assert res.untouched() and rs.untouched(), f"{tag}: guards written"
        _equal(f"{tag} residual", res.t, e.h)
        got = rs.t[0].cpu().double()
        assert bool(torch.isfinite(got).all()), tag
        r = ((got - e.rs).abs() / e.rs_tol).max()
        assert float(r) <= 1, f"{tag}: rs {got.tolist()} vs {e.rs.tolist()}, err/tol {float(r):.3f}"
        worst = max(worst, float(r))
    print(f"{name}: worst err/tol {worst:.3f}")


@pytest.mark.parametrize("name", rr.SUMSQ_CASES)
def test_sums_of_squares(dev, name):
    c = rr.ROW_CASES[name]
    i = rr.row_inputs(name)
    worst = 0.0
    for op in ("row", "embed", "add"):
        e = rr.sumsq_expected(name, op)
        ssp = _Out(1, rr.SSP_LD, torch.float32, dev)
        tag = f"{name} {op}"
        if op == "row":
            ops.row_sumsq(_place(i.resid, dev, c.strided), out=ssp.t)
        elif op == "embed":
            h = _Out(c.rows, c.hidden, torch.bfloat16, dev)
            ops.embed_sumsq(_vec(i.ids, dev, 0), _place(i.table, dev), ssp.t, out=h.t)
        else:
            h = _Out(c.rows, c.hidden, torch.bfloat16, dev, c.strided)
            h.t.copy_(i.resid)
            ops.residual_add_sumsq(h.t, _place(i.x, dev, not c.strided), ssp.t)
        torch.cuda.synchronize()
        if op != "row":
            assert h.untouched(), f"{tag}: guards written"
            _equal(f"{tag} rows", h.t, e.h)
        assert ssp.untouched(), f"{tag}: guards written"
        _equal(f"{tag} ssp beyond the rows", ssp.t[0, c.rows:], torch.full((rr.SSP_LD - c.rows,), rr.SENT))
        got = ssp.t[0, : c.rows].cpu()
        if c.exact_stats:
            _equal(f"{tag} ss", got, e.ss.float())
        else:
            r = ((got.double() - e.ss).abs() / e.tol).max()
            assert float(r) <= 1, f"{tag}: err/tol {float(r):.3f}"
            worst = max(worst, float(r))
    print(f"{name}: " + ("exact" if c.exact_stats else f"worst err/tol {worst:.3f}"))


def test_sums_of_squares_refuse_129_rows(dev):
    n = rr.SUMSQ_REFUSED_ROWS
    x = torch.zeros(n, 64, dtype=torch.bfloat16, device=dev)
    ssp = torch.zeros(1, 256, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError):
        ops.row_sumsq(x, out=ssp)
    with pytest.raises(RuntimeError):
        ops.residual_add_sumsq(x.clone(), x, ssp)
    with pytest.raises(RuntimeError):
        ops.embed_sumsq(torch.zeros(n, dtype=torch.long, device=dev), x, ssp, out=torch.empty_like(x))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- SiLU * up

def _silu_report(name, i, e, y):
    """Which elements of the ladder are off, by band of z."""
    j = rr.judge(y.cpu(), e.o, e.s, e.c)
    bad = ~j.ok
    z = e.z
    bands = (("z < -88.72", z < -88.72), ("-88.72 <= z <= -87.34", (z >= -88.72) & (z <= -87.34)),
             ("z > -87.34", z > -87.34))
    txt = "; ".join(f"{lab}: {int((bad & m).sum())} of {int(m.sum())}" for lab, m in bands)
    tol = rr.half_ulp_bf16(e.o) + e.c * rr.U23 * e.s
    r = ((y.cpu().double() - e.o).abs() / tol)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    r = torch.where(bad, r, torch.zeros_like(r))
    k = int(r.argmax())
    return (f"{name}: {int(bad.sum())} elements outside the bracket ({txt}); worst err/tol {float(r.max()):.3g} at "
            f"z = {float(z.flatten()[k]):.6g}, up = {float((i.up.double().flatten()[k])):.6g}: got "
            f"{float(y.cpu().double().flatten()[k]):.9g}, oracle {float(e.o.flatten()[k]):.9g}")


@pytest.mark.parametrize("name", list(rr.SILU_CASES))
def test_silu_and_mul(dev, name):
    c = rr.SILU_CASES[name]
    i = rr.silu_inputs(name)
    e = rr.silu_expected(name)
    rows, inter = rr.SILU_ROWS, c.inter
    r = _vec(i.r, dev) if i.r is not None else None
    # gate and up as column blocks of one NaN-filled buffer with guard columns, out as a column block of a sentinel one
    buf = torch.full((rows + 2, 2 * inter + 24), NAN, dtype=torch.bfloat16, device=dev)
    gate, up = buf[1:1 + rows, 8:8 + inter], buf[1:1 + rows, 16 + inter:16 + 2 * inter]
    gate.copy_(i.gate)
    up.copy_(i.up)
    ob = torch.full((rows + 2, inter + 16), rr.SENT, dtype=torch.bfloat16, device=dev)
    out = ob[1:1 + rows, 8:8 + inter]
    ops.silu_and_mul_views(gate, up, out, row_scale=r, per=c.per)
    torch.cuda.synchronize()
    chk = ob.clone()
    chk[1:1 + rows, 8:8 + inter] = rr.SENT
    assert rr.same_bits(chk, torch.full_like(chk, rr.SENT)), f"{name}: guard rows or columns written"
    runs = [out]
    if c.per == 0:   # the contiguous entry point makes the same choice
        x = _place(torch.cat([i.gate, i.up], 1), dev)
        o2 = _Out(rows, inter, torch.bfloat16, dev)
        ops.silu_and_mul(x, out=o2.t, row_scale=r)
        torch.cuda.synchronize()
        assert o2.untouched(), f"{name}: guard rows written"
        runs.append(o2.t)
    worst = 0.0
    for y in runs:
        j = rr.judge(y.cpu(), e.o, e.s, e.c)
        assert bool(j.ok.all()), _silu_report(name, i, e, y)
        worst = max(worst, j.ratio)
    print(f"{name}: worst err/tol {worst:.3f}, undecided {j.undecided:.4f}")


def test_silu_refuses_bad_shapes(dev):
    g = torch.zeros(2, 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError):
        ops.silu_and_mul_views(g, g.clone(), torch.empty_like(g), per=9)
    with pytest.raises(RuntimeError):
        ops.silu_and_mul_views(g[:, :60], g.clone()[:, :60], torch.empty_like(g)[:, :60])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- RoPE + KV write

def _caches(c, dev):
    shape = (rr.ROPE_BLOCKS + 2, c.hkv, c.block_size, c.d)
    kb = torch.full(shape, rr.SENT, dtype=torch.bfloat16, device=dev)
    vb = torch.full(shape, rr.SENT, dtype=torch.bfloat16, device=dev)
    return kb, vb


def _judge_caches(name, c, e, kb, vb):
    """K under the bracket (exact family: equal), V equal or under the one-multiply bracket; sentinels elsewhere."""
    worst = 0.0
    k, v = kb[1:-1].cpu(), vb[1:-1].cpu()
    sent = torch.full_like(k, rr.SENT)
    for lab, t, b in (("K", k, kb), ("V", v, vb)):
        _equal(f"{name} {lab} cache outside the written slots", torch.where(e.written, sent, t), sent)
        _equal(f"{name} {lab} guard blocks", b[[0, -1]], torch.full_like(b[[0, -1]].cpu(), rr.SENT))
    w = e.written
    if c.family == "exact":
        assert torch.equal(k[w].double(), e.k[w]), f"{name}: K differs from the exact rotation"
    else:
        worst = _bracketed(f"{name} K", k[w], e.k[w], e.ks[w], e.c)
    if e.v_exact:
        assert torch.equal(v[w].double(), rr.rne_bf16(e.v[w])), f"{name}: V differs"
    else:
        worst = max(worst, _bracketed(f"{name} V", v[w], e.v[w], e.v[w].abs(), rr.C_V))
    return worst


@pytest.mark.parametrize("name", rr.ROPE_CASES)
def test_rope_and_cache(dev, name):
    c = rr.ROPE_CASES_BY_NAME[name]
    i = rr.rope_inputs(name)
    e = rr.rope_expected(name)
    t, qw = rr.ROPE_TOKENS, c.hq * c.d
    pad = 64 if c.wide else 0
    buf = torch.full((t + 2, c.width + pad), NAN, dtype=torch.bfloat16, device=dev)
    qkv = buf[1:1 + t] if c.wide else buf[1:1 + t, : c.width]
    qkv[:, : c.width] = i.qkv.to(dev)
    before = buf.clone()
    kb, vb = _caches(c, dev)
    r = _vec(i.r, dev) if i.r is not None else None
    ops.rope_and_cache(qkv, _vec(i.positions, dev, 0), _place(i.table, dev), _vec(i.slots, dev, 0), kb[1:-1], vb[1:-1],
                       c.hq, c.hkv, c.d, rot_q=c.rot_q, row_scale=r)
    torch.cuda.synchronize()
    after = buf.cpu()
    keep = before.cpu()
    if c.rot_q:
        keep[1:1 + t, :qw] = after[1:1 + t, :qw]
    _equal(f"{name}: qkv outside the rotated q columns", after, keep)   # k, v, the wide columns, guard rows; q if kept
    worst = 0.0
    if c.rot_q:
        q = after[1:1 + t, :qw].view(t, c.hq, c.d)
        if c.family == "exact":
            assert torch.equal(q.double(), e.q), f"{name}: q differs from the exact rotation"
        else:
            worst = _bracketed(f"{name} q", q, e.q, e.qs, e.c)
    worst = max(worst, _judge_caches(name, c, e, kb, vb))
    print(f"{name}: " + ("exact" if c.family == "exact" else f"worst err/tol {worst:.3f}"))


@pytest.mark.parametrize("name", rr.ROPE_SLAB_CASES)
def test_rope_and_cache_slab(dev, name):
    c = rr.ROPE_CASES_BY_NAME[name]
    i = rr.rope_inputs(name)
    e = rr.rope_expected(name)
    t, qw = rr.ROPE_TOKENS, c.hq * c.d
    kb, vb = _caches(c, dev)
    qo = _Out(t, qw, torch.bfloat16, dev)
    ops.rope_and_cache_slab(_place(i.slab, dev), _vec(i.positions, dev, 0), _place(i.table, dev),
                            _vec(i.slots, dev, 0), kb[1:-1], vb[1:-1], c.hq, c.hkv, c.d, q_out=qo.t)
    torch.cuda.synchronize()
    assert qo.untouched(), f"{name}: q_out guard rows written"
    q = qo.t.cpu().view(t, c.hq, c.d)
    worst = 0.0
    if c.family == "exact":
        assert torch.equal(q.double(), e.q), f"{name}: q differs from the exact rotation"
    else:
        worst = _bracketed(f"{name} q", q, e.q, e.qs, e.c)
    worst = max(worst, _judge_caches(name, c, e, kb, vb))
    print(f"{name}: " + ("exact" if c.family == "exact" else f"worst err/tol {worst:.3f}"))


def test_rope_refuses_strided_or_host_index_tensors(dev):
    """positions, slot_mapping and cos_sin are read through raw pointers: a strided view or a host tensor must raise
    before anything is launched."""
    c = rr.ROPE_CASES_BY_NAME["rope-d64-h1x1-b16-exact-q"]
    i = rr.rope_inputs(c.name)
    t = rr.ROPE_TOKENS
    good = dict(pos=i.positions.to(dev), slots=i.slots.to(dev), table=i.table.to(dev))
    strided = dict(pos=torch.zeros(2 * t, dtype=torch.long, device=dev)[::2],
                   slots=torch.full((2 * t,), -1, dtype=torch.long, device=dev)[::2],
                   table=torch.zeros(rr.MAX_POS, 2 * c.d, device=dev)[:, : c.d])
    host = dict(pos=i.positions, slots=i.slots, table=i.table)
    for bad in (strided, host):
        for key in ("pos", "slots", "table"):
            a = dict(good, **{key: bad[key]})
            kb, vb = _caches(c, dev)
            with pytest.raises(RuntimeError):
                ops.rope_and_cache(i.qkv.to(dev), a["pos"], a["table"], a["slots"], kb[1:-1], vb[1:-1], c.hq, c.hkv, c.d)
            with pytest.raises(RuntimeError):
                ops.rope_and_cache_slab(i.qkv.float().to(dev)[None], a["pos"], a["table"], a["slots"], kb[1:-1], vb[1:-1],
                                        c.hq, c.hkv, c.d)
            assert rr.same_bits(kb, torch.full_like(kb, rr.SENT)) and rr.same_bits(vb, torch.full_like(vb, rr.SENT))
    with pytest.raises(RuntimeError):   # no kernel for this head size
        kb = torch.zeros(2, 1, 16, 32, dtype=torch.bfloat16, device=dev)
        ops.rope_and_cache(torch.zeros(1, 96, dtype=torch.bfloat16, device=dev), good["pos"], torch.zeros(4, 32, device=dev),
                           good["slots"], kb, kb.clone(), 1, 1, 32)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- block movers

def _pool(name, dev):
    """The case's pool as a contiguous range of a sentinel-filled buffer."""
    p = rr.mover_pool(name)
    buf = torch.full((p.numel() + 64,), rr.SENT, dtype=torch.bfloat16, device=dev)
    v = buf[32:32 + p.numel()].view(p.shape)
    v.copy_(p)
    return p, buf, v


def _guards_ok(buf):
    g = torch.cat([buf[:32], buf[-32:]])
    return rr.same_bits(g, torch.full_like(g, rr.SENT))


@pytest.mark.parametrize("name", list(rr.MOVER_CASES))
def test_block_movers(dev, name):
    c = rr.MOVER_CASES[name]
    p, buf, pool = _pool(name, dev)
    ops.copy_blocks(pool, torch.tensor(rr.COPY_PAIRS, dtype=torch.long, device=dev))
    torch.cuda.synchronize()
    _equal(f"{name} copy_blocks", pool, rr.copied(p, rr.COPY_PAIRS))
    assert _guards_ok(buf), f"{name}: copy_blocks wrote outside the pool"
    for ids in rr.MOVE_IDS:
        p, buf, pool = _pool(name, dev)
        idt = _vec(torch.tensor(ids), dev, 0)
        n = len(ids)
        stage = _Out(n, c.planes * c.slab, torch.bfloat16, dev)
        ops.gather_blocks(pool, idt, buf=stage.t.view(n, c.planes, c.slab))
        torch.cuda.synchronize()
        want = rr.gathered(p, ids)
        _equal(f"{name} gather_blocks {ids}", stage.t.view(n, c.planes, c.slab), want)
        assert stage.untouched() and _guards_ok(buf), f"{name}: gather_blocks wrote outside its buffer"
        _equal(f"{name} gather_blocks left the pool", pool, p)
        # scatter into a sentinel-filled pool: the listed blocks arrive, the others keep the sentinel
        tb = torch.full_like(buf, rr.SENT)
        target = tb[32:32 + p.numel()].view(p.shape)
        ops.scatter_blocks(target, idt, stage.t.view(n, c.planes, c.slab))
        torch.cuda.synchronize()
        _equal(f"{name} scatter_blocks {ids}", target, rr.scattered(torch.full_like(p, rr.SENT), ids, want))
        assert _guards_ok(tb), f"{name}: scatter_blocks wrote outside the pool"
        # the row form: planes [plane0, plane0 + nplanes) of each block into its own packet row
        for plane0, nplanes in {(0, c.planes), (c.planes - 1, 1), (min(1, c.planes - 1), max(1, c.planes - 2))}:
            rows = _Out(n, c.planes * c.slab, torch.bfloat16, dev)
            order = list(reversed(range(n)))                        # block j of the list lands in row order[j]
            dst = torch.tensor([rows.t[k].data_ptr() for k in order], dtype=torch.long, device=dev)
            ops.gather_blocks_rows(pool, idt, dst, plane0, nplanes)
            torch.cuda.synchronize()
            exp = torch.full((n, c.planes, c.slab), rr.SENT, dtype=torch.bfloat16)
            for j, k in enumerate(order):
                exp[k, plane0:plane0 + nplanes] = want[j, plane0:plane0 + nplanes]
            _equal(f"{name} gather_blocks_rows {ids} planes {plane0}+{nplanes}", rows.t.view(n, c.planes, c.slab), exp)
            assert rows.untouched(), f"{name}: gather_blocks_rows wrote outside its rows"
    print(f"{name}: exact")
