"""The mixture-of-experts kernels (csrc/kernels/moe.hip: topk_softmax, moe_route<8|16>, moe_align, moe_gather,
moe_combine, moe_combine_residual) against the float64 oracles of tests/moe_reference.py on its case lists, through
the wrappers of src/ops and, where an output has to lie in a sentinel-filled buffer or a refusal lives in the binding,
through ops._kern(). test_moe_reference_cpu.py proves for every case used here which wrong kernels it would notice.

Expert ids are compared with torch.equal, slot order included, on every row without a NaN (there: K distinct ids in
range); routing weights within the derived fp32 tolerance; combine outputs and sums of squares of the exact family bit
for bit, of the random family inside the bracket; align by its contract. Every input is a view of a poisoned buffer
(NaN; for index arrays a value whose use would show), every output a view of a sentinel-filled one that must be
bit-identical outside its region. Every launch runs twice and must repeat itself bit for bit (align: offsets; sorted
and pos must satisfy the contract both times); in-place ops run once each on fresh copies. A launch that has to be
refused must raise. Each test prints its worst err / tol."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from tests import moe_reference as mr  # noqa: E402
from tests import rowwise_reference as rr  # noqa: E402

NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), "HIP extension must be built for GPU tests"
    return torch.device("cuda:0")


def _place(t, dev, strided=False, fill=NAN):
    """t [rows, cols] as a view of a buffer filled with `fill`: guard rows before and after, and with `strided` a
    longer row stride with guard columns."""
    rows, cols = t.shape
    buf = torch.full((rows + 2, cols + (8 if strided else 0)), fill, dtype=t.dtype, device=dev)
    v = buf[1:1 + rows, :cols]
    v.copy_(t)
    assert strided == (not v.is_contiguous()) or rows == 1
    return v


def _vec(t, dev, fill):
    """A 1-D tensor as a contiguous slice of a longer one."""
    buf = torch.full((t.numel() + 16,), fill, dtype=t.dtype, device=dev)
    v = buf[8:8 + t.numel()]
    v.copy_(t)
    return v


class _Out:
    """An output [rows, cols] as a view of a sentinel-filled buffer (guard rows, with `strided` guard columns);
    untouched() is true when everything outside the view still holds the sentinel."""

    def __init__(self, rows, cols, dtype, dev, strided=False):
        self.value = mr.SENT_I if dtype == torch.int32 else mr.SENT
        self.buf = torch.full((rows + 2, cols + (8 if strided else 0)), self.value, dtype=dtype, device=dev)
        self.t = self.buf[1:1 + rows, :cols]

    def untouched(self):
        c = self.buf.clone()
        c[1:1 + self.t.shape[0], : self.t.shape[1]] = self.value
        return rr.same_bits(c, torch.full_like(c, self.value))


class _OutVec:
    """A 1-D int32 output of which only the first `n` entries may be written: .t is the slice handed to the kernel
    (longer than n), untouched() checks the guards before it and everything from n on."""

    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((n + 24,), mr.SENT_I, dtype=torch.int32, device=dev)
        self.t = self.buf[8:]

    def untouched(self):
        c = self.buf.clone()
        c[8:8 + self.n] = mr.SENT_I
        return bool((c == mr.SENT_I).all())


def _equal(label, got, want):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, label
    if not rr.same_bits(got, want):
        d = rr.bits(got) != rr.bits(want)
        k = int(d.flatten().nonzero()[0])
        raise AssertionError(f"{label}: {int(d.sum())} of {d.numel()} elements differ; first at flat index {k}: got "
                             f"{float(got.flatten()[k]):.9g}, want {float(want.flatten()[k]):.9g}")


def _routing_runs(label, runs, e, num_experts):
    """runs: (ids, w) of repeated launches: all bit-identical, the first judged against the oracle."""
    ids0, w0 = runs[0]
    for ids, w in runs[1:]:
        assert rr.same_bits(ids.contiguous(), ids0.contiguous()) and rr.same_bits(w.contiguous(), w0.contiguous()), \
            f"{label}: a repeated launch gives other bits"
    j = mr.judge_routing(ids0, w0, e, num_experts)
    assert not j.errs, f"{label}: " + "; ".join(j.errs)
    return j.ratio


# ---------------------------------------------------------------------------------------------- topk_softmax

@pytest.mark.parametrize("name", [c.name for c in mr.TOPK_ALL])
def test_topk_softmax(dev, name):
    c = mr.TOPK_CASES[name]
    e = mr.topk_expected(name)
    g = _place(mr.topk_inputs(name), dev)
    runs = [ops.topk_softmax(g, c.k, c.renorm) for _ in range(2)]
    w, ids = _Out(c.t, c.k, torch.float32, dev), _Out(c.t, c.k, torch.int32, dev)
    ops._kern().topk_softmax(w.t, ids.t, g, c.renorm)
    torch.cuda.synchronize()
    assert w.untouched() and ids.untouched(), f"{name}: guard rows written"
    _equal(f"{name}: the logits", g, mr.topk_inputs(name))
    ratio = _routing_runs(name, [(r[1], r[0]) for r in runs] + [(ids.t, w.t)], e, c.e)
    print(f"{name}: worst err/tol {ratio:.3f}")


# ---------------------------------------------------------------------------------------------- moe_route

@pytest.mark.parametrize("name", mr.ROUTE_FUSED_CASES)
def test_moe_route_fused(dev, name):
    i = mr.route_inputs(name)
    c = i.c
    e = mr.route_expected(name)
    x, wg = _place(i.x, dev, c.strided), _place(i.wg, dev)
    runs = [ops.moe_route(x, wg, c.k, c.renorm) for _ in range(2)]
    w, ids = _Out(c.t, c.k, torch.float32, dev), _Out(c.t, c.k, torch.int32, dev)
    ops._kern().moe_route(w.t, ids.t, x, wg, c.renorm)        # the binding has no other path than the fused kernel
    torch.cuda.synchronize()
    assert w.untouched() and ids.untouched(), f"{name}: guard rows written"
    _equal(f"{name}: x", x, i.x)
    ratio = _routing_runs(name, [(r[1], r[0]) for r in runs] + [(ids.t, w.t)], e, c.e)
    print(f"{name}: worst err/tol {ratio:.3f}")


def test_moe_route_fallback_agrees_with_the_fused_oracle(dev):
    """T = 257: ops.moe_route takes the router GEMM + topk_softmax. On the exact family the GEMM's bf16 logits are
    the oracle's, so ids and weights have to be the ones the fused kernel is held to."""
    name = mr.ROUTE_FALLBACK.name
    i = mr.route_inputs(name)
    c = i.c
    assert c.t > ops.MOE_ROUTE_MAX_T
    e = mr.route_expected(name)
    x, wg = _place(i.x, dev), _place(i.wg, dev)
    logits = torch.nn.functional.linear(x, wg)
    _equal(f"{name}: the GEMM's logits", logits.double(), mr.route_logits(i.x, i.wg))
    runs = [ops.moe_route(x, wg, c.k, c.renorm) for _ in range(2)]
    torch.cuda.synchronize()
    ratio = _routing_runs(name, [(r[1], r[0]) for r in runs], e, c.e)
    print(f"{name}: worst err/tol {ratio:.3f}")


# ---------------------------------------------------------------------------------------------- moe_align

@pytest.mark.parametrize("name", [c.name for c in mr.ALIGN_ALL])
def test_moe_align(dev, name):
    c = mr.ALIGN_CASES[name]
    ids_cpu = mr.align_ids(name)
    ids = _vec(ids_cpu, dev, c.e)           # a guard entry read as an id would count past the last expert
    offs = []
    for _ in range(2):
        off, srt, pos = _OutVec(c.e + 1, dev), _OutVec(c.n, dev), _OutVec(c.n, dev)
        ops._kern().moe_align(off.t, srt.t, pos.t, ids, c.e)
        torch.cuda.synchronize()
        assert off.untouched() and srt.untouched() and pos.untouched(), f"{name}: written outside the outputs"
        errs = mr.check_align(off.t[: c.e + 1], srt.t[: c.n], pos.t[: c.n], ids_cpu, c.e)
        assert not errs, f"{name}: " + "; ".join(errs)
        offs.append(off.t[: c.e + 1].clone())
    assert torch.equal(offs[0], offs[1]), f"{name}: a repeated launch gives other offsets"
    off, srt, pos = ops.moe_align(ids, c.e)
    torch.cuda.synchronize()
    assert off.dtype == srt.dtype == pos.dtype == torch.int32 and off.numel() == c.e + 1 and srt.numel() == c.n
    errs = mr.check_align(off, srt, pos, ids_cpu, c.e)
    assert not errs, f"{name} (wrapper): " + "; ".join(errs)
    _equal(f"{name}: ids", ids, ids_cpu)


# ---------------------------------------------------------------------------------------------- moe_gather

@pytest.mark.parametrize("name", [c.name for c in mr.GATHER_ALL])
def test_moe_gather(dev, name):
    i = mr.gather_inputs(name)
    c = i.c
    n = mr.GATHER_T * c.k
    if c.source == "align":
        srt_cpu = ops.moe_align(i.ids.to(dev), mr.GATHER_E)[1].cpu()
        assert torch.equal(srt_cpu.long().sort().values, torch.arange(n))
    else:
        srt_cpu = i.sorted
    srt = _vec(srt_cpu, dev, 0)
    x = _place(i.x, dev)
    want = mr.gathered(i.x, srt_cpu, c.k)
    outs = []
    for _ in range(2):
        xs = _Out(n, c.h, torch.bfloat16, dev)
        ops._kern().moe_gather(xs.t, x, srt, c.k)
        torch.cuda.synchronize()
        assert xs.untouched(), f"{name}: guard rows written"
        _equal(name, xs.t, want)
        outs.append(xs.t)
    assert rr.same_bits(outs[0], outs[1])
    _equal(f"{name}: x", x, i.x)


# ---------------------------------------------------------------------------------------------- combine

def _combine_args(i, dev):
    return _place(i.ys, dev), _vec(i.pos, dev, 0), _place(i.w, dev)


@pytest.mark.parametrize("name", [c.name for c in mr.COMBINE_ALL])
def test_moe_combine(dev, name):
    i = mr.combine_inputs(name)
    c = i.c
    e = mr.combine_expected(name, False)
    ys, pos, w = _combine_args(i, dev)
    outs = []
    for _ in range(2):
        out = _Out(c.t, c.h, torch.bfloat16, dev)
        ops._kern().moe_combine(out.t, ys, pos, w)
        torch.cuda.synchronize()
        assert out.untouched(), f"{name}: guard rows written"
        outs.append(out.t)
    assert rr.same_bits(outs[0], outs[1]), f"{name}: a repeated launch gives other bits"
    ratio = _judge_rows(name, outs[0], e)
    print(f"{name}: " + ("exact" if e.exact else f"worst err/tol {ratio:.3f}"))


def _judge_rows(label, got, e):
    if e.exact:
        _equal(label, got, e.h.to(torch.bfloat16))
        return 0.0
    j = rr.judge(got.cpu(), e.o, e.s, e.c)
    assert bool(j.ok.all()), f"{label}: {int((~j.ok).sum())} of {j.ok.numel()} elements outside the bracket, worst " \
                             f"err/tol {j.ratio:.3f}"
    return j.ratio


@pytest.mark.parametrize("name", [c.name for c in mr.COMBINE_ALL])
def test_moe_combine_residual(dev, name):
    i = mr.combine_inputs(name)
    c = i.c
    e = mr.combine_expected(name, True)
    ys, pos, w = _combine_args(i, dev)
    runs = []
    for _ in range(2):          # in place: each run on a fresh copy of the residual
        res = _Out(c.t, c.h, torch.bfloat16, dev, c.strided)
        res.t.copy_(i.resid)
        ssp = _Out(1, mr.SSP_LD, torch.float32, dev)
        ops._kern().moe_combine_residual(ssp.t, res.t, ys, pos, w)
        torch.cuda.synchronize()
        assert res.untouched() and ssp.untouched(), f"{name}: guard rows or columns written"
        _equal(f"{name}: ssp beyond the rows", ssp.t[0, c.t:], torch.full((mr.SSP_LD - c.t,), mr.SENT))
        runs.append((res.t, ssp.t[0, : c.t]))
    assert rr.same_bits(runs[0][0].contiguous(), runs[1][0].contiguous()) and rr.same_bits(runs[0][1], runs[1][1]), \
        f"{name}: a repeated launch gives other bits"
    got, ss = runs[0]
    ratio = _judge_rows(name, got, e)
    if e.exact:
        _equal(f"{name}: ssp", ss, e.ss.float())
        ss_ratio = 0.0
    else:       # the statistics of the rows as written (which the bracket has just judged)
        want = got.cpu().double().pow(2).sum(-1)
        r = (ss.cpu().double() - want).abs() / rr.sumsq_tol(want, c.h)
        ss_ratio = float(r.max())
        assert ss_ratio <= 1, f"{name}: ssp err/tol {ss_ratio:.3f}"
    _equal(f"{name}: ys", ys, i.ys)
    print(f"{name}: " + ("exact" if e.exact else f"worst err/tol {ratio:.3f}, ssp err/tol {ss_ratio:.3f}"))


# ---------------------------------------------------------------------------------------------- refusals

def test_refused_launches_raise(dev):
    kern = ops._kern()
    bf = dict(dtype=torch.bfloat16, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError):
        ops.topk_softmax(torch.zeros(2, mr.TOPK_REFUSED_E, **bf), 2)
    with pytest.raises(RuntimeError):
        ops.topk_softmax(torch.zeros(2, 8, **bf), 9)
    w, ids = torch.zeros(2, 2, **f32), torch.zeros(2, 2, **i32)
    with pytest.raises(RuntimeError):
        kern.moe_route(w, ids, torch.zeros(2, 64, **bf), torch.zeros(mr.ROUTE_REFUSED_E, 64, **bf), True)
    with pytest.raises(RuntimeError):
        kern.moe_route(w, ids, torch.zeros(2, mr.REFUSED_H, **bf), torch.zeros(8, mr.REFUSED_H, **bf), True)
    with pytest.raises(RuntimeError):
        kern.moe_route(torch.zeros(2, 9, **f32), torch.zeros(2, 9, **i32), torch.zeros(2, 64, **bf),
                       torch.zeros(8, 64, **bf), True)                                      # K > E
    with pytest.raises(RuntimeError):
        ops.moe_align(torch.zeros(4, **i32), mr.ALIGN_REFUSED_E)
    h = mr.REFUSED_H
    pos = torch.arange(4, **i32)
    with pytest.raises(RuntimeError):
        kern.moe_gather(torch.zeros(4, h, **bf), torch.zeros(2, h, **bf), pos, 2)
    with pytest.raises(RuntimeError):
        kern.moe_combine(torch.zeros(2, h, **bf), torch.zeros(4, h, **bf), pos, torch.zeros(2, 2, **f32))
    ssp = torch.zeros(1, 256, **f32)
    with pytest.raises(RuntimeError):
        kern.moe_combine_residual(ssp, torch.zeros(2, h, **bf), torch.zeros(4, h, **bf), pos, torch.zeros(2, 2, **f32))
    t = mr.COMBINE_REFUSED_T
    with pytest.raises(RuntimeError):
        kern.moe_combine_residual(ssp, torch.zeros(t, 8, **bf), torch.zeros(t, 8, **bf), torch.arange(t, **i32),
                                  torch.zeros(t, 1, **f32))
    torch.cuda.synchronize()
    assert bool((ssp == 0).all())
