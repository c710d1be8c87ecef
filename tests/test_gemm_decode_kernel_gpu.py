"""The decode GEMM (csrc/kernels/gemm_decode.hip) element by element against the float64 oracle of
tests/gemm_decode_reference.py on its case lists: every instantiated (wr, kc, XR) with rings of 1 .. 2 S + 1
chunks and uneven splits, row-major and tile-order weights, the image selection at every M boundary on both load
paths, all six epilogues, the half ring, the greedy candidates with forced ties, and the grouped form.
test_gemm_decode_reference_cpu.py proves for every case used here that a single wrong product changes the
expectation. Integer family: torch.equal on every output of modes 0, 2 and 3, on ss, on the candidates and on
mode 6's slab; SiLU outputs within the derived bound. Everything sits in poisoned buffers: x, w and the statistics
are views of NaN-filled ones, every output a view of a sentinel-filled one that must be bit-identical outside the
specified region; tickets read zero after every launch and every split launch runs twice. A launch that the
launcher has to refuse must raise. Each test prints its worst err / tol."""

from dataclasses import replace

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.ops.decode_tiles import GD_TILES, HALF_RING, TILED  # noqa: E402
from tests import gemm_decode_reference as gr  # noqa: E402

NAN = float("nan")
WORST: dict = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), "HIP extension must be built for GPU tests"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _poisoned(t, dev, pad_rows=2, pad_cols=8, lead=0):
    """t [rows, cols] as a view of a NaN-filled buffer with more rows (before and after) and a longer row stride."""
    buf = torch.full((lead + t.shape[0] + pad_rows, t.shape[1] + pad_cols), NAN, dtype=t.dtype, device=dev)
    v = buf[lead:lead + t.shape[0], : t.shape[1]]
    v.copy_(t)
    return v


def _weights(w, dev):
    """w as a contiguous row range of a NaN-filled buffer."""
    flat = w.reshape(-1, w.shape[-1])
    return _poisoned(flat, dev, pad_rows=2, pad_cols=0, lead=2).view(w.shape)


class _Sentinel:
    """An output tensor as a view of a sentinel-filled buffer; untouched() is true when everything outside the
    regions handed to it still holds the sentinel."""

    def __init__(self, shape, dtype, dev, view, value=gr.SENT):
        self.value = int(value) if dtype == torch.int32 else value
        self.buf = torch.full(shape, self.value, dtype=dtype, device=dev)
        self.t = view(self.buf)

    def untouched(self, *written):
        """written: index expressions into the buffer that the kernel may have changed."""
        c = self.buf.clone()
        for idx in written:
            c[idx] = self.value
        return _same(c, torch.full_like(c, self.value))


def _flat(numel, dev):
    """A contiguous fp32 region between two 4-float guards."""
    return _Sentinel((numel + 8,), torch.float32, dev, lambda b: b[4:-4])


def _judge(label, y, o, tol):
    y = y.cpu().double()
    assert bool(torch.isfinite(y).all()), f"{label}: non-finite output"
    r = (y - o).abs() / tol
    i = int(r.argmax())
    assert float(r.max()) <= 1, f"{label}: {int((r > 1).sum())} elements off; worst err/tol {float(r.max()):.3f} at " \
                               f"flat index {i}: got {y.flatten()[i]:.9g}, oracle {o.flatten()[i]:.9g}"
    return float(r.max())


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def _launch(c, i, m, nt, tiled, w, dev, argmax=False):
    """One launch of m rows; returns the outputs on the CPU after the sentinel and ticket checks."""
    k = ops._kern()
    n, sk = c.n, c.sk
    x = _poisoned(i.x[:m], dev)
    mode = c.mode | (TILED if tiled else 0) | (HALF_RING if c.half_ring else 0)
    e = torch.empty(0, device=dev)
    out = {}
    cnt = _Sentinel((gr.NTILES + 1,), torch.int32, dev, lambda b: b[: gr.NTILES], gr.SENT_I)
    cnt.t.zero_()
    resid = ssp_out = ssp_in = e
    if c.mode in (2, 3):
        ys = _flat(sk * m * n, dev)
        y = ys.t.view(sk, m, n)
    elif argmax:
        ys = _Sentinel((m + 2, n), torch.bfloat16, dev, lambda b: b[:m])
        y = ys.t
        am = _Sentinel((m + 2, gr.NTILES, 2), torch.int32, dev, lambda b: b, gr.SENT_I)
    else:
        ys = _Sentinel((m + 2, n + 8), torch.bfloat16, dev, lambda b: b[:m, :n])
        y = ys.t
    if c.mode == 3:
        rs = _Sentinel((m + 2, n + 8), torch.bfloat16, dev, lambda b: b[:m, :n])
        rs.t.copy_(i.resid[:m])
        so = _Sentinel((gr.NTILES + 1, gr.SSP_LD), torch.float32, dev, lambda b: b)
        resid, ssp_out = rs.t, so.t
    if c.mode in (4, 6):
        s = i.ssp.clone()
        s[:, m:] = NAN
        ssp_in = _poisoned(s, dev, pad_rows=3, pad_cols=0)
    if c.mode == 6 and sk > 1:
        s6 = _flat(sk * m * 2 * n, dev)
        ssp_out = s6.t
    counters = cnt.t if (c.mode in (3, 6) and sk > 1) else e
    if argmax:
        k.gemm_decode_argmax(y, x, w, c.wr, c.kc, tiled, am.t)
    else:
        k.gemm_decode(y, x, w, mode, c.wr, c.kc, sk, nt, resid, ssp_out, counters, ssp_in, gr.EPS)
    torch.cuda.synchronize()
    tag = f"{c.name} M={m} nt={nt} tiled={tiled}"
    assert int(cnt.t.abs().sum()) == 0 and cnt.untouched(slice(0, gr.NTILES)), f"{tag}: tickets not re-armed"
    if c.mode in (2, 3):
        written = c.mode == 2 or sk > 1
        assert ys.untouched(*([slice(4, -4)] if written else [])), f"{tag}: slab guard or unused slab written"
        out["slab"] = y.cpu() if written else None
    elif argmax:
        assert ys.untouched(slice(0, m)) and am.untouched(slice(0, m)), f"{tag}: rows >= M written"
        out["y"], out["amax"] = y.cpu(), am.t[:m].cpu()
    else:
        assert ys.untouched((slice(0, m), slice(0, n))), f"{tag}: y written outside [M, N]"
        out["y"] = y.cpu()
    if c.mode == 3:
        assert rs.untouched((slice(0, m), slice(0, n))), f"{tag}: resid written outside [M, N]"
        assert so.untouched((slice(0, gr.NTILES), slice(0, c.rr))), f"{tag}: ssp_out written outside [tiles, RR]"
        out["h"], out["ss"] = rs.t.cpu(), so.t[: gr.NTILES, : c.rr].cpu()
    if c.mode == 6 and sk > 1:
        assert s6.untouched(slice(4, -4)), f"{tag}: slab guard written"
        out["slab6"] = s6.t.view(sk, m, 2 * n).cpu()
    return out


def _check_exact(c, e, out, m, tag):
    if c.mode == 0:
        assert _same(out["y"], e.yb), f"{tag}: y differs in {int((out['y'] != e.yb).sum())} elements"
        if "amax" in out:
            val = out["amax"][..., 0].contiguous().view(torch.float32)
            assert torch.equal(val, e.amax_val.float()), f"{tag}: candidate values"
            assert torch.equal(out["amax"][..., 1].long(), e.amax_col), f"{tag}: candidate columns (lowest of a tie)"
    if c.mode in (2, 3) and out["slab"] is not None:
        assert torch.equal(out["slab"], e.parts.float()), \
            f"{tag}: slab differs in {int((out['slab'] != e.parts.float()).sum())} elements"
    if c.mode == 3:
        assert _same(out["h"], e.h), f"{tag}: residual differs in {int((out['h'] != e.h).sum())} elements"
        assert torch.equal(out["ss"][:, :m], e.ss.float()), f"{tag}: ss"
        assert bool((out["ss"][:, m:] == 0).all()), f"{tag}: ss rows M .. RR - 1 not zero"
    if c.mode == 6 and "slab6" in out:
        assert torch.equal(out["slab6"], e.slab6.float()), f"{tag}: mode 6 slab"


def _run_dense(c, dev):
    """Every launch of a dense case: rows x layouts (x twice when split), against the oracle."""
    i = gr.inputs(c.name)
    ws = {False: _weights(i.w, dev),
          True: _weights(ops.gd_pack_weights(i.w, c.wr, silu=c.silu, kc=c.kc), dev)}
    worst = 0.0
    for m, nt in c.rows:
        e = gr.expected(c.name, m)
        tol = gr.random_bounds(c, i, e, m) if c.family == "random" else None
        outs = []
        for tiled in (False, True):
            tag = f"{c.name} M={m} nt={nt} tiled={tiled}"
            out = _launch(c, i, m, nt, tiled, ws[tiled], dev)
            if c.sk > 1:
                again = _launch(c, i, m, nt, tiled, ws[tiled], dev)
                assert all(v is None or _same(v, again[key]) for key, v in out.items()), f"{tag}: second launch differs"
            if c.amax:
                am = _launch(c, i, m, True, tiled, ws[tiled], dev, argmax=True)
                assert nt and _same(am["y"], out["y"]), f"{tag}: the candidate launch wrote another y"
                out["amax"] = am["amax"]
            outs.append(out)
            if c.family == "int":
                _check_exact(c, e, out, m, tag)
                if c.silu:
                    worst = max(worst, _judge(tag, out["y"], e.o, e.tol))
            else:
                worst = max(worst, _check_random(c, e, tol, out, m, tag))
        assert all(v is None or _same(v, outs[1][key]) for key, v in outs[0].items()), \
            f"{c.name} M={m}: row-major and tile-order weights give different bits"
    return worst


def _check_random(c, e, t, out, m, tag):
    worst = 0.0
    if out.get("slab") is not None:
        worst = max(worst, _judge(tag + " slab", out["slab"], e.parts, t.parts))
    if "slab6" in out:
        worst = max(worst, _judge(tag + " slab6", out["slab6"], e.slab6, gr.slab6_layout(t.parts, c.wr)))
    if c.mode == 0:
        worst = max(worst, _judge(tag, out["y"], e.y, t.y))
        v = out["y"].double().view(m, gr.NTILES, c.wr)   # the candidates of the kernel's own rounded outputs
        val = v.max(2).values
        col = (v == val[:, :, None]).to(torch.int32).argmax(2) + torch.arange(gr.NTILES) * c.wr
        assert torch.equal(out["amax"][..., 0].contiguous().view(torch.float32), val.float()), f"{tag}: candidate values"
        assert torch.equal(out["amax"][..., 1].long(), col), f"{tag}: candidate columns"
    if c.mode == 3:
        worst = max(worst, _judge(tag + " h", out["h"], e.h64, t.h))
        ss = out["h"].double().pow(2).view(m, gr.NTILES, c.wr).sum(2).T   # of the residual the kernel wrote
        worst = max(worst, _judge(tag + " ss", out["ss"][:, :m], ss, c.wr * 2.0 ** -24 * ss + 1e-30))
        assert bool((out["ss"][:, m:] == 0).all())
    if c.silu:
        worst = max(worst, _judge(tag, out["y"], e.o, t.o))
    return worst


def _run_refused(c, dev, argmax=False):
    i = gr.inputs(c.name) if not c.refused else None
    for m, nt in c.rows:
        if i is None:
            x = torch.ones(m, c.k, dtype=torch.bfloat16, device=dev)
            w = torch.ones(gr.NTILES * c.wr, c.k, dtype=torch.bfloat16, device=dev)
            y = torch.full((c.sk, m, c.n), gr.SENT, device=dev)
            e = torch.empty(0, device=dev)
            with pytest.raises(RuntimeError):
                ops._kern().gemm_decode(y, x, w, c.mode, c.wr, c.kc, c.sk, nt, e, e, e, e, 0.0)
            assert bool((y == gr.SENT).all()), f"{c.name}: a refused launch wrote"
        else:
            with pytest.raises(RuntimeError):
                _launch(c, i, m, True, False, _weights(i.w, dev), dev, argmax=True)


def _tile_cases(kind, wr, kc):
    return [c for c in gr.ALL if c.kind == kind and (c.wr, c.kc) == (wr, kc)]


@pytest.mark.parametrize("wr,kc", GD_TILES)
def test_ring_sweep(dev, wr, kc):
    """Mode 2 on every image of the tile: 1, 2, S - 1, S, S + 1 and 2 S + 1 chunks in one slice, uneven splits of
    1 and 2 chunks per slice (sk = 2 of 3 chunks, sk = 3 of 4 and 5), M at the top of the image and the smallest M
    that selects it; row-major and tile order give the oracle's bits."""
    cases = _tile_cases("ring", wr, kc)
    assert cases
    for c in cases:
        _run_dense(c, dev)
    print(f"ring sweep {wr}x{kc}: {len(cases)} cases exact")


@pytest.mark.parametrize("wr,kc", gr.IMAGE_TILES)
def test_image_selection(dev, wr, kc):
    """M = 1, 15 .. 17, 31 .. 33, 63 .. 65, 127, 128 with and without nt; where no image holds M the launch raises."""
    cases = _tile_cases("image", wr, kc)
    assert len(cases) == 2 * len(gr.IMAGE_MS)
    refused = 0
    for c in cases:
        if c.refused:
            _run_refused(c, dev)
            refused += 1
        else:
            _run_dense(c, dev)
    assert refused == sum(c.name in gr.REFUSED_LAUNCHES for c in cases)
    print(f"image selection {wr}x{kc}: {len(cases) - refused} launches exact, {refused} refused")


@pytest.mark.parametrize("wr,kc", GD_TILES)
def test_epilogues(dev, wr, kc):
    """Modes 0 (with and without candidates, ties forced), 1, 3 (sk 1 - 5 and 8, strided residual, half ring), 4
    (1 .. 256 statistics tiles) and 6 (sk 1 - 4, slab against the partials) on every image of the tile."""
    cases = _tile_cases("epi", wr, kc)
    assert cases
    worst = {}
    for c in cases:
        if c.amax and not gr.amax_ok(c.wr):
            assert c.name in gr.REFUSED_AMAX
            _run_refused(c, dev, argmax=True)
            r = _run_dense(replace(c, amax=False), dev)
        else:
            r = _run_dense(c, dev)
        if c.silu:
            worst[c.mode] = max(worst.get(c.mode, 0.0), r)
            _note(f"int mode {c.mode}", r)
    print(f"epilogues {wr}x{kc}: {len(cases)} cases; SiLU worst err/tol by mode {worst}")


@pytest.mark.parametrize("xr", gr.XRS)
def test_grouped(dev, xr):
    """gemm_decode_grouped, modes 0 and 1, max_rows = the image: groups that are empty and of 1, XR - 1, XR and 3
    rows, one and two segments per expert, sorted rows and rows gathered with k = 2; rows of y outside every group
    keep the sentinel."""
    cases = [c for c in gr.ALL if c.kind == "grouped" and c.xr == xr]
    assert cases
    worst = 0.0
    for c in cases:
        i = gr.inputs(c.name)
        x = _poisoned(i.x, dev)
        w = _weights(i.w, dev)
        ys = _Sentinel((i.r + 2, c.n + 8), torch.bfloat16, dev, lambda b: b[: i.r, : c.n])
        rows = i.rowmap.to(dev) if c.gather else torch.empty(0, dtype=torch.int32, device=dev)
        ops._kern().gemm_decode_grouped(ys.t, x, w, i.offsets.to(dev), c.mode, c.wr, c.kc, rows, i.k, xr, c.segs)
        torch.cuda.synchronize()
        inside = i.inside.nonzero().flatten().to(dev)
        assert ys.untouched((inside[:, None], torch.arange(c.n, device=dev)[None, :])), \
            f"{c.name}: rows outside every group (or columns >= N) written"
        y = ys.t.cpu()[i.inside]
        e = gr.finish(c, i.y[None], i.r)
        if c.mode == 0:
            assert _same(y, e.yb[i.inside]), f"{c.name}: y differs in {int((y != e.yb[i.inside]).sum())} elements"
        else:
            worst = max(worst, _judge(c.name, y, e.o[i.inside], e.tol[i.inside]))
    _note("int mode 1 grouped", worst)
    print(f"grouped XR={xr}: {len(cases)} cases; SiLU worst err/tol {worst:.3f}")


@pytest.mark.parametrize("name", gr.RANDOM_CASES)
def test_random_family(dev, name):
    """Magnitudes like the workload's, one case per epilogue, within the summation bound of the module docstring."""
    c = gr.case(name)
    r = _run_dense(c, dev)
    _note(f"random mode {c.mode}", r)
    print(f"{name}: worst err/tol {r:.3f}")


def test_report():
    """Prints the worst err / tol of the module's tolerance-judged families (docs/performance.md records them)."""
    print("decode GEMM oracle, worst err/tol:", {k: round(v, 3) for k, v in sorted(WORST.items())})
