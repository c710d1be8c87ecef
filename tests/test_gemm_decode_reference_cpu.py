"""The decode-GEMM oracle (tests/gemm_decode_reference.py) before the kernel is judged by it: it equals the fp32
reference on random inputs, its slices add up, the tile-order packing round-trips and pairs gate with up, and for
every GPU case by name the exactness conditions and the SiLU sensitivity caps hold and a mutation of the inputs
(one product zeroed, two 16-byte chunks of one w row swapped, two w rows of a tile swapped, an x row replaced by
its neighbour, the last K-chunk of a slice dropped, a statistics tile dropped) moves the expected outputs. The
coverage of the case lists over the instantiated tiles is a test here, not something to check by eye.

What "moves" means per mutation: a zeroed product moves its own output element in every sample (exact modes: by
>= 1; SiLU: by > 4 tol in at least 3 of 4 samples, the sensitivity cap). The other mutations act on a whole row
or column of outputs through sums of +-1 products, where single elements coincide by chance (two rows of +-1 agree
on a sum with probability 2 - 25 %, most at kc = 32): at least half of the affected elements must move and every
affected output tensor (slab, h, ss, candidates) must differ."""

import pytest
import torch

from src import ops
from src.ops import reference as ref
from src.ops.decode_tiles import GD_TILES, gd_tile_valid, ring_slots
from tests import gemm_decode_reference as gr

INT_CASES = [c for c in gr.ALL if c.family == "int" and not c.refused]
GROUPS = sorted({(c.kind, c.wr, c.kc) for c in INT_CASES})


def test_oracle_equals_fp32_reference():
    gen = torch.Generator().manual_seed(7)
    for m, n, k, kc, sk in ((5, 96, 768, 256, 3), (33, 192, 512, 64, 5), (128, 64, 1024, 128, 1)):
        x = torch.randn(m, k, generator=gen).to(torch.bfloat16)
        w = (torch.randn(2 * n, k, generator=gen) / k ** 0.5).to(torch.bfloat16)
        parts = gr.partials(x.double(), w.double(), kc, sk)
        y = parts.sum(0)
        want = x.float() @ w.float().T
        scale = x.float().abs() @ w.float().abs().T
        assert float(((y - want.double()).abs() / scale.double()).max()) <= 1e-6
        # the slices are a partition of K in whole chunks, sizes differing by at most one chunk
        sl = gr.slices(k, kc, sk)
        assert sl[0][0] == 0 and sl[-1][1] == k and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        sizes = [(hi - lo) // kc for lo, hi in sl]
        assert all((hi - lo) % kc == 0 for lo, hi in sl) and max(sizes) - min(sizes) <= 1 and min(sizes) >= 1
        assert float((y - x.double() @ w.double().T).abs().max()) <= 1e-12
        o, _, _ = gr.silu_mul(y[:, :n], y[:, n:], 1.0)
        want = ref.silu_and_mul(want)
        assert float(((o - want.double()).abs() / (want.double().abs() + scale[:, :n].double())).max()) <= 1e-6
        ssp = torch.rand(4, 128, generator=gen) * k
        r = gr.row_scale(ssp, m, k)
        assert torch.allclose(r, torch.rsqrt(ssp[:, :m].double().sum(0) / k + gr.EPS), rtol=1e-14)


def test_half_ulp():
    o = torch.tensor([1.0, 1.5, 255.0, 256.0, 0.0, 2.0 ** -126, 2.0 ** -130, 3e-39], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -1, 2.0 ** 0, 2.0 ** -134, 2.0 ** -134, 2.0 ** -134, 2.0 ** -134],
                        dtype=torch.float64)
    assert torch.equal(gr.half_ulp_bf16(o), want)
    b = torch.tensor([1.0, 255.0, 3.0e5]).to(torch.bfloat16)
    nxt = (b.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal(gr.half_ulp_bf16(b.double()), (nxt.double() - b.double()) / 2)


@pytest.mark.parametrize("wr,kc", GD_TILES)
def test_pack_round_trip_and_silu_pairing(wr, kc):
    gen = torch.Generator().manual_seed(wr * 1000 + kc)
    k = 3 * kc
    w = torch.randn(3 * wr, k, generator=gen).to(torch.bfloat16)
    wt = ops.gd_pack_weights(w, wr, kc=kc)
    assert wt.shape == w.shape and not torch.equal(wt, w)
    assert torch.equal(ops.gd_unpack_weights(wt, wr, kc=kc), w)
    # SiLU pairing: unpacked as a plain tile order, tile t holds gate rows [t no, (t + 1) no) then the same up rows
    no, n = wr // 2, 3 * wr // 2
    un = ops.gd_unpack_weights(ops.gd_pack_weights(w, wr, silu=True, kc=kc), wr, kc=kc).view(3, wr, k)
    for t in range(3):
        assert torch.equal(un[t, :no], w[t * no:(t + 1) * no])
        assert torch.equal(un[t, no:], w[n + t * no:n + (t + 1) * no])


def test_image_rule_and_refusals():
    assert gr.REFUSED_LAUNCHES == [f"img-64x256-m{m}-{s}" for m in (65, 127, 128) for s in ("nt", "ld")]
    assert gr.REFUSED_AMAX == [c.name for c in gr.ALL if c.kind == "epi" and c.mode == 0 and c.wr in (48, 96, 112)]
    assert all(gr.amax_ok(wr) == (wr in (32, 64, 128)) for wr, _ in GD_TILES)
    for c in gr.ALL:
        for m, nt in c.rows:
            assert gr.select_xr(c.wr, c.kc, m, nt) == c.xr, c.name
    # every image boundary on both load paths, and every way the waves share a chunk
    kinds = {(2 if c.xr >= 64 else (0 if c.kc >= 128 else 1)) for n in gr.IMAGE_CASES for c in [gr.case(n)] if c.xr}
    assert kinds == {0, 1, 2}
    assert {c.xr for n in gr.IMAGE_CASES for c in [gr.case(n)]} == {16, 32, 64, 128, None}


def test_coverage():
    """Every instantiated (wr, kc, XR) runs one chunk and a wrapped ring, row-major and tile order, and every
    epilogue it is eligible for."""
    valid = [(wr, kc, xr) for wr, kc in GD_TILES for xr in gr.XRS if gd_tile_valid(wr, kc, xr)]
    assert valid == list(gr.VALID) and len(valid) >= 40
    by = {}
    for c in gr.ALL:
        by.setdefault((c.kind, c.wr, c.kc, c.xr), []).append(c)
    for wr, kc, xr in valid:
        s = ring_slots(wr, kc, xr)
        ring = by[("ring", wr, kc, xr)]
        one = {c.tch for c in ring if c.sk == 1}
        assert {1, 2, s, s + 1, 2 * s + 1} <= one and (s - 1 in one or s == 1), (wr, kc, xr)
        assert {(c.sk, c.tch) for c in ring if c.sk > 1} == {(2, 3), (3, 4), (3, 5)}
        assert all(len(c.rows) == 2 or c.rows[0][0] == 1 or xr == 16 for c in ring)
        assert all(max(m for m, _ in c.rows) == xr for c in ring)
        epi = by[("epi", wr, kc, xr)]
        wrap = min(s + 1, 1280 // kc)  # SiLU cases keep K <= 1,280 (sensitivity caps); the ring sweep wraps every ring
        assert {c.tch for c in epi if c.mode == 0} == {1, s + 1} and {c.tch for c in epi if c.mode == 1} == {1, wrap}
        assert all(c.amax for c in epi if c.mode == 0)
        counts = (1, 2, 8, 9, 255, 256) if xr <= 32 else (1, 127, 128)
        assert {c.tiles for c in epi if c.mode == 4} == set(counts)
        assert {c.tch for c in epi if c.mode == 4} == {1, wrap}
        assert {c.sk for c in epi if c.mode == 6} == {1, 2, 3, 4}
        assert {c.sk for c in epi if c.mode == 3 and not c.half_ring} == ({1, 2, 3, 4, 5, 8} if wr in (32, 64, 128) else set())
        if wr in (32, 64, 128) and gr.half_ring_slots(wr, kc, xr):
            assert any(c.half_ring for c in epi)
        assert {c.mode for c in by[("grouped", wr, kc, xr)]} == {0, 1}
    grp = [gr.case(n) for n in gr.GROUPED_CASES]
    for xr in gr.XRS:
        assert {(c.segs, c.gather) for c in grp if c.xr == xr} == {(1, False), (2, False), (1, True), (2, True)}
    assert all(c.counts == (0, 1, c.xr - 1, c.xr, 0, 3) for c in grp)
    # split cases take slices of one chunk and of several, in both layouts (the GPU test runs every case in both)
    for mode, sks in ((3, (2, 3, 4, 5, 8)), (6, (2, 3, 4))):
        split = [c for c in gr.ALL if c.kind == "epi" and c.mode == mode and not c.half_ring]
        for wr in {c.wr for c in split}:
            for sk in sks:  # every wr sees every split count with one-chunk slices and with longer ones
                assert {c.tch == sk for c in split if c.wr == wr and c.sk == sk} == {True, False}, (mode, wr, sk)
    assert sorted(gr.case(n).mode for n in gr.RANDOM_CASES) == [0, 1, 2, 3, 4, 6]
    assert all(c.tch <= 17 and c.mx <= 128 and 3 * c.wr <= 384 for c in gr.ALL)


def _outputs(c, e):
    """Every tensor the GPU test compares for a launch, as float64."""
    if c.mode == 0:
        out = {"y": e.yb.double()}
        if c.amax and gr.amax_ok(c.wr):
            out["amax"] = torch.stack([e.amax_val, e.amax_col.double()], 2)
        return out
    if c.mode == 2:
        return {"y": e.parts.permute(1, 2, 0)}
    if c.mode == 3:
        out = {"y": e.h.double(), "ss": e.ss.T}
        if c.sk > 1:
            out["slab"] = e.parts.permute(1, 2, 0)
        return out
    out = {"y": e.o}
    if c.mode == 6 and c.sk > 1:
        out["slab"] = e.slab6.permute(1, 2, 0)
    return out


def _moved(c, a, b, key):
    """Boolean map of the elements of output `key` that the mutation moved (SiLU output: by more than 4 tol)."""
    if key == "y" and c.silu:
        return (a.o - b.o).abs() > 4 * a.tol
    return _outputs(c, a)[key] != _outputs(c, b)[key]


def _check_case(c):
    i = gr.inputs(c.name)
    gr.conditions(c.name)
    if c.kind == "grouped":
        parts, resid, ssp, m = i.y[None], None, None, i.r
        x, w = i.xs, None
    else:
        parts, resid, ssp, m = i.parts, i.resid, i.ssp, c.mx
        x, w = i.x.double(), i.w.double()
    base = gr.finish(c, parts, m, resid, ssp)
    gen = torch.Generator().manual_seed(c.seed + 1)
    rnd = lambda n: int(torch.randint(0, n, (1,), generator=gen))  # noqa: E731
    if c.silu:
        rows = i.inside if c.kind == "grouped" else slice(None)
        ins = ~gr.sensitivity(base.g, base.u, base.r)[rows]
        share, row, col = float(ins.float().mean()), float(ins.float().mean(1).max()), float(ins.float().mean(0).max())
        assert share <= 0.10 and row <= 0.25 and col <= 0.25, f"{c.name}: insensitive {share:.3f}, row {row:.3f}, column {col:.3f}"
    if c.kind == "grouped":
        return  # the grouped form shares the mutations of the dense cases of its tile (same oracle functions)
    sl = gr.slices(c.k, c.kc, c.sk)
    ncol = parts.shape[2]
    outcol = (lambda n: n % c.n) if c.silu else (lambda n: n)

    # one product zeroed
    hits = 0
    for _ in range(4):
        mm, n, k = rnd(m), rnd(ncol), rnd(c.k)
        by = next(b for b, (lo, hi) in enumerate(sl) if lo <= k < hi)
        p = parts.clone()
        p[by, mm, n] -= x[mm, k] * w[n, k]
        mut = gr.finish(c, p, m, resid, ssp)
        hits += bool(_moved(c, base, mut, "y")[mm, outcol(n)].any())
        if "slab" in _outputs(c, base):
            assert bool(_moved(c, base, mut, "slab")[mm].any())
    assert hits == 4 or (c.silu and hits >= 3), f"{c.name}: a zeroed product moved {hits} of 4 outputs"

    def column_mutation(p, cols, what):
        mut = gr.finish(c, p, m, resid, ssp)
        mv = _moved(c, base, mut, "y")[:, [outcol(n) for n in cols]]
        assert float(mv.float().mean()) >= 0.5, f"{c.name}: {what} moved {float(mv.float().mean()):.2f} of its column"
        for key in _outputs(c, base):
            if key not in ("amax", "ss"):  # a swap inside a tile keeps its maximum and its sum of squares
                assert bool(_moved(c, base, mut, key).any()), f"{c.name}: {what} left {key} unchanged"

    # two 16-byte chunks of one w row swapped: of eight seeded (row, chunk pair) picks whose chunks differ in at
    # least four places, the first that moves half of its column (a pair of chunks that mostly agree moves few rows)
    best = 0.0
    for _ in range(8):
        n, (a, b) = rnd(ncol), sorted(torch.randperm(c.k // 8, generator=gen)[:2].tolist())
        w1 = w[n:n + 1].clone()
        w1[0, 8 * a:8 * a + 8], w1[0, 8 * b:8 * b + 8] = w[n, 8 * b:8 * b + 8], w[n, 8 * a:8 * a + 8]
        if int((w1 != w[n:n + 1]).sum()) < 8:
            continue
        p = parts.clone()
        p[:, :, n] = gr.partials(x, w1, c.kc, c.sk)[:, :, 0]
        mv = _moved(c, base, gr.finish(c, p, m, resid, ssp), "y")[:, outcol(n)]
        best = max(best, float(mv.reshape(m, -1).any(1).float().mean()))
        if best >= 0.5:
            break
    assert best >= 0.5, f"{c.name}: no chunk swap moved half of its column ({best:.2f})"

    # two w rows of a tile swapped (columns 2 and 3 of a tile are never copies of each other)
    n1 = rnd(ncol // c.no) * c.no + 2
    p = parts.clone()
    p[:, :, [n1, n1 + 1]] = parts[:, :, [n1 + 1, n1]]
    column_mutation(p, (n1, n1 + 1), "row swap")

    # an x row replaced by its neighbour
    if m >= 2:
        mm = rnd(m)
        nb = mm + 1 if mm + 1 < m else mm - 1
        p = parts.clone()
        p[:, mm] = parts[:, nb]
        mut = gr.finish(c, p, m, resid, ssp)
        mv = _moved(c, base, mut, "y")[mm]
        assert float(mv.float().mean()) >= 0.5, f"{c.name}: row {mm} <- {nb} moved {float(mv.float().mean()):.2f}"
        for key in _outputs(c, base):
            assert bool(_moved(c, base, mut, key)[mm].any()), f"{c.name}: row replacement left {key} unchanged"

    # the last K-chunk of a slice dropped
    by = rnd(c.sk)
    hi = sl[by][1]
    p = parts.clone()
    p[by] -= x[:, hi - c.kc:hi] @ w[:, hi - c.kc:hi].T
    mut = gr.finish(c, p, m, resid, ssp)
    mv = _moved(c, base, mut, "y")
    mv = mv[..., by] if c.mode == 2 else mv
    assert float(mv.float().mean()) >= 0.5, f"{c.name}: dropped chunk moved {float(mv.float().mean()):.2f}"
    for key in _outputs(c, base):
        assert bool(_moved(c, base, mut, key).any()), f"{c.name}: dropped chunk left {key} unchanged"

    # every row's witness statistics tile dropped, and doubled
    if c.tiles:
        wt = ssp[:, :m].argmax(0)
        for f in (0.0, 2.0):
            s2 = ssp.clone()
            s2[wt, torch.arange(m)] *= f
            mv = _moved(c, base, gr.finish(c, parts, m, resid, s2), "y")
            assert float(mv.float().mean()) >= 0.75, f"{c.name}: witness tile x {f} moved {float(mv.float().mean()):.2f}"


@pytest.mark.parametrize("kind,wr,kc", GROUPS)
def test_cases_conditions_and_mutations(kind, wr, kc):
    cases = [c for c in INT_CASES if (c.kind, c.wr, c.kc) == (kind, wr, kc)]
    assert cases
    for c in cases:
        _check_case(c)


def test_deleting_a_product_changes_the_expectation_not_the_conditions():
    """The statement the GPU test rests on, at the level of the inputs: with one product's operand removed (x set
    to 0 there for one output column's weight copy), the conditions still hold and the expected output differs."""
    picks = [next(c for c in INT_CASES if c.kind == kind and c.mode == mode and c.sk == sk)
             for kind, mode, sk in (("epi", 0, 1), ("epi", 3, 4), ("ring", 2, 3))]
    for c in picks:
        i = gr.inputs(c.name)
        gr.conditions(c.name)
        w = i.w.clone()
        w[5, 17] = 0
        p = gr.partials(i.x.double(), w.double(), c.kc, c.sk)
        assert float((i.x.double().abs() @ w.double().abs().T).max()) < 2 ** 24
        a, b = gr.finish(c, i.parts, c.mx, i.resid, i.ssp), gr.finish(c, p, c.mx, i.resid, i.ssp)
        assert bool((a.y != b.y)[:, 5].all()) and float(b.y.abs().max()) <= 256 + 3
        assert bool((_outputs(c, a)["y"] != _outputs(c, b)["y"])[:, 5].reshape(c.mx, -1).any(1).all())


def test_random_family_bounds_are_small():
    """The random family's tolerance stays a small multiple of the output rounding: it cannot hide a product."""
    for name in gr.RANDOM_CASES:
        c, i = gr.case(name), gr.inputs(name)
        m = c.mx
        e = gr.expected(name, m)
        t = gr.random_bounds(c, i, e, m)
        assert float((t.parts / i.absum[:m].clamp_min(1e-30)).max()) <= (c.k + c.sk) * 2.0 ** -24
        one = (i.x[:m, :1].double() * i.w[:, :1].double().T).abs()     # the products of k = 0
        if c.mode == 2:
            assert float((t.parts[0] < one / 4).float().mean()) >= 0.9
