"""The row-kernel oracles (tests/rowwise_reference.py) before any kernel is judged by them: they equal the fp32
reference (src/ops/reference.py) on ordinary inputs and closed forms where a family has one, and for every GPU case
by name the exactness conditions hold, at most 1 % of the elements are undecided, and every mutation that applies
to the case (a 16-byte chunk left out of the statistics, hidden +- 8 in the mean, eps = 0, statistics of the
unrounded sum, a neighbouring row's scale, a dropped or doubled slab, swapped rotation halves, the sign of the sine
term, the table row of position +- 1, a neighbouring token's or head's slot, the row scale on q or left off v, gate
and up swapped, the row scale applied once) moves the expectation on at least 8 decided elements of every affected
row or head, or a statistic by more than 4 tol. The coverage of the lists over the kernels' instantiations is a test
here too."""

import pytest
import torch

from src.ops import reference as ref
from tests import rowwise_reference as rr

NEED = rr.MIN_CHANGED


def _rows_changed(e, m, c):
    """Per row: decided elements of e whose expectation the mutated m leaves."""
    ch = rr.changed(e.o, e.s, m.o, m.s, c)
    return ch.reshape(ch.shape[0], -1).sum(-1)


# ---------------------------------------------------------------------------------------------- the tools

def test_rne_bf16_and_bracket():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(20000, generator=gen, dtype=torch.float64) * 10.0 ** torch.randint(-30, 30, (20000,), generator=gen)
    r = rr.rne_bf16(x)
    assert torch.equal(r, r.to(torch.bfloat16).double())                    # representable
    assert bool(((r - x).abs() <= rr.half_ulp_bf16(x)).all())               # nearest
    far = ((x - x.to(torch.bfloat16).double()).abs() < 0.49 * 2 * rr.half_ulp_bf16(x))
    assert torch.equal(r[far], x.to(torch.bfloat16).double()[far])         # torch's rounding away from ties
    # ties go to even, in one rounding: 1 + 2^-8 + 2^-40 is above the tie, a float round trip would put it on it
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, -(1 + 2.0 ** -8)], dtype=torch.float64)
    assert rr.rne_bf16(t).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0]
    o = torch.tensor([1.0, 1 + 2.0 ** -8 - 1e-9, 3e-39, 0.0], dtype=torch.float64)
    lo, hi = rr.bracket(o, o.abs(), 8.0)
    assert (lo == hi).tolist() == [True, False, True, True]
    sub = float(rr.rne_bf16(o[2:3]))
    assert sub != 3e-39 and abs(sub - 3e-39) <= 2.0 ** -134
    j = rr.judge(torch.tensor([1.0, 1 + 2.0 ** -7, sub, -0.0], dtype=torch.float64), o, o.abs(), 8.0)
    assert j.ok.tolist() == [True, True, True, True] and j.undecided == 0.25
    assert not bool(rr.judge(torch.tensor([1 + 2.0 ** -7]).to(torch.bfloat16), o[:1], o[:1].abs(), 8.0).ok.any())
    assert rr.same_bits(torch.tensor([0.0]), torch.tensor([0.0])) and not rr.same_bits(torch.tensor([0.0]),
                                                                                       torch.tensor([-0.0]))


def test_constants():
    assert [rr.c_norm(h) for h in (8, 2048, 2056, 16384)] == [7.0, 7.0, 9.0, 21.0]
    assert [rr.sum_depth(h) for h in (8, 2048, 2056, 8192)] == [18, 18, 26, 42]
    assert rr.EPS32 != rr.EPS and abs(rr.EPS32 - rr.EPS) < 1e-12


def test_oracles_equal_fp32_reference():
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(5, 4104, generator=gen).to(torch.bfloat16)
    res = torch.randn(5, 4104, generator=gen).to(torch.bfloat16)
    w = torch.randn(4104, generator=gen).to(torch.bfloat16)
    o, _ = rr.norm_y(x, w, rr.sumsq(x), 4104)
    assert torch.allclose(o.float(), ref.rms_norm(x, w, rr.EPS).float(), rtol=1e-2, atol=2e-2)
    y, r = ref.fused_add_rms_norm(x, res, w, rr.EPS)
    h = rr.added(res, x)
    assert rr.same_bits(h, r)
    assert torch.allclose(rr.norm_y(h, w, rr.sumsq(h), 4104)[0].float(), y.float(), rtol=1e-2, atol=2e-2)
    # slabs: sequential fp32 sums, and the same thing through the fused op of the summed slab where that is exact
    slab = torch.stack([x.float() * k for k in (3, -2)])
    assert rr.same_bits(rr.slab_sum(slab, res).to(torch.bfloat16), h)
    assert torch.equal(rr.slab_sum(slab), x.float())
    g = torch.cat([x, res], 1)
    o, _, _ = rr.silu_mul(x, res)
    assert torch.allclose(o.float(), ref.silu_and_mul(g).float(), rtol=1e-2, atol=2e-2)
    rs = torch.rand(5, generator=gen) + 0.5
    o2, _, _ = rr.silu_mul(x, res, rs)
    want = torch.nn.functional.silu(x.float() * rs[:, None]) * (res.float() * rs[:, None])
    assert torch.allclose(o2.float(), want, rtol=1e-4, atol=1e-5)
    assert torch.allclose(rr.real_table(128), ref.rope_cos_sin(rr.MAX_POS, 128, rr.ROPE_THETA))
    assert torch.allclose(rr.real_table(64), ref.rope_cos_sin(rr.MAX_POS, 64, rr.ROPE_THETA))


@pytest.mark.parametrize("name", ["rope-d128-h8x1-b16-real-q", "rope-d64-h4x4-b32-real-q"])
def test_rope_oracle_equals_fp32_reference(name):
    i = rr.rope_inputs(name)
    c = i.c
    e = rr.rope_expected(name)
    qkv = i.qkv.clone()
    kc = torch.zeros(rr.ROPE_BLOCKS, c.hkv, c.block_size, c.d, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    ref.rope_and_cache(qkv, i.positions, i.table, i.slots, kc, vc, c.hq, c.hkv, c.d)
    assert torch.allclose(e.q.reshape(rr.ROPE_TOKENS, -1).float(), qkv[:, : c.hq * c.d].float(), rtol=1e-2, atol=2e-2)
    assert torch.allclose(e.k.float(), kc.float(), rtol=1e-2, atol=2e-2)
    assert torch.equal(e.v.to(torch.bfloat16), vc)
    assert int(e.written.sum()) == 5 * c.hkv * c.d and not bool(e.written[1].any()) and not bool(e.written[3].any())


def test_closed_forms():
    # biased family: the rounded sum is the residual itself, the unrounded statistics are (257 / 256)^2 larger
    i = rr.row_inputs("norm-h4096-biased")
    e = rr.norm_expected("norm-h4096-biased", "add")
    assert rr.same_bits(e.h, i.resid)
    u = rr.norm_expected("norm-h4096-biased", "add", unrounded=True)
    ratio = u.ss / e.ss      # every element grows by half an ulp: (1 + 1 / 2M)^2 with the mantissa M in 128 .. 254
    assert bool((ratio > (1 + 1 / 508) ** 2).all()) and bool((ratio < (1 + 1 / 256) ** 2).all())
    assert bool((u.ss > e.ss).all()) and bool((i.x.double().abs() * 2 == 2 * rr.half_ulp_bf16(i.resid.double())).all())
    assert rr.same_bits(rr.norm_expected("norm-h4096-biased", "slab").h, i.resid)
    # int family: slabs add up to x, so the slab form leaves the fused form's residual
    for name in rr.NORM_CASES:
        if rr.ROW_CASES[name].family in ("int", "biased"):
            assert rr.same_bits(rr.norm_expected(name, "slab").h, rr.norm_expected(name, "add").h), name
    # rs: a row of +-2 has rs = rsqrt(4 + eps)
    assert abs(float(rr.rs_exact(torch.tensor([4.0 * 4096], dtype=torch.float64), 4096)) - (4 + rr.EPS32) ** -0.5) < 1e-7
    # the exact table: entries from the allowed set, neighbouring rows differ in every dim
    for d in (64, 128):
        t = rr.exact_table(d)
        assert set(t.flatten().tolist()) <= {0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0}
        pairs = torch.stack([t[:, : d // 2], t[:, d // 2:]], -1)
        for sh in (1, 2, 3):
            assert bool((pairs[sh:] != pairs[:-sh]).any(-1).all())
    # SiLU at a gate of 0 and far out
    o, _, _ = rr.silu_mul(torch.tensor([[0.0, 200.0, -800.0]]), torch.tensor([[3.0, 2.0, 2.0]]))
    assert o.tolist() == [[0.0, 400.0, 0.0]]


# ---------------------------------------------------------------------------------------------- norms

def _forms(c):
    return ("plain", "add", "slab") if c.op == "norm" else ("rs_plain", "rs_add")


@pytest.mark.parametrize("name", rr.NORM_CASES + rr.RS_CASES)
def test_norm_case(name):
    c = rr.ROW_CASES[name]
    i = rr.row_inputs(name)
    rows = c.rows
    if c.family == "int":
        for t in (i.x, i.resid) + ((i.slab,) if c.op == "norm" else ()):
            assert bool((t.double() == t.double().round()).all())
        assert bool((i.x != 0).all()) and bool((rr.added(i.resid, i.x) != 0).all())
        assert float(rr.sumsq(rr.added(i.resid, i.x)).max()) < 2 ** 24 and float(rr.sumsq(i.resid).max()) < 2 ** 24
        if c.op == "norm":
            part = i.resid.double()
            for s in range(c.sk):   # every partial sum is a small integer: exact in fp32 in any order
                part = part + i.slab[s].double()
                assert float(part.abs().max()) < 2 ** 10
    if c.family == "small":
        var = rr.sumsq(rr.added(i.resid, i.x)) / c.hidden
        assert bool((var > 2e-5).all()) and bool((var < 2e-3).all())    # eps is 0.5 .. 50 % of it
    for form in _forms(c):
        e = rr.norm_expected(name, form)
        if c.op == "rs":
            assert bool(torch.isfinite(e.rs).all()) and bool((e.rs_tol < 1e-5 * e.rs).all())
            muts = [dict(drop_weakest=True), dict(hdelta=8), dict(hdelta=-8)]
            if c.family == "small":
                muts.append(dict(eps=0.0))
            if c.family == "biased" and form == "rs_add":
                muts.append(dict(unrounded=True))
            if rows > 1:
                muts.append(dict(shift_rows=True))
            for mut in muts:
                m = rr.norm_expected(name, form, **mut)
                d = (m.rs - e.rs).abs()
                d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
                assert bool((d > 4 * e.rs_tol).all()), f"{name} {form} {mut}: rs moves by {d / e.rs_tol} tol"
            continue
        lo, hi = rr.bracket(e.o, e.s, e.c)
        assert float((lo != hi).double().mean()) <= rr.UNDECIDED_CAP, f"{name} {form}"
        need = min(NEED, c.hidden)
        muts = [dict(drop_weakest=True), dict(hdelta=8), dict(hdelta=-8)]
        if c.family == "small":
            muts.append(dict(eps=0.0))
        if c.family == "biased" and form != "plain":
            muts.append(dict(unrounded=True))
        if rows > 1:
            muts.append(dict(shift_rows=True))
        for mut in muts:
            n = _rows_changed(e, rr.norm_expected(name, form, **mut), e.c)
            assert int(n.min()) >= need, f"{name} {form} {mut}: {n.tolist()} decided elements move"
        if form == "slab":
            alts = [tuple(s for s in range(c.sk) if s != d) for d in range(c.sk)] + \
                   [tuple(range(c.sk)) + (d,) for d in range(c.sk)]
            for slabs in alts:
                m = rr.norm_expected(name, form, slabs=slabs)
                moved = (rr.bits(m.h) != rr.bits(e.h)).sum(-1)
                assert int(moved.min()) >= need, f"{name} slabs {slabs}: {moved.tolist()} residual elements move"


@pytest.mark.parametrize("name", rr.SUMSQ_CASES)
def test_sumsq_case(name):
    c = rr.ROW_CASES[name]
    i = rr.row_inputs(name)
    assert int(i.ids.min()) == 0 or int(i.ids.max()) == rr.EMBED_VOCAB - 1
    if c.rows > 2:
        assert {0, rr.EMBED_VOCAB - 1} <= set(i.ids.tolist()) and len(set(i.ids.tolist())) < c.rows
    for op in ("row", "embed", "add"):
        e = rr.sumsq_expected(name, op)
        if c.exact_stats:
            assert float(e.ss.max()) < 2 ** 24 and bool((e.ss == e.ss.round()).all()) and float(e.tol.max()) == 0
        # any chunk left out: the weakest one already moves ss by more than 4 tol
        assert bool((rr.weakest_chunk(e.h) > 4 * e.tol).all()), f"{name} {op}"
        if op == "add" and c.family == "biased":
            u = rr.sumsq_expected(name, op, unrounded=True)
            assert bool(((u.ss - e.ss).abs() > 4 * e.tol).all())
        # a neighbouring row (embed: any other table row)
        if op == "embed":
            ts = rr.sumsq(i.table)
            gap = (ts[1:] - ts[:-1]).abs()
            assert float(gap.min()) > 4 * float(rr.sumsq_tol(ts, c.hidden).max() if not c.exact_stats else 0)
        elif c.rows > 1:
            assert bool(((e.ss[1:] - e.ss[:-1]).abs() > 4 * torch.maximum(e.tol[1:], e.tol[:-1])).all()), f"{name} {op}"


# ---------------------------------------------------------------------------------------------- SiLU

def test_ladder():
    g, u = rr.ladder("ladder")
    o, _, z = rr.silu_mul(g, u)
    gd = g.double()
    band = rr._bf16_values(-92.0, -87.0)
    assert band.numel() == 11
    for v in band.tolist():                         # every bf16 gate of the band, with a normal oracle
        sel = gd == v
        assert int(sel.sum()) >= 2 and bool((o[sel].abs() >= 2.0 ** -120).all())
    assert bool(((o == 0) | (o.abs() >= 2.0 ** -120)).all()) and bool((o.abs() <= 2.0 ** 120).all())
    for v in range(-110, 111):
        assert bool((gd == v).any()), v
    assert bool((gd == rr.BF16_MAX).any()) and bool((gd == -rr.BF16_MAX).any())
    assert bool(((gd == 0) & torch.signbit(gd)).any()) and bool(((gd == 0) & ~torch.signbit(gd)).any())
    # the band where the bare reciprocal's argument is >= 2^126, and the one past the fast exp's overflow
    assert int(((gd > -88.72) & (gd <= -87.34)).sum()) >= 4 and int((gd < -88.72).sum()) >= 60
    assert g.numel() <= 2040
    g, u = rr.ladder("ladder_rs")
    for r in rr.LADDER_RS:
        o, _, z = rr.silu_mul(g, u, r)
        assert bool((o.abs() >= 2.0 ** -120).all()) and float(z.min()) < -100 and float(z.max()) > -92
        assert int((z < -88.72).sum()) >= 20
    assert g.numel() <= 2040


@pytest.mark.parametrize("name", list(rr.SILU_CASES))
def test_silu_case(name):
    c = rr.SILU_CASES[name]
    i = rr.silu_inputs(name)
    assert bool(torch.isfinite(i.gate.float()).all()) and bool(torch.isfinite(i.up.float()).all())
    e = rr.silu_expected(name)
    assert bool(torch.isfinite(e.o).all())
    lo, hi = rr.bracket(e.o, e.s, e.c)
    share = float((lo != hi).double().mean())
    assert share <= rr.UNDECIDED_CAP, f"{name}: {share:.4f} undecided"
    need = min(NEED, c.inter)
    n = _rows_changed(e, rr.silu_expected(name, swap=True), e.c)
    assert int(n.min()) >= need, f"{name} swapped: {n.tolist()}"
    if c.scaled:
        assert i.r is not None and bool((i.r != 1).all())
        n = _rows_changed(e, rr.silu_expected(name, once=True), e.c)
        assert int(n.min()) >= need, f"{name} scale once: {n.tolist()}"
        # a neighbouring row's scale
        j = rr.silu_inputs(name)
        o, s, _ = rr.silu_mul(j.gate, j.up, j.r.roll(1))
        ch = rr.changed(e.o, e.s, o, s, e.c).sum(-1)
        assert len(set(i.r.tolist())) == rr.SILU_ROWS and int(ch.min()) >= need, f"{name} neighbour scale: {ch.tolist()}"
    else:
        assert i.r is None


# ---------------------------------------------------------------------------------------------- RoPE

@pytest.mark.parametrize("name", rr.ROPE_CASES + rr.ROPE_SLAB_CASES)
def test_rope_case(name):
    c = rr.ROPE_CASES_BY_NAME[name]
    i = rr.rope_inputs(name)
    e = rr.rope_expected(name)
    assert sorted(i.slots.tolist()) == sorted([0, c.block_size - 1, (rr.ROPE_BLOCKS - 1) * c.block_size,
                                               rr.ROPE_BLOCKS * c.block_size - 1, -1, 2 * c.block_size + 3])
    assert {0, rr.MAX_POS - 1} <= set(i.positions.tolist()) and len(set(i.positions.tolist())) == rr.ROPE_TOKENS
    assert c.rot_q or not c.sk
    assert not c.scaled or not c.rot_q
    if c.family == "exact":
        # everything the kernel rounds is representable in bf16, and exact in fp32 at every step
        for t in (e.q, e.k, e.v):
            assert torch.equal(t, rr.rne_bf16(t)) and float(t.abs().max()) <= 64
        assert bool((e.q * 8 == (e.q * 8).round()).all()) and bool((e.k * 32 == (e.k * 32).round()).all())
        if c.sk:
            part = torch.zeros_like(i.slab[0], dtype=torch.float64)
            for s in range(c.sk):
                part = part + i.slab[s].double()
                assert float(part.abs().max()) < 2 ** 10 and bool((part == part.round()).all())
        if i.r is not None:
            assert bool((torch.frexp(i.r)[0] == 0.5).all()) and len(set(i.r.tolist())) > 1
        c_used = 0.0
    else:
        c_used = e.c
        for o, s in ((e.q, e.qs), (e.k[e.written], e.ks[e.written])):
            lo, hi = rr.bracket(o, s, e.c)
            assert float((lo != hi).double().mean()) <= rr.UNDECIDED_CAP, name
    need = NEED
    wr = e.written

    def kv_moved(m):
        """Per written (block, head, slot) row of the cache: decided K elements that move; V elements that differ."""
        both = wr.any(-1) & m.written.any(-1)
        assert bool(both.any())
        k = rr.changed(e.k, e.ks, m.k, m.ks, c_used).sum(-1)[both]
        v = (rr.rne_bf16(e.v) != rr.rne_bf16(m.v)).sum(-1)[both]
        return k, v

    for mut in (dict(swap_halves=True), dict(flip_sin=True), dict(pos_shift=1), dict(pos_shift=-1)):
        m = rr.rope_expected(name, **mut)
        k, _ = kv_moved(m)
        # pos_shift clamps at the table's ends: the token at position 0 / MAX_POS - 1 keeps its row for one sign
        # likewise the real table's row 0 has no sine to flip
        keep = 1 if "pos_shift" in mut or ("flip_sin" in mut and c.family == "real") else 0
        assert int((k < need).sum()) <= keep * c.hkv, f"{name} {mut}: K {k.tolist()}"
        if c.rot_q:
            q = rr.changed(e.q, e.qs, m.q, m.qs, c_used).sum(-1)
            assert int((q < need).sum()) <= keep * c.hq, f"{name} {mut}: q {q.tolist()}"
    # a neighbouring token's slot: every written cache row holds another token, or is written where none was
    m = rr.rope_expected(name, slot_shift=1)
    k, v = kv_moved(m)
    assert int(k.min()) >= need and int(v.min()) >= need, f"{name} token slot: {k.tolist()} {v.tolist()}"
    if c.hkv > 1:
        k, v = kv_moved(rr.rope_expected(name, head_shift=1))
        assert int(k.min()) >= need and int(v.min()) >= need, f"{name} head slot: {k.tolist()} {v.tolist()}"
    if c.scaled:
        # the scale on the untouched q (rot_q = False): every head of every token whose scale is not 1 moves
        m = rr.rope_expected(name, scale_q=True)
        assert torch.equal(e.q, i.rows.double()[:, : c.hq * c.d].view(rr.ROPE_TOKENS, c.hq, c.d))
        assert torch.equal(m.q, e.q * i.r.double()[:, None, None])
        moved = (rr.rne_bf16(m.q) != rr.rne_bf16(e.q)).sum(-1)[i.r != 1]
        assert moved.numel() >= c.hq and int(moved.min()) >= need, f"{name} q scaled: {moved.tolist()}"
        _, v = kv_moved(rr.rope_expected(name, unscaled_v=True))
        sel = (i.r != 1)[i.slots >= 0]
        assert bool(sel.any())
        if not e.v_exact:
            lo, hi = rr.bracket(e.v[wr], e.v[wr].abs(), rr.C_V)
            assert float((lo != hi).double().mean()) <= rr.UNDECIDED_CAP, f"{name} V"
        assert int(v.min()) >= 0 and int((v >= need).sum()) >= int(sel.sum()) * c.hkv, f"{name} v unscaled: {v.tolist()}"
    if c.sk:
        for slabs in [tuple(s for s in range(c.sk) if s != d) for d in range(c.sk)] + \
                     [tuple(range(c.sk)) + (d,) for d in range(c.sk)]:
            m = rr.rope_expected(name, slabs=slabs)
            k, v = kv_moved(m)
            q = (rr.rne_bf16(m.q) != rr.rne_bf16(e.q)).sum(-1)
            assert int(k.min()) >= need and int(v.min()) >= need and int(q.min()) >= need, f"{name} slabs {slabs}"


# ---------------------------------------------------------------------------------------------- movers, coverage

@pytest.mark.parametrize("name", list(rr.MOVER_CASES))
def test_mover_case(name):
    c = rr.MOVER_CASES[name]
    pool = rr.mover_pool(name)
    assert bool(torch.isfinite(pool.float()).all())
    chunks = rr.bits(pool).view(-1, 8)[:, 0]
    assert chunks.unique().numel() == chunks.numel() or c.planes * c.blocks * c.slab > 32000
    srcs, dsts = [p[0] for p in rr.COPY_PAIRS], [p[1] for p in rr.COPY_PAIRS]
    assert not set(srcs) & set(dsts) and {0, c.blocks - 1} <= set(srcs + dsts)
    cp = rr.copied(pool, rr.COPY_PAIRS)
    for s, d in rr.COPY_PAIRS:
        assert torch.equal(cp[:, d], pool[:, s]) and not torch.equal(pool[:, d], pool[:, s])
    for ids in rr.MOVE_IDS:
        assert len(set(ids)) == len(ids) and {0, c.blocks - 1} <= set(ids)
        buf = rr.gathered(pool, ids)
        assert buf.shape == (len(ids), c.planes, c.slab)
        for n, b in enumerate(ids):
            for p in range(c.planes):
                assert torch.equal(buf[n, p], pool[p, b])
        blank = torch.zeros_like(pool)
        back = rr.scattered(blank, ids, buf)
        assert torch.equal(back[:, list(ids)], pool[:, list(ids)])
        rest = [b for b in range(c.blocks) if b not in ids]
        assert not rest or not bool(back[:, rest].any())
        # a neighbouring id is visible
        assert not torch.equal(rr.gathered(pool, [(b + 1) % c.blocks for b in ids]), buf)
    assert sorted(rr.MOVE_IDS[1]) == list(range(c.blocks))
    assert c.slab == 8 or (c.slab // 8 > 256 and (c.slab // 8) % 256)


def test_coverage():
    by_nc = {}
    for name in rr.NORM_CASES:
        c = rr.ROW_CASES[name]
        by_nc.setdefault(rr.nc_of(c.hidden), []).append(c)
    assert sorted(by_nc) == list(range(1, 9))
    for nc, cs in by_nc.items():
        hs = {c.hidden for c in cs}
        assert {2048 * (nc - 1) + 8, 2048 * (nc - 1) + 16, 2048 * nc} <= hs
        assert {c.rows for c in cs} == {1, 3} and {c.sk for c in cs} == {1, 2, 5} and {c.strided for c in cs} == {True, False}
        assert {c.family for c in cs} == set(rr.FAMILIES)
    assert 8 in {rr.ROW_CASES[n].hidden for n in rr.NORM_CASES}
    rs_nc = {}
    for name in rr.RS_CASES:
        c = rr.ROW_CASES[name]
        rs_nc.setdefault(rr.nc_of(c.hidden), []).append(c)
    assert sorted(rs_nc) == [1, 2, 3, 4]
    for nc, cs in rs_nc.items():
        assert {2048 * (nc - 1) + 8, 2048 * (nc - 1) + 16, 2048 * nc} <= {c.hidden for c in cs}
        assert {c.rows for c in cs} == {1, 3} and {c.strided for c in cs} == {True, False}
        assert {c.family for c in cs} == set(rr.FAMILIES)
    assert rr.nc_of(rr.NORM_REFUSED_HIDDEN) == 9 and rr.nc_of(rr.RS_REFUSED_HIDDEN) == 5
    assert {(rr.ROW_CASES[n].hidden, rr.ROW_CASES[n].rows) for n in rr.SUMSQ_CASES} == \
        {(h, r) for h in (8, 2040, 2048, 2056, 8192) for r in (1, 7, 128)}
    assert rr.SUMSQ_REFUSED_ROWS == rr.SSP_LD + 1
    # SiLU: every chunks-per-lane count at every size, every family wherever it fits, two workgroups per row
    for inter in rr.SILU_INTERS:
        for per in range(9):
            fams = {c.family for c in rr.SILU_ALL if c.inter == inter and c.per == per}
            assert fams == ({"random"} if inter < 2040 else {"random", "ladder", "ladder_rs"})
    assert set(rr.SILU_INTERS) >= {8, 2040, 2048, 2056} and any(256 < i // 8 <= 512 for i in rr.SILU_INTERS)
    assert {c.scaled for c in rr.SILU_ALL if c.family == "random"} == {True, False}
    # RoPE: both head sizes of both kernels, every head pair, block size, family; items below, at, above one pass
    for slab in (False, True):
        cs = [c for c in rr.ROPE_ALL if bool(c.sk) == slab]
        assert {(c.d, c.hq, c.hkv, c.block_size, c.family) for c in cs} == \
            {(d, hq, hkv, bs, f) for d in (64, 128) for hq, hkv in rr.ROPE_HEADS for bs in (16, 32)
             for f in ("exact", "real")}
        for d in (64, 128):
            items = {rr.rope_items(d, c.hq, c.hkv, c.rot_q) for c in cs if c.d == d}
            assert min(items) < 256 < max(items) or d == 64
        assert 256 in {rr.rope_items(c.d, c.hq, c.hkv, c.rot_q) for c in cs}
    assert {c.sk for c in rr.ROPE_ALL} == {0, 1, 2, 5}
    plain = [c for c in rr.ROPE_ALL if not c.sk]
    assert {(c.rot_q, c.scaled) for c in plain} == {(True, False), (False, False), (False, True)}
    assert {c.wide for c in plain} == {True, False}
    assert {(1, 1), (8, 1), (4, 4), (32, 8)} <= set(rr.ROPE_HEADS)
    assert {(c.planes, c.slab) for c in rr.MOVER_ALL} == {(p, s) for p in (1, 6) for s in (8, 2400)}
