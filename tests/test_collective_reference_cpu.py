"""The oracle of tests/collective_reference.py before a kernel is judged by it (no GPU): it equals a plain fp32 torch
reference on the random family and closed forms on `own` and `order`; for every call of the GPU test's plan, by name
and for 2, 4 and 8 ranks, the premise of its family holds and every mutation the case claims changes at least 8
elements (or all of a smaller case), a statistic by more than 4 times its tolerance; the lists cover both parities
of every kernel, flag slots 0 and 255, one and several passes of the 512-thread loop, both activation images, both
ring forms and sk 1 and 2."""

import pytest
import torch

from tests import collective_reference as cr
from tests import gemm_decode_reference as gr

ALL = [c.name for c, _ in cr.PLAN]


def _fp32_sum(xs):
    s = torch.zeros(xs.shape[1:], dtype=torch.float32)
    for p in range(xs.shape[0]):
        s = s + xs[p].float()
    return s


@pytest.mark.parametrize("world", cr.WORLDS)
def test_oracle_equals_fp32_reference_on_random(world):
    sim = cr.simulate(world)
    seen = set()
    for name, st in sim.items():
        c = st.c
        if c.family != "random" or c.kind == "gemm":
            continue
        seen.add(c.kind)
        if c.kind == "gat":
            assert torch.equal(cr.bits(st.exp.out), cr.bits(torch.cat(list(st.i.xs), -1)))
            continue
        s = _fp32_sum(st.i.xs)
        if c.kind == "ar":
            assert torch.equal(st.exp.out.to(torch.bfloat16), s.to(torch.bfloat16)), name
        else:
            h = (st.i.resid.float() + s.to(torch.bfloat16).float()).to(torch.bfloat16)
            assert torch.equal(st.exp.out.to(torch.bfloat16), h), name
            ss = h.float().pow(2).sum(-1).double()
            assert bool(((st.exp.ss - ss).abs() <= cr.ss_bound(st.exp.ss, c.hidden)).all()), name
    assert seen == {"ar", "res", "gat"}


@pytest.mark.parametrize("world", cr.WORLDS)
def test_random_gemm_against_fp32_reference(world):
    st = cr.simulate(world)["gemm-64x128-m19-s2-row-n16-random"]
    c = st.c
    y = torch.stack([(st.i.xs[p].float() @ st.i.ws[p].float().T).to(torch.bfloat16) for p in range(world)])
    h = (st.resid.float() + _fp32_sum(y).to(torch.bfloat16).float()).to(torch.bfloat16).double()
    lo, hi = cr.random_gemm_bracket(st)
    assert bool(((h >= lo) & (h <= hi)).all())
    # the worst-case bound leaves many elements undecided (a quarter at 2 ranks, more at 8); every row still has
    # elements that are decided bit for bit, and the mutation checks count only those
    print("undecided share", float((lo != hi).double().mean()))
    assert int((lo == hi).sum(-1).min()) >= cr.MIN_CHANGED
    assert bool(((st.exp.out >= lo) & (st.exp.out <= hi)).all())


@pytest.mark.parametrize("world", cr.WORLDS)
def test_closed_forms(world):
    sim = cr.simulate(world)
    for name, st in sim.items():
        c = st.c
        if c.kind != "ar":
            continue
        if c.family == "own":       # (2^W - 1) times rank 0's value, exactly
            assert torch.equal(st.exp.out, st.msgs[0] * (2 ** world - 1)), name
        if c.family == "order":     # the small term survives: the largest magnitude times 2^-26 (W = 2: 2.5 x_0)
            want = st.msgs[0] * 2.5 if world == 2 else st.msgs.sum(0)
            assert torch.equal(st.exp.out, want), name
            if world > 2:
                assert torch.equal(st.exp.out.abs(), st.msgs.abs().max(0).values * 2.0 ** -26), name


def test_rounding_helpers():
    v = torch.tensor([257.0, 259.0, 256.5, 257.5, 258.5, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -257.0, 3e-40],
                     dtype=torch.float64)
    assert torch.equal(cr.bf16(v), v.to(torch.bfloat16).double())
    r = torch.randn(4096, dtype=torch.float64) * 100
    assert torch.equal(cr.bf16(cr.f32(r)), r.float().to(torch.bfloat16).double())
    assert cr.bf16(torch.tensor([257.0], dtype=torch.float64)).item() == 256.0
    assert cr.bf16(torch.tensor([259.0], dtype=torch.float64)).item() == 260.0
    assert cr.f32(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64)).item() == 2.0 ** 24


@pytest.mark.parametrize("world", cr.WORLDS)
@pytest.mark.parametrize("name", ALL)
def test_premise(name, world):
    cr.premise(name, world)


def _changed(c, st, e, m):
    """(changed elements of the output, changed statistics) of mutated expectation m against e."""
    if c.kind == "gat":
        return int((cr.bits(e.out) != cr.bits(m.out)).sum()), 0
    if c.kind == "gemm" and c.family == "random":
        lo, hi = cr.random_gemm_bracket(st)
        out = int(((lo == hi) & (m.out != lo)).sum())
    else:
        out = int((e.out != m.out).sum())
    ss = 0
    if e.ss is not None:
        if c.family == "exact":
            tol = torch.zeros_like(e.ss)
        else:
            tol = cr.ss_bound(e.ss, c.hidden) if c.kind == "res" else cr.gemm_ss_bound(e.ss, c.wr)
        ss = int(((e.ss - m.ss).abs() > 4 * tol).sum())
    return out, ss


@pytest.mark.parametrize("world", cr.WORLDS)
@pytest.mark.parametrize("name", ALL)
def test_claimed_mutations_move_the_expectation(name, world):
    st = cr.simulate(world)[name]
    c = st.c
    for mut in cr.claims(c, world):
        assert mut in cr.MUTATIONS
        for who in (range(world) if mut in ("drop", "double") else (0,)):
            m = cr.evaluate(name, world, st, mut, who=who)
            out, ss = _changed(c, st, st.exp, m)
            if mut.startswith("ss_"):
                nstat = st.exp.ss.numel() - (st.exp.ss.shape[0] if mut == "ss_next_row" and c.kind == "gemm" else 0)
                assert ss >= min(cr.MIN_CHANGED, nstat), (name, mut, ss)
                continue
            need = min(cr.MIN_CHANGED, c.wr if mut == "clamp_row" else c.n)
            assert out >= need, (name, world, mut, who, out)
            if st.exp.ss is not None and mut in ("drop", "double", "no_mid_round", "partial_unrounded"):
                assert ss >= 1, (name, mut, "the statistic does not notice")


def test_every_listed_mutation_is_claimed_somewhere():
    claimed = {m for w in cr.WORLDS for c, _ in cr.plan(w) for m in cr.claims(c, w)}
    assert claimed == set(cr.MUTATIONS)
    # and, kernel by kernel, the changes the issue names: the reversed rank loop (ar, res), the own rank read from the
    # other half (every kind), the rounding before the residual add (res, gemm), statistics before the rounding
    # (res, gemm), the gather's row with cvec + 1, the rounding before the exchange (gemm)
    by = {}
    for c, _ in cr.plan(8):
        by.setdefault(c.kind, set()).update(cr.claims(c, 8))
    assert all("own_other_half" in v for v in by.values())
    assert {"reversed", "other_half", "prev_stamp", "drop", "double", "neighbour"} <= by["ar"]
    assert {"reversed", "other_half", "no_mid_round", "ss_unrounded", "ss_drop_chunk", "ss_next_row"} <= by["res"]
    assert {"cvec_plus", "cvec_minus", "rank_minor", "other_half", "neighbour"} <= by["gat"]
    assert {"partial_unrounded", "no_mid_round", "neighbour_tile", "clamp_row", "other_half", "ss_unrounded"} <= by["gemm"]


def test_coverage():
    for world in cr.WORLDS:
        cov = cr.coverage(world)
        for kind, par in cov["parity"].items():
            assert par == {0, 1}, kind
        # the last flag slot a group sharing one GPU can reach (cr.RESIDENT): 255 at 2 ranks, 127 at 4, 63 at 8
        assert {0, min(256, cr.RESIDENT // world) - 1} <= cov["slots"]
        # trailing workgroups without a vector need per (grid - 1) >= nvec, which the launchers' 64 vectors per
        # workgroup allow from 66 workgroups on: out of reach of the 64 that 8 ranks on one GPU may use
        assert cov["passes"] == {1, 2} and cov["empty_wg"] == (cr.RESIDENT // world >= 66)
        assert cov["xr"] == {16, 32, 64}
        assert cov["ring"] == {False, True} and cov["sk"] == {1, 2} and cov["tiled"] == {False, True}
        assert all(c.grid * world <= cr.RESIDENT for c, _ in cr.plan(world))
    assert 255 in cr.coverage(2)["slots"]
    # parities per kernel again inside the sequences (the chain is odd, so passes alternate)
    seq = {}
    for c, e in cr.PLAN:
        if c.group == "seq":
            seq.setdefault(c.name.split("-", 2)[2], set()).add(e & 1)
    assert all(v == {0, 1} for v in seq.values()) and len(seq) == 5
    # the n == cap case fills the small object's half; every message fits its object
    assert all(any(c.n == cr.CAPS[c.obj] for c, _ in cr.plan(w)) for w in cr.WORLDS)
    # half-ring twins exist for both tiles and take their twin's inputs
    halves = [c for c, _ in cr.PLAN if c.half_ring]
    assert {c.wr for c in halves} == {32, 64}
    for c in halves:
        a, b = cr.inputs(c.name, 8), cr.inputs(c.twin, 8)
        assert torch.equal(a.xs, b.xs) and torch.equal(a.ws, b.ws) and torch.equal(a.resid, b.resid)
    # the residency rule of the fused exchange at 8 ranks on one 256-CU GPU
    from src.parallel.custom_allreduce import fused_exchange_ok
    assert all(fused_exchange_ok(c.ntiles, 0, 0, 8, 256) for c, _ in cr.PLAN if c.kind == "gemm")


def test_stamping_separates_calls():
    """Two calls never carry the same values, and what a call finds in the other staging half is the previous call's."""
    sim = cr.simulate(4)
    prev = {}
    for c, e in cr.PLAN:
        st = sim[c.name]
        if c.obj in prev and not c.twin:
            p = prev[c.obj]
            k = min(p.c.n, c.n)
            sent = (p.i.xs.float() if p.c.kind == "gat" else p.msgs.float()).reshape(4, -1)
            assert torch.equal(st.stale[:, :k], sent[:, :k]), c.name
        a, b = cr.inputs(c.name, 4), cr.inputs(c.name, 4, -1)
        assert not torch.equal(cr.bits(a.xs), cr.bits(b.xs)), c.name
        prev[c.obj] = st


def test_gemm_partial_reuses_the_decode_reference():
    c = cr.CASES["gemm-64x128-m17-s2-tile-n16-exact"] if "gemm-64x128-m17-s2-tile-n16-exact" in cr.CASES else \
        next(c for c, _ in cr.PLAN if c.kind == "gemm" and c.sk == 2 and c.family == "exact")
    i = cr.inputs(c.name, 2)
    y, _ = cr.gemm_partial(c, i.xs[0], i.ws[0])
    assert torch.equal(y, gr.partials(i.xs[0].double(), i.ws[0].double(), c.kc, c.sk).sum(0))
    assert torch.equal(y, i.xs[0].double() @ i.ws[0].double().T)
