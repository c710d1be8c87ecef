"""tests/moe_reference.py judged on the CPU, before test_moe_kernel_gpu.py judges the kernels of
csrc/kernels/moe.hip by it: the exactness premises of every exact case, and for every case by name the mutations it
claims (moe_reference.CLAIMS): each has to move the expectation beyond tolerance in at least MIN_CHANGED rows or
elements, in all of them where the case holds fewer. The align checker has to reject hand-made wrong answers, and
ref.topk_softmax (the CPU fallback) has to choose as the oracle does."""

import pytest
import torch

from src.ops import reference as ref
from tests import moe_reference as mr
from tests import rowwise_reference as rr


# ---------------------------------------------------------------------------------------------- the lists themselves

def test_case_lists_cover_what_they_name():
    tk = mr.TOPK_ALL
    assert {c.t for c in tk} == set(mr.TOPK_T) and {c.e for c in tk} == set(mr.TOPK_E)
    for e in mr.TOPK_E:
        assert {c.k for c in tk if c.e == e} == {1, min(2, e), min(e, 8), e}
    for fam in mr.TOPK_FAMILIES:
        sub = [c for c in tk if c.family == fam]
        assert {c.t for c in sub} == set(mr.TOPK_T) and {c.renorm for c in sub} == {False, True}
        assert {c.e for c in sub} == set(mr.TOPK_E)
    rt = mr.ROUTE_ALL
    assert {c.t for c in rt} == set(mr.ROUTE_T) and {c.h for c in rt} == set(mr.ROUTE_H)
    for h in mr.ROUTE_H:
        for e in mr.ROUTE_E:
            sub = [c for c in rt if c.h == h and c.e == e]
            assert {c.k for c in sub} == {1, min(2, e), e}
    for e in mr.ROUTE_E:
        sub = [c for c in rt if c.e == e]
        assert {c.renorm for c in sub} == {False, True} and {c.t for c in sub} == set(mr.ROUTE_T)
    for h in mr.ROUTE_H:
        for em in (8, 16):
            assert {c.strided for c in rt if c.t == 3 and c.h == h and mr.route_em(c.e) == em} == {False, True}
    assert {c.gen for c in rt if c.h > 8} == {"designed"}
    f = mr.ROUTE_FALLBACK
    assert f.t > mr.ROUTE_MAX_T and f.gen == "random"
    cb = mr.COMBINE_ALL
    assert {c.t for c in cb} >= set(mr.COMBINE_T) and {c.k for c in cb} == set(mr.COMBINE_K)
    assert {(c.k, c.h) for c in cb if c.family == "exact"} >= {(k, h) for k in mr.COMBINE_K for h in mr.COMBINE_H}
    assert {c.strided for c in cb} == {False, True} and {c.family for c in cb} == {"exact", "random"}
    for c in cb:
        i = mr.combine_inputs(c.name)
        n = c.t * c.k
        assert torch.equal(i.pos.long().sort().values, torch.arange(n))
        assert n == 1 or not bool((i.pos.long() == torch.arange(n)).any()), "pos: a permutation without a fixed point"
    al = mr.ALIGN_ALL
    assert {c.n for c in al} == set(mr.ALIGN_N) and {c.e for c in al} == set(mr.ALIGN_E)
    assert {c.dist for c in al} == set(mr.ALIGN_DISTS)


def test_every_mutation_is_claimed_widely():
    """The rules in claims_of() leave no mutation to a handful of cases."""
    def share(cases, m):
        return sum(m in mr.CLAIMS[c.name] for c in cases) / len(cases)
    rt = [c for c in mr.ROUTE_ALL if c.e >= 2]
    assert share(rt, "drop") >= 0.9 and share(rt, "tie_high") >= 0.9
    assert share([c for c in rt if c.k >= 2 and c.e >= 3], "index_order") >= 0.9
    assert share([c for c in mr.ROUTE_ALL if c.k < c.e], "renorm_skipped") >= 0.3
    assert share([c for c in mr.ROUTE_ALL if c.k < c.e], "renorm_applied") >= 0.3
    assert share([c for c in mr.ROUTE_ALL if c.e in (1, 7, 9)], "leak") >= 0.6
    for e in (7, 9):        # both kernels' padded rows, with and without renormalisation
        assert {c.renorm for c in mr.ROUTE_ALL if c.e == e and "leak" in mr.CLAIMS[c.name]} == {False, True}
    assert all(m in mr.CLAIMS[mr.ROUTE_FALLBACK.name] for m in ("drop", "tie_high", "index_order", "renorm_skipped"))
    for t in mr.TOPK_T:
        for words in (range(1, 65), range(65, 129), range(129, 257)):      # the words of the kernel's taken set
            sub = [c for c in mr.TOPK_ALL if c.t == t or c.e in words]
            assert any("tie_high" in mr.CLAIMS[c.name] for c in sub)
            assert any("index_order" in mr.CLAIMS[c.name] for c in sub)
    for c in mr.COMBINE_ALL:
        assert {"drop", "double"} <= set(mr.CLAIMS[c.name])


# ---------------------------------------------------------------------------------------------- exactness

@pytest.mark.parametrize("name", [c.name for c in mr.ROUTE_ALL + [mr.ROUTE_FALLBACK]]
                         + [c.name for c in mr.COMBINE_ALL if c.family == "exact"])
def test_conditions(name):
    mr.conditions(name)


@pytest.mark.parametrize("name", mr.ROUTE_FUSED_CASES)
def test_route_fp32_sums_are_exact_in_any_order(name):
    """fp32 arithmetic in two very different orders reproduces the float64 logits bit for bit."""
    i = mr.route_inputs(name)
    want = mr.route_logits(i.x, i.wg)
    x, wg = i.x.float(), i.wg.float()
    fwd = (x[:, None, :] * wg[None]).cumsum(-1)[..., -1]
    rev = (x[:, None, :] * wg[None]).flip(-1).view(x.shape[0], wg.shape[0], -1, 8).sum(-1).sum(-1)
    for got in (fwd, rev):
        assert torch.equal(got.to(torch.bfloat16).double(), want)


@pytest.mark.parametrize("name", [c.name for c in mr.ROUTE_ALL if c.gen == "designed"])
def test_designed_route_rows_decide_a_tie(name):
    c = mr.ROUTE_CASES[name]
    i = mr.route_inputs(name)
    g = mr.route_logits(i.x, i.wg)
    e = mr.route_expected(name)
    if c.e >= 2:
        srt = g.sort(-1, descending=True).values
        cut = 0 if c.k == 1 else (c.k - 1 if c.k < c.e else c.e - 2)
        assert bool((srt[:, cut] == srt[:, cut + 1]).all()), "every row ties where the rule has to decide"
    if c.k >= 2 and c.e >= 3:
        assert bool((e.ids[:, 0] > e.ids[:, 1]).all())
    if c.t == 3 and c.e >= 2:
        assert len({tuple(r.tolist()) for r in g}) == 3, "the rows have logits of their own"


# ---------------------------------------------------------------------------------------------- oracles vs plain forms

def test_topk_oracle_equals_plain_softmax_where_nothing_ties():
    g = torch.randn(64, 8, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    g = g[[len(set(r.tolist())) == 8 for r in g]]
    assert g.shape[0] >= 32
    for renorm in (False, True):
        e = mr.topk(g, 2, renorm)
        p = torch.softmax(g.double(), -1)
        w, ids = torch.topk(p, 2, -1)
        if renorm:
            w = w / w.sum(-1, keepdim=True)
        assert torch.equal(e.ids.long(), ids) and torch.allclose(e.w, w, rtol=1e-14, atol=0)
        assert float((e.tol / e.w).max()) < 4e-6, "Mixtral-sized rows: a few fp32 ulp"


def test_weight_constant_as_documented():
    """E = 8, K = 2, all logits equal (d = 0): c = 0.5 * 7 + 4.5 = 8 without, 0.5 + 9.5 = 10 with renormalisation."""
    g = torch.zeros(1, 8, dtype=torch.bfloat16)
    assert torch.equal(mr.topk(g, 2, False).c, torch.full((1, 2), 8.0, dtype=torch.float64))
    assert torch.equal(mr.topk(g, 2, True).c, torch.full((1, 2), 10.0, dtype=torch.float64))


def test_topk_rule_on_hand_rows():
    g = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0],
                      [-mr.INF, 0.0, -mr.INF, -mr.INF, -mr.INF],
                      [-mr.INF] * 5]).to(torch.bfloat16)
    e = mr.topk(g, 3, False)
    assert e.ids.tolist() == [[1, 2, 4], [1, 0, 2], [0, 1, 2]]
    assert e.w[1].tolist() == [1.0, 0.0, 0.0] and bool(torch.isnan(e.w[2]).all())
    assert mr.topk(g, 3, False, tie="high").ids.tolist()[0] == [4, 2, 1]
    assert mr.topk(g[:1], 4, False, order="index").ids.tolist() == [[1, 2, 3, 4]]


@pytest.mark.parametrize("name", [c.name for c in mr.TOPK_ALL if c.family in ("tied", "nonfinite")])
def test_cpu_fallback_chooses_as_the_oracle(name):
    c = mr.TOPK_CASES[name]
    g = mr.topk_inputs(name)
    e = mr.topk_expected(name)
    w, ids = ref.topk_softmax(g, c.k, c.renorm)
    assert ids.dtype == torch.int32
    j = mr.judge_routing(ids, w, e, c.e)
    assert not [m for m in j.errs if not m.startswith("weights")], j.errs
    fin = torch.isfinite(e.w).all(-1)
    assert torch.allclose(w[fin].double(), e.w[fin], rtol=1e-5, atol=1e-37)      # fp32 torch arithmetic


def test_judge_routing_rejects_wrong_answers():
    name = next(c.name for c in mr.TOPK_ALL if c.family == "nonfinite" and c.t >= 255 and c.e == 8 and c.k == 2)
    e = mr.topk_expected(name)
    ok = mr.judge_routing(e.ids, e.w.float(), e, 8)
    assert ok.errs == [] and ok.ratio < 1
    ids = e.ids.clone()
    nan_row = int(e.nan_row.nonzero()[0])
    ids[nan_row] = -1
    assert any("outside" in m for m in mr.judge_routing(ids, e.w.float(), e, 8).errs)
    ids = e.ids.clone()
    ids[nan_row] = ids[nan_row, 0]
    assert any("repeat" in m for m in mr.judge_routing(ids, e.w.float(), e, 8).errs)
    ids = e.ids.clone()
    clean = int((~e.nan_row).nonzero()[0])
    ids[clean] = ids[clean].flip(0)
    assert any("differ" in m for m in mr.judge_routing(ids, e.w.float(), e, 8).errs)
    w = e.w.clone()
    fin = int(torch.isfinite(e.w).all(-1).nonzero()[0])
    w[fin, 0] = w[fin, 0] * (1 + 1e-4) + 1e-30
    assert any("weights" in m for m in mr.judge_routing(e.ids, w.float(), e, 8).errs)


# ---------------------------------------------------------------------------------------------- mutations

@pytest.mark.parametrize("name", [c.name for c in mr.TOPK_ALL if mr.CLAIMS[c.name]])
def test_topk_mutations_change_the_expectation(name):
    e = mr.topk_expected(name)
    for m in mr.CLAIMS[name]:
        ch = mr.rows_changed(e, mr.topk_expected(name, **mr.ROUTING_MUTATIONS[m]))
        assert mr.enough(ch), f"{name}: {m} changes {int(ch.sum())} of {ch.numel()} rows"


@pytest.mark.parametrize("name", [c.name for c in mr.ROUTE_ALL + [mr.ROUTE_FALLBACK] if mr.CLAIMS[c.name]])
def test_route_mutations_change_the_expectation(name):
    e = mr.route_expected(name)
    for m in mr.CLAIMS[name]:
        ch = mr.rows_changed(e, mr.route_expected(name, **mr.ROUTING_MUTATIONS[m]))
        assert mr.enough(ch), f"{name}: {m} changes {int(ch.sum())} of {ch.numel()} rows"


@pytest.mark.parametrize("name", [c.name for c in mr.COMBINE_ALL])
def test_combine_mutations_change_the_expectation(name):
    c = mr.COMBINE_CASES[name]
    for residual in (False, True):
        e = mr.combine_expected(name, residual)
        for m in mr.CLAIMS[name]:
            mu = mr.combine_expected(name, residual, **{m: True})
            if m == "unrounded":
                if not residual:
                    continue
                ch = (e.ss - mu.ss).abs() > e.ss_tol + mu.ss_tol
            else:
                ch = mr.elements_changed(e, mu)
                if m in ("shift_pos", "shift_w"):       # a neighbour's term can agree in single elements
                    ch = ch.any(-1) if e.exact else ch.sum(-1) >= min(mr.MIN_CHANGED, c.h)
                elif not e.exact:                       # undecided elements (<= 1 %) cannot count
                    ch = ch.sum(-1) >= 0.9 * c.h
            assert mr.enough(ch), f"{name} residual={residual}: {m} changes {int(ch.sum())} of {ch.numel()}"
        if not e.exact:
            assert float((rr.bracket(e.o, e.s, e.c)[0] != rr.bracket(e.o, e.s, e.c)[1]).double().mean()) \
                <= rr.UNDECIDED_CAP


def test_combine_exact_equals_fp32_in_kernel_order():
    """fp32, term by term from 0 (resp. from resid) as the kernels add, equals the float64 oracle bit for bit."""
    for name in ("combine-t5-k8-h4104-exact", "combine-t5-k2-h8-exact", "combine-t128-k2-h2048-exact"):
        i = mr.combine_inputs(name)
        c = i.c
        for residual in (False, True):
            acc = i.resid.float().clone() if residual else torch.zeros(c.t, c.h)
            pos = i.pos.long().view(c.t, c.k)
            for k in range(c.k):
                acc = acc + i.w[:, k, None] * i.ys.float()[pos[:, k]]
            e = mr.combine_expected(name, residual)
            assert torch.equal(acc.to(torch.bfloat16).double(), e.h)
            assert torch.equal(acc.to(torch.bfloat16).float().pow(2).sum(-1).double(), e.ss)


@pytest.mark.parametrize("name", [c.name for c in mr.GATHER_ALL])
def test_gather_index_mutation(name):
    i = mr.gather_inputs(name)
    c = i.c
    srt = i.sorted if i.sorted is not None else mr.align_model(i.ids, mr.GATHER_E)[1]
    assert torch.equal(srt.long().sort().values, torch.arange(mr.GATHER_T * c.k))
    want, mut = mr.gathered(i.x, srt, c.k), mr.gathered(i.x, srt, c.k, mod=True)
    assert mr.enough((rr.bits(want) != rr.bits(mut)).any(-1))
    assert len({tuple(r.tolist()) for r in rr.bits(i.x)[:, :8]}) == mr.GATHER_T, "every row's first chunk is its own"


# ---------------------------------------------------------------------------------------------- align

@pytest.mark.parametrize("name", [c.name for c in mr.ALIGN_ALL])
def test_align_checker(name):
    c = mr.ALIGN_CASES[name]
    ids = mr.align_ids(name)
    assert ids.numel() == c.n and (c.n == 0 or (0 <= int(ids.min()) and int(ids.max()) < c.e))
    if c.dist == "ends_empty" and c.n:
        assert int(ids.min()) >= 1 and int(ids.max()) <= c.e - 2
    if c.dist == "distinct":
        k = min(mr.ALIGN_K.get(c.n, 1), c.e)
        rows = ids.view(-1, k).sort(-1).values
        assert k == 1 or bool((rows[:, 1:] != rows[:, :-1]).all())
    off, srt, pos = mr.align_model(ids, c.e)
    assert mr.check_align(off, srt, pos, ids, c.e) == []
    # any order inside a group is as good
    if c.n > 2:
        rev = srt.clone()
        for e in range(c.e):
            rev[off[e]:off[e + 1]] = srt[off[e]:off[e + 1]].flip(0)
        p2 = torch.empty_like(pos)
        p2[rev.long()] = torch.arange(c.n, dtype=torch.int32)
        assert mr.check_align(off, rev, p2, ids, c.e) == []
    # hand-made wrong answers
    for e in {0, c.e // 2, c.e}:
        bad = off.clone()
        bad[e] += 1
        assert mr.check_align(bad, srt, pos, ids, c.e), "an offset off by one"
        bad[e] -= 2
        assert mr.check_align(bad, srt, pos, ids, c.e), "an offset off by one"
    if c.n >= 2:
        bad = pos.clone()
        bad[[0, 1]] = bad[[1, 0]]
        assert mr.check_align(off, srt, bad, ids, c.e), "a pos that is not the inverse"
        dup = srt.clone()
        dup[0] = dup[1]
        assert mr.check_align(off, dup, pos, ids, c.e), "sorted with a repeated entry"
    counts = torch.bincount(ids.long(), minlength=c.e)
    if int((counts > 0).sum()) >= 2:
        a, b = (counts > 0).nonzero().flatten()[[0, -1]].tolist()
        ja, jb = int(off[a]), int(off[b])
        sw, pw = srt.clone(), pos.clone()
        sw[[ja, jb]] = sw[[jb, ja]]
        pw[sw.long()] = torch.arange(c.n, dtype=torch.int32)          # pos stays the inverse: only the groups are wrong
        assert mr.check_align(off, sw, pw, ids, c.e) == ["an entry of sorted lies in another expert's range"]
