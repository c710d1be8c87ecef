"""The attention oracle and its inputs, before any kernel is judged by them (tests/attention_reference.py): the
oracle against the fp32 reference and against closed forms, the fused-prologue model against rope_and_cache +
attention, and, for every case of the GPU file's lists by name, the conditions on the inputs: removing one key set
moves the oracle by at least 4 tolerances (proved on the oracle, never on project code), and the tolerance is at
most a quarter of the 2.5e-2 the older attention tests allow."""

import pytest
import torch

from src.ops import reference as ref
from tests import attention_reference as ar

D = ar.D


@pytest.mark.parametrize("g", [1, 4, 8])
def test_oracle_matches_fp32_reference(g):
    """Ragged q lengths, cached prefixes (pos0 = 172, 936, 128, 135), G in {1, 4, 8}: the fp32 reference agrees to fp32
    accuracy (softmax and PV sums over <= 1,000 keys of magnitude <= 0.75)."""
    c = ar.case(f"random-pf-small-g{g}")
    e = c.expected()
    r = ref.attention(c.q.float(), c.kc.float(), c.vc.float(), c.bt, c.cu, torch.tensor(c.ctxs), c.hq, c.hkv, c.scale)
    assert r.dtype == torch.float32
    assert float((r.double() - e.o).abs().max()) < 2e-6
    assert float(e.slack.abs().max()) == 0 and torch.equal(e.tol, e.base)


@pytest.mark.parametrize("name", [n for n in ar.ALL_CASES if n.startswith(("flat", "staircase"))])
def test_closed_form(name):
    c = ar.case(name)
    assert float((c.expected().o - c.closed).abs().max()) <= 1e-12


def test_staircase_levels_cross_the_rescale_threshold():
    """A wave's consecutive tiles step by +9 (rescale), +7 (none) and -20; the highest level lies in the last three
    chunks, so with merged parts never in part 0."""
    for stride, ctx in ((4, 2048), (4, 1025), (1, 1000), (1, 700)):
        lv = ar.levels(ctx, stride)
        per_step = lv[:: 32 * stride]
        d = set((per_step[1:] - per_step[:-1]).tolist())
        assert d == {9, 7, -20}
        assert int(lv.argmax()) >= ctx - 3 * 32 * stride
        assert all(len(set(lv[i:i + 32].tolist())) == 1 for i in range(0, ctx, 32))


@pytest.mark.parametrize("name", ["random-b4x8+fused", "witness-b1x4+fused", "random-b1x4+fused-sk3-t256",
                                  "random-few+fused"])
def test_fused_oracle_matches_rope_and_cache(name):
    """The prologue model against ref.rope_and_cache + ref.attention on the same bf16-rounded qkv. The reference
    rounds qkv before it rotates (the kernel and the oracle after), so q and the new key differ by an ulp in many
    elements: the difference is within the all-elements slack."""
    c = ar.case(name)
    f, fs, e = c.fused, ar.fused_step(c), c.expected()
    qkv = ar.bf(f.slab.double().sum(0) * ar._row_scale(f.ssp, c.n)[:, None])
    ka, va = f.kc0.clone(), f.vc0.clone()
    ref.rope_and_cache(qkv, f.pos, f.cs, f.real, ka, va, c.hq, c.hkv, D)
    r = ref.attention(qkv[:, : c.hq * D].float(), ka.float(), va.float(), c.bt, c.cu, torch.tensor(c.ctxs), c.hq,
                      c.hkv, c.scale)
    assert bool(((r.double() - e.o).abs() <= e.slack + 1e-5).all())
    dq = (qkv[:, : c.hq * D].double() - fs.q.double()).abs()   # rope_and_cache rotated qkv's q columns in place
    assert float(dq.max()) <= 2.0 ** -6 * float(fs.q.double().abs().max()), "the two q differ by rounding only"
    # the caches: what the step attends to has every new token, what it leaves lacks the padded rows'
    pad = (f.slots < 0).nonzero().flatten().tolist()
    assert pad, "every fused case has a padded row"
    for i, slot in enumerate(f.real.tolist()):
        row_att, row_aft = fs.k_att[slot // 16, :, slot % 16], fs.k_after[slot // 16, :, slot % 16]
        assert bool(torch.isfinite(row_att.float()).all()) and not bool((row_att.float() == ar.STALE_K).all())
        assert bool((row_aft.float() == ar.STALE_K).all()) == (i in pad)
    assert bool(torch.isnan(fs.k_after[c.poison].float()).all())


def test_rope_on_load_model():
    """rope_q against ref.apply_rope (fp32) on q_scale-scaled rows: equal up to one bf16 ulp, where they differ."""
    c = ar.case("random-pf-large-g4+cs+qs")
    q, moves = ar.rope_q(c)
    pos = torch.cat([torch.arange(ctx - ql, ctx) for ql, ctx in zip(c.qlens, c.ctxs)])
    r = ref.apply_rope((c.q.float() * c.q_scale[:, None]).reshape(-1, c.hq, D), pos, c.cs).reshape(-1, c.hq * D)
    assert float(((q.double() - r.double()).abs() / r.double().abs().clamp_min(1e-3)).max()) <= 2.0 ** -7
    assert 0 < int((moves > 0).sum()) < moves.numel() // 256   # a few elements sit on a midpoint, not many


@pytest.mark.parametrize("name", ["flat-b4x8", "witness-few", "staircase-multi4k", "flat-pf-small-g4",
                                  "witness-b1x4+fused"])
def test_leave_out_form_is_the_oracle_without_the_keys(name):
    """drop_ratios subtracts a key set's share from the sums; the same figure from a real second evaluation."""
    c = ar.case(name)
    e = c.expected()
    q, kc, vc = c.oracle_inputs()
    gen = torch.Generator().manual_seed(5)
    keep = [torch.rand(ctx, generator=gen) < 0.9 for ctx in c.ctxs]
    o2 = ar.oracle(q, kc, vc, c.bt, c.cu, c.ctxs, c.hq, c.hkv, c.scale, keep=keep)[0]
    for s in range(c.n):
        b0, b1 = int(c.cu[s]), int(c.cu[s + 1])
        want = float(((o2[b0:b1] - e.o[b0:b1]).abs() / e.tight[b0:b1]).max())
        got = ar.drop_ratios(c, s, sets=(~keep[s])[None])[0]
        assert abs(got - want) <= 1e-6 * max(1.0, want)
        j = c.ctxs[s] // 2   # the single-key path against the set path
        m = torch.zeros(c.ctxs[s], dtype=torch.bool)
        m[j] = True
        r = _first_row(c, s, [j])
        one = ar.drop_ratios(c, s, keys=[j], rows=r)[0]
        assert abs(one - ar.drop_ratios(c, s, sets=m[None], rows=[slice(r[0], r[0] + 1)])[0]) <= 1e-6 * max(1.0, one)


def _first_row(c, s, keys):
    pos0 = c.ctxs[s] - c.qlens[s]
    return [max(0, k - pos0) for k in keys]


@pytest.mark.parametrize("name", ar.ALL_CASES)
def test_inputs_make_every_key_count(name):
    """The conditions on the GPU inputs, case by case. flat: every single key, and (decode) every aligned run of C
    chunks for C = 1 .. maxp, which are all the parts any chunks-per-part choice of the launcher could cut;
    witness: each witness key, which also holds >= 1 / (4 |W|) of its row's weight; staircase: each top-level tile.
    Removing the set moves some element by >= 4 tol (the tighter of the two tolerances the GPU test asserts). A key
    of a prefill case is judged on the first q row that sees it. And tol, before the slack of the fused paths, is
    <= 2.5e-2 / 4 wherever |o| <= 1."""
    c = ar.case(name)
    e = c.expected()
    assert bool(torch.isfinite(e.o).all()) and bool(torch.isfinite(e.tol).all())
    assert bool((e.base[e.o.abs() <= 1] <= 2.5e-2 / 4).all())
    assert bool((e.tight <= e.tol + 1e-12).all())
    fam = c.family
    if fam == "random":
        return
    worst = float("inf")
    for s in range(c.n):
        ctx, qlen = c.ctxs[s], c.qlens[s]
        if fam == "flat":
            keys = list(range(ctx))
            worst = min([worst] + ar.drop_ratios(c, s, keys=keys, rows=_first_row(c, s, keys)))
            if qlen == 1:
                nch = (ctx + 127) // 128
                maxp = (c.max_ctx + 127) // 128
                ch = torch.arange(ctx) // 128
                sets = [(ch >= p * cc) & (ch < (p + 1) * cc) for cc in range(1, maxp + 1)
                        for p in range((nch + cc - 1) // cc)]
                worst = min([worst] + ar.drop_ratios(c, s, sets=sets))
        elif fam == "witness":
            w = c.witnesses[s]
            rows = _first_row(c, s, w)
            worst = min([worst] + ar.drop_ratios(c, s, keys=w, rows=rows))
            q, kc, vc = c.oracle_inputs()
            b0 = int(c.cu[s])
            ee = ar._terms(q[b0:b0 + qlen, : c.hq * D], kc, vc, c.bt[s], qlen, ctx, c.hq, c.hkv, c.scale)[0]
            p = ee / ee.sum(-1, keepdim=True)
            assert float(p[:, rows, w].min()) >= 1 / (4 * len(w)), (name, s)
        else:
            tiles = ar.top_tiles(ctx, c.stride)
            worst = min([worst] + ar.drop_ratios(c, s, sets=tiles, rows=[slice(qlen - 1, qlen)] * len(tiles)))
    print(f"{name}: least |delta o| / tol over the key sets = {worst:.2f}")
    assert worst >= 4, name


def test_lists_cover_what_the_kernels_branch_on():
    """The shapes the lists promise: the few-pair contexts give 2, 8, 9 and 16 one-chunk parts (the merge's batches
    of 8 run full, one over, and twice); the two prefill sizes sit on both sides of the launcher's 256-token
    threshold; pos0 = 443 is off the 32- and 64-key grids; fused variants cover odd slab-row counts at G = 1."""
    assert [(x + 127) // 128 for x in ar.DECODE_CONFIGS["few"][2]] == [2, 8, 9, 16]
    small, large = ar.case("flat-pf-small-g1"), ar.case("flat-pf-large-g1")
    assert small.max_q_len == 256
    assert large.max_q_len == 257
    assert (700 - 257) % 32 and (700 - 257) % 64
    assert {(cfg, sk) for cfg, sk, _ in ar.FUSED_VARIANTS} >= {("b1x4", 1), ("b1x4", 3)}
    assert {t for _, _, t in ar.FUSED_VARIANTS} | {4} == {4, 130, 256}
    assert max(ar.BATCH32) == 777 and len(ar.BATCH32) == 32 and min(ar.BATCH32) >= 2
    assert len(set(ar.AMPS)) == len(ar.AMPS) >= 256
    assert all(float(torch.tensor(a).to(torch.bfloat16)) == a for a in ar.AMPS)
