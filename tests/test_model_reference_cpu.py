"""The model oracle (tests/model_reference.py) judged before any GPU path is judged by it: it equals the float64
reference path through the paged reference ops, folding is exact on the weight family, and for every GPU case by
name the tolerance stays under its cap and each mutation the case claims clears MUT_FACTOR x tol. For mixtral-tiny
also: every routing decision of every case is decided, the routing-weight tolerance has teeth, and the shards that
``load_state_dict`` cuts under tensor and expert parallelism follow the Megatron rule."""

import pytest
import torch

from tests import model_reference as mr

CASES = mr.cases()


def _scripts():
    """One representative case per distinct (arch, fold, script)."""
    seen, out = set(), []
    for name, c in CASES.items():
        key = mr._script_key(c.arch, c.script, c.fold)
        if key not in seen:
            seen.add(key)
            out.append(name)
    return out


@pytest.mark.parametrize("name", ["slab_prefill_128", "rowscale_chunked", "rowscale_keep", "norm_loop_129",
                                  "slab_decode_5", "moe_norm_128", "moe_chunked", "moe_keep", "moe_unfolded",
                                  "moe_fused_5_embed"])
def test_oracle_equals_the_float64_reference_path(name):
    """Ragged, chunked, kept-row and decode scripts: the oracle (lists, unfolded gains) against
    ``reference_copy("cpu", float64)`` through block tables and the paged reference ops, to 1e-12 per row; on
    mixtral-tiny with the identical expert sets and routing weights as well."""
    c = CASES[name]
    got = mr.run_paged(mr.reference_model(c.arch, c.fold, torch.float64), c.script)
    want = mr.oracle_taps(c.arch, c.script)
    assert mr.untouched(got)
    for tap, e in mr.row_errors(got, want, mr.arch_of(c.arch).num_layers).items():
        assert float(e.max()) < 1e-12, (name, tap, float(e.max()))
    if c.arch == "moe":
        for li in range(mr.arch_of(c.arch).num_layers):
            for g, w, gw, ww in zip(got.moe[f"route{li}"], want.moe[f"route{li}"], got.moe[f"rw{li}"],
                                    want.moe[f"rw{li}"]):
                assert torch.equal(g, w), (name, li)
                assert g.shape[0] == 0 or float((gw - ww).abs().max()) < 1e-12, (name, li)


@pytest.mark.parametrize("arch", ["tiny", "mini"])
def test_folding_is_exact_on_the_family(arch):
    """Gains are powers of two: the folded bf16 weights are the products exactly, and the float64 model on the
    folded weights (unit gains) equals the one on the family's own tensors to 0."""
    folded = mr.family_model(arch, "cpu", torch.bfloat16, fold=True)
    sd, w = mr.family_state_dict(arch), mr.family_weights(arch)
    assert folded.norms_folded and all(bool((lw.ln1 == 1).all() and (lw.ln2 == 1).all()) for lw in folded.layers)
    wf = mr.Weights.from_model(folded)
    for li, (a, b) in enumerate(zip(wf.layers, w.layers)):
        assert torch.equal(a["q"], b["q"] * b["ln1"][None, :]) and torch.equal(a["up"], b["up"] * b["ln2"][None, :])
    assert torch.equal(wf.lm_head, w.lm_head) and torch.equal(wf.embed, sd["model.embed_tokens.weight"].double())
    unfolded = mr.family_model(arch, "cpu", torch.bfloat16, fold=False)
    assert not unfolded.norms_folded  # gains still in the norms: the folded-only paths are off
    script = CASES["slab_decode_5"].script if arch == "tiny" else CASES["fused_mini_p13_on"].script
    a, b = mr.Oracle(wf).run(script), mr.oracle_taps(arch, script)
    for tap, e in mr.row_errors(a, b, w.arch.num_layers).items():
        assert float(e.max()) == 0.0, (tap, float(e.max()))


@pytest.mark.parametrize("arch,mode", [("tiny", "tp"), ("moe", "tp"), ("moe", "ep")])
@pytest.mark.parametrize("world", [2, 4])
def test_checkpoint_shards_follow_the_megatron_rule(arch, mode, world):
    """The W shards that ``load_state_dict`` alone cuts from the family (unfolded), put together again by the
    Megatron rule written out here, are the family's tensors bit for bit: q heads, o columns, gate / up rows, down
    columns and vocabulary rows in rank order; kv heads in rank order, or each replicated on W / kv ranks in a row;
    under expert parallelism whole experts [r E / W, (r + 1) E / W)."""
    from src.models.llama import CausalLM
    from src.parallel.tp import TPContext

    a, sd = mr.arch_of(arch), mr.family_state_dict(arch)
    d, nq, nkv, big, E = a.head_dim, a.num_heads, a.num_kv_heads, a.intermediate_size, a.num_experts
    ms = []
    for r in range(world):
        m = CausalLM(a, "cpu", dtype=torch.bfloat16, tp=TPContext(rank=r, world_size=world), seed=1,
                     max_position=mr.MAX_POS, moe_parallel=mode)
        skipped = a.num_layers * 3 * (E - E // world) if mode == "ep" else 0   # w1 / w3 / w2 of the other ranks' experts
        assert m.load_state_dict(sd, fold=False) == len(sd) - skipped
        ms.append(m)
    f = lambda t: t.float()  # noqa: E731  (bf16 numbers: exact)
    cat = lambda ts, dim=0: torch.cat([f(t) for t in ts], dim)  # noqa: E731
    hq, hkv = nq // world, max(1, nkv // world)
    assert [(m.hq, m.hkv) for m in ms] == [(hq, hkv)] * world
    assert torch.equal(cat([m.lm_head for m in ms]), sd["lm_head.weight"]) and ms[0].vocab_parallel
    for m in ms:
        assert torch.equal(f(m.embed), sd["model.embed_tokens.weight"]) and torch.equal(f(m.norm), sd["model.norm.weight"])
    for li in range(a.num_layers):
        p = f"model.layers.{li}."
        lws = [m.layers[li] for m in ms]
        for lw in lws:
            assert torch.equal(f(lw.ln1), sd[p + "input_layernorm.weight"])
            assert torch.equal(f(lw.ln2), sd[p + "post_attention_layernorm.weight"])
        assert torch.equal(cat([lw.qkv[: hq * d] for lw in lws]), sd[p + "self_attn.q_proj.weight"])
        assert torch.equal(cat([lw.o for lw in lws], 1), sd[p + "self_attn.o_proj.weight"])
        for name, lo in (("k_proj", hq * d), ("v_proj", (hq + hkv) * d)):
            full = sd[p + f"self_attn.{name}.weight"]
            parts = [lw.qkv[lo:lo + hkv * d] for lw in lws]
            if nkv >= world:
                assert torch.equal(cat(parts), full)
            else:  # head j on the ranks [j W / kv, (j + 1) W / kv): the rank's query heads are that head's group
                rep = world // nkv
                for r, part in enumerate(parts):
                    assert torch.equal(f(part), full[(r // rep) * d:(r // rep + 1) * d]), (name, r)
                    assert r * hq // (nq // nkv) == r // rep
        if not a.is_moe:
            i = big // world
            assert torch.equal(cat([lw.gate_up[:i] for lw in lws]), sd[p + "mlp.gate_proj.weight"])
            assert torch.equal(cat([lw.gate_up[i:] for lw in lws]), sd[p + "mlp.up_proj.weight"])
            assert torch.equal(cat([lw.down for lw in lws], 1), sd[p + "mlp.down_proj.weight"])
            continue
        for lw in lws:
            assert torch.equal(f(lw.router), sd[p + "block_sparse_moe.gate.weight"])
        for x in range(E):
            e = p + f"block_sparse_moe.experts.{x}."
            if mode == "ep":  # expert x whole on rank x // (E / W), at local index x % (E / W), and nowhere else
                el = E // world
                r, xl = x // el, x % el
                assert (ms[r].expert0, ms[r].experts_local, ms[r].inter) == (r * el, el, big)
                assert lws[r].w13.shape[0] == el and lws[r].w2.shape[0] == el
                assert torch.equal(f(lws[r].w13[xl, :big]), sd[e + "w1.weight"])
                assert torch.equal(f(lws[r].w13[xl, big:]), sd[e + "w3.weight"])
                assert torch.equal(f(lws[r].w2[xl]), sd[e + "w2.weight"])
            else:
                i = big // world
                assert torch.equal(cat([lw.w13[x, :i] for lw in lws]), sd[e + "w1.weight"])
                assert torch.equal(cat([lw.w13[x, i:] for lw in lws]), sd[e + "w3.weight"])
                assert torch.equal(cat([lw.w2[x] for lw in lws], 1), sd[e + "w2.weight"])


def test_embedding_rows_of_neighbours_differ_by_2x():
    for name, c in CASES.items():
        emb = mr.family_weights(c.arch).embed
        for toks in c.script.seqs.values():
            n = emb[torch.tensor(toks)].norm(dim=-1)
            r = n[1:] / n[:-1]
            assert bool(((r > 1.6) | (r < 1 / 1.6)).all()), name


@pytest.mark.parametrize("name", _scripts())
def test_tolerance_is_under_the_cap(name):
    c = CASES[name]
    tol = mr.case_tolerance(c)
    print(name, {k: round(v, 4) for k, v in tol.items()})
    assert max(tol.values()) <= mr.TOL_CAP, (name, tol)


@pytest.mark.parametrize("name", list(CASES))
def test_claimed_mutations_clear_the_tolerance(name):
    """Each claimed mutation moves >= MUT_ROWS rows (all the rows it affects in a smaller case) beyond
    MUT_FACTOR x tol on at least one tap."""
    c = CASES[name]
    L = mr.arch_of(c.arch).num_layers
    tol = mr.case_tolerance(c)
    clean = mr.oracle_taps(c.arch, c.script)
    assert c.claims
    for mut in c.claims:
        errs = mr.row_errors(mr.oracle_taps(c.arch, c.script, mut, c.world), clean, L)
        best = {}
        for tap, e in errs.items():
            affected = int((e > 1e-6).sum())
            beyond = int((e > mr.MUT_FACTOR * tol[tap]).sum())
            best[tap] = (beyond, affected)
        if c.arch == "moe":  # the route taps: another expert set, or a routing weight beyond MUT_FACTOR x its tolerance
            r = mr.routing_errors(mr.oracle_taps(c.arch, c.script, mut, c.world), c, tol["resid"])
            best["route"] = (r["beyond"], r["affected"])
        assert any(aff > 0 and bey >= min(mr.MUT_ROWS, aff) for bey, aff in best.values()), (name, mut, best)


MOE = [n for n, c in CASES.items() if c.arch == "moe"]


@pytest.mark.parametrize("name", [n for n in _scripts() if n in MOE])
def test_routing_is_decided_in_every_moe_case(name):
    """No (token, layer) of an MoE case has its K-th and (K+1)-th router logit closer than GAP_FACTOR x the bf16
    reference's largest router-logit deviation on that case, and the bf16 reference chooses the oracle's set on
    every one of them: the route taps can be compared exactly."""
    cond = mr.moe_conditions(CASES[name])
    print(name, {k: v for k, v in cond.items() if k != "experts"})
    assert cond["undecided"] == 0 and cond["differ"] == 0, cond
    assert cond["min_gap"] > mr.ROUTE_GAP


def test_every_expert_is_exercised_and_a_decode_step_leaves_some_idle():
    for name in MOE:
        c = CASES[name]
        per_step = mr.moe_conditions(c)["experts"]
        if all(st.prefill for st in c.script.steps) and c.script.tokens() >= 5:
            total = [sum(col) for col in zip(*per_step)]
            assert min(total) > 0, (name, total)
    idle = [name for name in MOE for st, n in zip(CASES[name].script.steps, mr.moe_conditions(CASES[name])["experts"])
            if not st.prefill and min(n) == 0]
    assert idle, "no decode step leaves an expert idle"


def test_the_routing_weight_bound_sees_a_wrong_weight():
    """The tolerance of ``rw`` (moe_reference.py's bound, widened by the input's error at the tolerance of
    ``resid``) passes the bf16 reference and fails the oracle without renormalisation or with the slots exchanged."""
    c = CASES["moe_rowscale_129"]
    tol = mr.case_tolerance(c)["resid"]
    ok = mr.routing_errors(mr.reference_taps(c.arch, c.script, c.fold), c, tol)
    print("bf16 reference:", ok)
    assert ok["differ"] == 0 and ok["rw"] <= 1.0, ok
    for mut in ("moe_no_renorm", "moe_slots_swapped"):
        bad = mr.routing_errors(mr.oracle_taps(c.arch, c.script, mut), c, tol)
        print(mut, bad)
        assert bad["rw"] > 1.0, (mut, bad)
    assert mr.routing_errors(mr.oracle_taps(c.arch, c.script, "moe_router_raw"), c, tol)["differ"] > 0


def test_case_lists_cover_every_path_and_entry():
    for what, pred in mr.COVERAGE.items():
        assert any(pred(n, c) for n, c in CASES.items()), what
    for c in CASES.values():  # every case names a known path
        if c.world > 1:
            for st in c.script.steps:
                mr.group_expected_counts(c, st, 2)
        elif c.arch == "moe":
            for st in c.script.steps:
                mr.moe_expected_counts(c, st, 2)
        else:
            mr.expected_counts(c.path, 2)
    claimed = {m for c in CASES.values() for m in c.claims}
    assert claimed == set(mr.MUTATIONS), set(mr.MUTATIONS) - claimed  # every switch of the oracle is claimed somewhere
    for name, c in CASES.items():  # a switch of a group's hand-offs only where there is a group, and one per group
        assert all(m[:3] not in ("tp_", "ep_", "sp_") for m in c.claims) or c.world > 1, name
    assert sorted(mr.group_cases("w2") + mr.group_cases("w4")) == sorted(n for n, c in CASES.items() if c.world > 1)
    assert {CASES[n].world for n in mr.group_cases("w2")} == {2} and {CASES[n].world for n in mr.group_cases("w4")} == {4}


@pytest.mark.parametrize("n", sorted(mr.RUNNER_PROMPTS))
def test_greedy_steps_are_decided(n):
    """On the oracle's own greedy path at most 10 % of the steps fall under the judged top-2 gap."""
    prompts = mr.runner_prompts(n)
    outs = mr.oracle_greedy(prompts, mr.RUNNER_TOKENS)
    script = mr.emitted_script(prompts, outs)
    tol = mr.tolerance("tiny", script)
    assert max(tol.values()) <= mr.TOL_CAP, tol
    steps = mr.decided_steps(script, tol["logits"])
    total = sum(int(ok.numel()) for _, ok in steps)
    under = sum(int((~ok).sum()) for _, ok in steps)
    for k, (arg, _) in enumerate(steps):  # the script is the oracle's own greedy walk
        assert arg.tolist() == [o[k] for o in outs]
    print(f"{n} prompts: {under} of {total} steps under the gap; tol {tol['logits']:.4f}")
    assert under <= 0.10 * total, (under, total)
    assert len({t for o in outs for t in o}) > n * mr.RUNNER_TOKENS // 2  # the walk does not repeat one token


def test_p13_packs_the_mini_family():
    """The family's folded gate/up stays inside the 13-bit layout's exponent window (else: rescale the family)."""
    from src import ops

    m = mr.family_model("mini", "cpu", torch.bfloat16)
    packed = [ops.gd_pack_weights_p13(lw.gate_up, *ops.P13_TILE, silu=True) for lw in m.layers]
    assert any(p is not None for p in packed)
