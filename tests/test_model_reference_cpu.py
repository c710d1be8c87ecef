"""The model oracle (tests/model_reference.py) judged before any GPU path is judged by it: it equals the float64
reference path through the paged reference ops, folding is exact on the weight family, and for every GPU case by
name the tolerance stays under its cap and each mutation the case claims clears MUT_FACTOR x tol."""

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
                                  "slab_decode_5"])
def test_oracle_equals_the_float64_reference_path(name):
    """Ragged, chunked, kept-row and decode scripts: the oracle (lists, unfolded gains) against
    ``reference_copy("cpu", float64)`` through block tables and the paged reference ops, to 1e-12 per row."""
    c = CASES[name]
    got = mr.run_paged(mr.reference_model(c.arch, c.fold, torch.float64), c.script)
    assert mr.untouched(got)
    for tap, e in mr.row_errors(got, mr.oracle_taps(c.arch, c.script), mr.arch_of(c.arch).num_layers).items():
        assert float(e.max()) < 1e-12, (name, tap, float(e.max()))


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
        errs = mr.row_errors(mr.oracle_taps(c.arch, c.script, mut), clean, L)
        best = {}
        for tap, e in errs.items():
            affected = int((e > 1e-6).sum())
            beyond = int((e > mr.MUT_FACTOR * tol[tap]).sum())
            best[tap] = (beyond, affected)
        assert any(aff > 0 and bey >= min(mr.MUT_ROWS, aff) for bey, aff in best.values()), (name, mut, best)


def test_case_lists_cover_every_path_and_entry():
    for what, pred in mr.COVERAGE.items():
        assert any(pred(n, c) for n, c in CASES.items()), what
    for c in CASES.values():
        mr.expected_counts(c.path, 2)  # every case names a known path
    claimed = {m for c in CASES.values() for m in c.claims}
    assert claimed == set(mr.MUTATIONS), set(mr.MUTATIONS) - claimed  # every switch of the oracle is claimed somewhere


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
