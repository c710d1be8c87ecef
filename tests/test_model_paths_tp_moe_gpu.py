"""The MoE forward paths of the model on one rank, and the tensor-, expert- and sequence-parallel paths on groups
of two and four ranks sharing the GPU, against the float64 oracle of tests/model_reference.py.

mixtral-tiny on the designed family, every case by name from ``model_reference.cases()``: the norm loop, the row-scale
prefill (whose MoE branch keeps ln2 explicit), ``_last_layer_kept_rows`` with an MoE block (a chunk that keeps no row
included), the unfolded model, the fused decode step with both entries, and one decode step captured in a graph. The
cases reach the three regimes of ``ops.moe_apply`` (one streamed pass up to 128 rows, segments up to 255, the library
GEMMs from 256) and both routers (fused ``moe_route`` up to 256 rows, router GEMM + ``topk_softmax`` above).

As in test_model_paths_gpu.py every tap of every token — final-norm hidden rows, the residual stream, the logits, K
and V per layer and kv head — is compared row by row, under ``MARGIN`` (2) x the worst row of the bf16 reference path
on the same script, computed here on the CPU. The scripts are drawn so that every routing decision is decided
(test_model_reference_cpu.py), so the chosen expert sets are compared exactly, and the routing weights within
moe_reference.py's bound widened by the input's error (``model_reference.routing_errors``). The launch counts of the
declared path, down to the MoE launches of the extension, are exact, and every pool slot the script did not write still
holds the sentinel.

Each single-rank case takes under two seconds on an MI355X (most of it the CPU reference that sets the tolerance).

The groups (one spawn each, ``model_reference.spawn_group``): every rank builds ``CausalLM(arch, tp=TPContext(...))``,
loads the full family through ``load_state_dict`` and runs the group's cases in order; the taps are put together as
the full model's (``assemble``) and judged against the same oracle and the same tolerance as on one rank. No path
needed more than margin 2 over the one-rank bf16 reference, so no W-rank CPU yardstick was measured. Per rank the
launch and collective counts of every step are exact, the untouched pool slots hold the sentinel, ``car.error()`` is
false and the epochs agree at the end.
"""

import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from tests import model_reference as mr  # noqa: E402

CASES = mr.cases()
MOE = [n for n, c in CASES.items() if c.arch == "moe" and c.world == 1]
CASE_LIMIT = 5.0   # seconds of GPU work a single-rank case may take (measured: under 1 s each on an MI355X)
# the spawned groups are dominated by process start (two or four fresh interpreters, each opening the GPU, the
# one-shot collectives' buffers and the models). Measured on an MI355X from start to the last report: 3.7 s for the
# 24 cases of the two ranks, 3.1 s for the 2 cases of the four; the limits leave room for a loaded machine
GROUP_LIMIT = {"w2": 90.0, "w4": 90.0}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available()
    return torch.device("cuda:0")


_models = {}


def gpu_model(fold: bool):
    """mixtral-tiny on the family's weights, with its decode scratch for every row bucket: the fused cases all run
    on the same scratch, one after the other."""
    if fold not in _models:
        m = mr.family_model("moe", "cuda:0", torch.bfloat16, fold)
        scratch = m.alloc_decode_scratch(ops.DECODE_GEMM_MAX_M) if fold else None
        if fold:
            assert scratch is not None and sorted(scratch["plans"]) == [32, 64, 128]
        _models[fold] = (m, scratch)
    return _models[fold]


def judge(name, taps):
    """Print every tap's worst row next to its tolerance, then assert them, the routing, the untouched slots and
    the launches of every step."""
    c = CASES[name]
    L = mr.arch_of(c.arch).num_layers
    tol = mr.case_tolerance(c)
    errs = mr.row_errors(taps, mr.oracle_taps(c.arch, c.script), L)
    bad = []
    for tap, e in errs.items():
        worst = float(e.max())
        print(f"{name:22s} {c.path:16s} {tap:7s} worst row {worst:.4f}  tol {tol[tap]:.4f}  "
              f"= {worst / (tol[tap] / mr.MARGIN):.2f} x the bf16 reference's worst row")
        if not worst <= tol[tap]:
            bad.append((tap, worst, tol[tap], int((e > tol[tap]).sum()), int(e.numel())))
    r = mr.routing_errors(taps, c, tol["resid"])
    print(f"{name:22s} {c.path:16s} route   {r['differ']} sets differ; worst routing weight at {r['rw']:.3f} of its "
          f"tolerance (bf16 reference's worst weight error {r['ref_worst']:.2e})")
    assert not bad, (name, bad)
    assert r["differ"] == 0 and r["rw"] <= 1.0, (name, r)
    assert mr.untouched(taps), name
    for i, (st, counts) in enumerate(zip(c.script.steps, taps.counts)):
        want = mr.moe_expected_counts(c, st, L)
        got = {n: counts.get(n, 0) for n in want}
        assert got == want, (name, i, {n: (got[n], want[n]) for n in got if got[n] != want[n]})


@pytest.mark.parametrize("name", [n for n in MOE if not CASES[n].opts.get("graph")])
def test_moe_path_matches_the_oracle(dev, name):
    c = CASES[name]
    m, scratch = gpu_model(c.fold)
    assert m.norms_folded == c.fold
    fused = c.path.startswith("moe_fused")
    script = c.script   # drawn before the clock starts
    t0 = time.time()
    taps = mr.run_paged(m, script, scratch=scratch if fused else None, pre_embedded=c.opts.get("entry") == "pre")
    torch.cuda.synchronize()
    seconds = time.time() - t0
    judge(name, taps)
    assert seconds <= CASE_LIMIT, (name, seconds)


def test_captured_moe_decode_step_equals_the_eager_one(dev):
    """Three fused decode steps of 5 rows, each captured with ``torch.cuda.graph`` and replayed: within tolerance
    of the oracle, with the launches of the streamed MoE pass (no host read under capture), and bit for bit the
    eager steps' hidden rows, logits, routing and KV pool."""
    name = "moe_fused_5_graph"
    c = CASES[name]
    m, scratch = gpu_model(True)
    eager = mr.run_paged(m, c.script, scratch=scratch)
    torch.cuda.synchronize()
    replay = mr.run_paged(m, c.script, scratch=scratch, graph=True)
    torch.cuda.synchronize()
    judge(name, replay)
    for tap in ("hidden", "resid", "logits"):
        for a, b in zip(getattr(eager, tap), getattr(replay, tap)):
            assert torch.equal(a, b), tap
    for key, steps in eager.moe.items():
        for a, b in zip(steps, replay.moe[key]):
            assert torch.equal(a, b), key
    assert torch.equal(eager.pool, replay.pool)


# --------------------------------------------------------------------------------------------------- the two groups
_aborted = []


def _group(name, world):
    """One spawn per group and module. A group that hung or lost a rank is not started again, and after it no other
    group is started on the GPU either."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if _aborted:
        pytest.fail(f"not started: group {_aborted[0]} hung or lost a rank")
    try:
        return mr.spawn_group(name, world, GROUP_LIMIT[name])
    except RuntimeError as e:
        _aborted.append(name)
        pytest.fail(str(e))


@pytest.fixture(scope="module")
def w2(dev):
    return _group("w2", 2)


@pytest.fixture(scope="module")
def w4(dev):
    return _group("w4", 4)


def judge_group(group, reports):
    """Every case of the group by name: what failed in each, and the group's own conditions."""
    failed = {}
    for name in mr.group_cases(group):
        c = CASES[name]
        L = mr.arch_of(c.arch).num_layers
        why = []
        try:
            taps = mr.assemble(c, reports, name)
        except AssertionError as e:
            failed[name] = [str(e)]
            continue
        tol = mr.case_tolerance(c)
        for tap, e in mr.row_errors(taps, mr.oracle_taps(c.arch, c.script), L).items():
            worst = float(e.max())
            print(f"{name:22s} {c.path:12s} {tap:7s} worst row {worst:.4f}  tol {tol[tap]:.4f}  "
                  f"= {worst / (tol[tap] / mr.MARGIN):.2f} x the bf16 reference's worst row")
            if not worst <= tol[tap]:
                why.append((tap, worst, tol[tap], int((e > tol[tap]).sum()), int(e.numel())))
        if c.arch == "moe":
            r = mr.routing_errors(taps, c, tol["resid"])
            print(f"{name:22s} {c.path:12s} route   {r['differ']} sets differ; worst routing weight at {r['rw']:.3f}")
            if r["differ"] or r["rw"] > 1.0:
                why.append(("route", r))
        for rank in range(c.world):
            rep = reports[rank]["cases"][name]
            if not rep["untouched"]:
                why.append(f"rank {rank}: a pool slot the script did not write lost the sentinel")
            for i, (st, counts) in enumerate(zip(c.script.steps, rep["counts"])):
                want = mr.group_expected_counts(c, st, L)
                got = {n: counts.get(n, 0) for n in want}
                if got != want:
                    why.append((f"rank {rank} step {i}", {n: (got[n], want[n]) for n in got if got[n] != want[n]}))
            if c.path == "tp_fused" and not all(rep["plans"].values()):
                why.append(f"rank {rank}: decode_plan's tp_fused {rep['plans']}")
            if c.path in ("tp_separate", "tp_fallback", "ep_fused") and any(rep["plans"].values()):
                why.append(f"rank {rank}: the separate form was asked for, tp_fused {rep['plans']}")
        if why:
            failed[name] = why
    assert not failed, failed
    assert not any(r["error"] for r in reports.values()), "car.error()"
    assert len({r["epoch"] for r in reports.values()}) == 1, {k: r["epoch"] for k, r in reports.items()}


def test_group_of_two_ranks_matches_the_oracle(w2):
    """llama-tiny (fused, separate and fallback decode forms, norm-loop, row-scale, kept-row, cached-prefix and
    sequence-parallel prefill, the vocabulary-parallel head) and mixtral-tiny with split experts and under expert
    parallelism, an all-remote 1-row step included, on two ranks sharing the GPU."""
    shape = {n: w2[1]["cases"][n]["shape"] for n in ("tp2_fused_5", "tp2_moe_tp_5", "tp2_moe_ep_5")}
    assert shape == {"tp2_fused_5": (2, 1, 0, 0, 512), "tp2_moe_tp_5": (2, 1, 4, 0, 512),
                     "tp2_moe_ep_5": (2, 1, 2, 2, 512)}, shape
    judge_group("w2", w2)


def test_group_of_four_ranks_matches_the_oracle(w4):
    """llama-tiny on four ranks: each kv head on two ranks (copies bit-identical), one query head per rank, prefill
    and the generic decode loop across a block edge."""
    assert w4[3]["cases"]["tp4_norm_5"]["shape"][:2] == (1, 1)
    judge_group("w4", w4)
