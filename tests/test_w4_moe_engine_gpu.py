"""An engine with weight_dtype="mxfp4_experts" (mixtral-tiny): a decode step streams the experts' MXFP4 copies through
the grouped W4 binding twice per layer and never calls the bf16 grouped binding, a default engine never calls the W4
one, hipGraph windows equal single eager steps, and the model is the bf16 model of the dequantised weights (the float64
model oracle, the bf16 decode step's tolerance, with the routing asserted equal so that a flip cannot pass as an
error)."""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cuda")]   # the fixture skips where there is no GPU

from src import ops  # noqa: E402
from tests import model_reference as mr  # noqa: E402
from tests.test_w8_moe_engine_gpu import build  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402


@pytest.fixture(scope="module")
def engine(cuda):
    return build(weight_dtype="mxfp4_experts")


def eager_decode_step_calls(eng, monkeypatch):   # of a prefill above 128 rows and exactly ONE decode step
    calls = []
    for mod, name in ((ops._C_w4, "gemm_decode_w4_grouped"), (ops._C, "gemm_decode_grouped")):
        monkeypatch.setattr(mod, name, lambda *a, f=getattr(mod, name), n=name, **k: (calls.append(n), f(*a, **k))[1])
    monkeypatch.setattr(eng, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(eng.runner, "graphs", {})   # eager single steps
    eng.generate([[3 + (7 * i) % 900 for i in range(150)]], SamplingParams(max_tokens=2))
    return calls


def test_decode_step_streams_mxfp4_experts(engine, monkeypatch):
    L, st = engine.arch.num_layers, engine.get_stats()
    assert st["weight_dtype"] == "mxfp4_experts" and st["fp4_tensors_quantized"] == 2 * L
    assert st["fp8_tensors_quantized"] == 0 and st["decode_weight_layout"] == "mxfp4_experts"
    calls = eager_decode_step_calls(engine, monkeypatch)
    # the prefill of 150 rows runs the bf16 segments on the dequantised weights, but for its last layer, which is cut
    # to the one kept row (a step of <= 32 rows: W4); the decode step behind it is W4 alone, twice per layer
    assert calls == ["gemm_decode_grouped"] * (2 * (L - 1)) + ["gemm_decode_w4_grouped"] * (2 + 2 * L)


def test_default_engine_never_calls_the_w4_grouped_binding(monkeypatch):
    calls = eager_decode_step_calls(build(capture=False), monkeypatch)
    assert "gemm_decode_w4_grouped" not in calls and "gemm_decode_grouped" in calls


def test_graph_windows_match_single_steps(engine, monkeypatch):
    ps = [[3 + (11 * i * (j + 1)) % 900 for i in range(5 + 43 * j)] for j in range(5)]
    windows = engine.generate(ps, SamplingParams(max_tokens=10))
    assert engine.runner.graphs, "decode hipGraphs should be captured"
    monkeypatch.setattr(engine, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(engine.runner, "graphs", {})
    assert engine.generate(ps, SamplingParams(max_tokens=10)) == windows


def test_same_model_as_bf16_on_the_dequantised_weights():
    m = mr.family_model("moe", "cuda:0")
    L = m.arch.num_layers
    assert m.quantize_expert_weights_mxfp4() == 2 * L
    # as test_w8_moe_engine_gpu.py: 5 sequences, 3 decode steps after the prefill; the oracle and the tolerance's bf16
    # reference path from THESE weights; the routing of the reference and of the run under test asserted equal to it
    script = mr.decode_script("moe", 5)
    want = mr.Oracle(mr.Weights.from_model(m), None, 1).run(script)
    ref = mr.run_paged(m.reference_copy("cpu", torch.bfloat16), script)
    got = mr.run_paged(m, script, scratch=m.alloc_decode_scratch(32))
    for li in range(L):
        for r, g, w in zip(ref.moe[f"route{li}"], got.moe[f"route{li}"], want.moe[f"route{li}"]):
            assert torch.equal(r, w), "the bf16 reference routes a token unlike the oracle: choose another script"
            assert torch.equal(g, w), f"layer {li}: a token is routed unlike the oracle"
    assert got.counts[-1].get("k.gemm_decode_grouped", 0) == 0, "the decode steps ran the bf16 grouped GEMM"
    ref_err = mr.row_errors(ref, want, L)
    for tap, e in mr.row_errors(got, want, L).items():
        tol = mr.MARGIN * float(ref_err[tap].max())
        print(f"mxfp4 experts  {tap:7s} worst row {float(e.max()):.4f}  tol {tol:.4f}")
        assert float(e.max()) <= tol, (tap, float(e.max()), tol)
