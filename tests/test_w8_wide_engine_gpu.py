"""An engine with weight_dtype="fp8" (llama-tiny) above 32 sequences, with the wide row buckets switched on
(ops.W8_WIDE_BUCKETS is shipped empty because the engine measured slower with them, see src/ops/w8.py; the path stays
pinned here): a decode step of 40 rows streams the FP8 copies
through the wide W8 binding four times per layer and never through the bf16 decode GEMM but for the LM head, its
hipGraph windows equal single eager steps, and at 40 and 128 rows it is the bf16 model of the dequantised weights (the
float64 model oracle; the tolerance is the CPU bf16 reference's own error on the same script, which stays under
mr.TOL_CAP at both row counts: 0.039 and 0.035 on the worst tap)."""

import gc

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cuda")]   # the fixture skips where there is no GPU

from src import ops  # noqa: E402
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402
from tests import model_reference as mr  # noqa: E402

N = 40
PROMPTS = [[3 + (11 * i * (j + 1)) % 900 for i in range(3 + j % 7)] for j in range(N)]


@pytest.fixture(scope="module", autouse=True)
def wide_buckets_on():
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "W8_WIDE_BUCKETS", (64, 128))
        yield


@pytest.fixture(scope="module")
def engine(cuda, wide_buckets_on):
    cfg = EngineConfig(max_num_seqs=N, max_num_batched_tokens=512, max_latency_ms=0.0, graph_batch_sizes=[N],
                       num_kv_blocks=256, weight_dtype="fp8")
    eng = LLMEngine.from_preset("llama-tiny", device="cuda:0", cfg=cfg, max_model_len=1024, capture=True)
    eng.eos_token_id = None
    yield eng
    del eng   # released (graphs and all) before the next module's engines are built
    gc.collect()
    torch.cuda.empty_cache()


def test_a_40_row_step_streams_fp8_weights_through_the_wide_kernel(engine, monkeypatch):
    calls, L = [], engine.arch.num_layers
    for mod, name in ((ops._C_w8, "gemm_decode_w8_wide"), (ops._C_w8, "gemm_decode_w8"), (ops._C, "gemm_decode"),
                      (ops._C, "gemm_decode_argmax")):
        monkeypatch.setattr(mod, name, lambda *a, f=getattr(mod, name), n=f"{mod.__name__}.{name}", **k:
                            (calls.append(n), f(*a, **k))[1])
    monkeypatch.setattr(engine, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(engine.runner, "graphs", {})   # eager: one prefill of all 40 prompts, then ONE decode step
    engine.generate(PROMPTS, SamplingParams(max_tokens=2))
    assert calls.count("src._C_w8.gemm_decode_w8_wide") == 4 * L and "src._C_w8.gemm_decode_w8" not in calls
    step = calls[calls.index("src._C_w8.gemm_decode_w8_wide"):]
    assert step.count("src._C.gemm_decode") + step.count("src._C.gemm_decode_argmax") == 1 and step[-1].startswith("src._C.")


def test_graph_windows_match_single_steps(engine, monkeypatch):
    windows = engine.generate(PROMPTS, SamplingParams(max_tokens=8))
    assert engine.runner.graphs, "decode hipGraphs should be captured"
    monkeypatch.setattr(engine, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(engine.runner, "graphs", {})
    assert engine.generate(PROMPTS, SamplingParams(max_tokens=8)) == windows


@pytest.fixture(scope="module")
def model(cuda, wide_buckets_on):
    m = mr.family_model("tiny", "cuda:0", torch.bfloat16)
    assert m.quantize_weights_fp8() == 4 * m.arch.num_layers
    return m


@pytest.mark.parametrize("n", (40, 128))
def test_same_model_as_bf16_on_the_dequantised_weights(model, n):
    script, L = mr.decode_script("tiny", n), model.arch.num_layers
    want = mr.Oracle(mr.Weights.from_model(model), None, 1).run(script)
    ref_err = mr.row_errors(mr.run_paged(model.reference_copy("cpu", torch.bfloat16), script), want, L)
    for tap, e in mr.row_errors(mr.run_paged(model, script), want, L).items():
        tol = mr.MARGIN * float(ref_err[tap].max())
        print(f"fp8 weights, {n} rows  {tap:7s} worst row {float(e.max()):.4f}  tol {tol:.4f}")
        assert tol <= mr.TOL_CAP and float(e.max()) <= tol, (tap, float(e.max()), tol)
