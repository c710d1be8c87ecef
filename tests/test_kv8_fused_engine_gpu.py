"""An engine with kv_cache_dtype="fp8" decodes on the five-launch fused layer (one FP8 ops.attn_decode_fused per layer,
no slab-path RoPE + KV-write), its hipGraph windows equal single eager steps; a bf16 pool keeps the bf16 binding."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402
from tests.test_kv8_engine_gpu import config  # noqa: E402


def build(**kw):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    eng = LLMEngine.from_preset("llama-tiny", device="cuda:0", cfg=config(num_kv_blocks=256, **kw), max_model_len=1024,
                                capture=False)
    eng.eos_token_id, eng.model.kv_scales = None, [(0.5, 2.0), (1.0, 0.25)]   # not all ones: a lost scale shows
    eng.runner.capture_graphs()   # after the scales: a captured launch holds them as arguments
    return eng


engine = pytest.fixture(scope="module")(lambda: build(kv_cache_dtype="fp8"))


def eager_decode_step_calls(eng, monkeypatch):   # of a prefill that is no slab-path step and exactly ONE decode step
    calls = []
    for mod, name in ((ops, "attn_decode_fused"), (ops, "rope_and_cache_slab"), (ops._C, "attn_decode_fused"),
                      (ops._C_kv8, "attn_decode_fused_kv8")):
        monkeypatch.setattr(mod, name, lambda *a, f=getattr(mod, name), n=name, **k: (calls.append(n), f(*a, **k))[1])
    monkeypatch.setattr(eng, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(eng.runner, "graphs", {})   # eager single steps
    eng.generate([[3 + (7 * i) % 900 for i in range(150)]], SamplingParams(max_tokens=2))   # > 128 rows: plain prefill
    return calls


def test_fp8_decode_takes_the_fused_layer(engine, monkeypatch):
    assert engine.pool.tensor.element_size() == 1 and engine.model._fused_decode_ok(engine.pool.tensor, 8)
    assert eager_decode_step_calls(engine, monkeypatch) == ["attn_decode_fused", "attn_decode_fused_kv8"] * 2


def test_graph_windows_match_single_steps(engine, monkeypatch):
    ps = [[3 + (11 * i * (j + 1)) % 900 for i in range(5 + 43 * j)] for j in range(5)]
    windows = engine.generate(ps, SamplingParams(max_tokens=10))
    assert engine.runner.graphs, "decode hipGraphs should be captured"
    monkeypatch.setattr(engine, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(engine.runner, "graphs", {})
    assert engine.generate(ps, SamplingParams(max_tokens=10)) == windows


def test_bf16_pool_calls_the_bf16_binding(monkeypatch):
    assert eager_decode_step_calls(build(), monkeypatch) == ["attn_decode_fused"] * 4   # op and binding, 2 layers
