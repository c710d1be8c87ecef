"""An engine with weight_dtype="fp8" (llama-tiny): its decode steps stream the FP8 copies through the W8 binding four
times per layer, its hipGraph windows equal single eager steps (bf16 and FP8 KV pools), it is the bf16 model of the
dequantised weights (the float64 model oracle, the bf16 decode step's tolerance), its KV pool grows by the copies not made."""

import gc

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cuda")]   # the fixture skips where there is no GPU

from src import ops  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.engine.llm_engine import plan_kv_blocks  # noqa: E402
from src.engine.model_runner import KVPool  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402
from tests import model_reference as mr  # noqa: E402
from tests.test_kv8_engine_gpu import config  # noqa: E402


def build(capture=True, **kw):
    eng = LLMEngine.from_preset("llama-tiny", device="cuda:0", cfg=config(num_kv_blocks=256, **kw), max_model_len=1024,
                                capture=capture)
    eng.eos_token_id = None
    return eng


@pytest.fixture(scope="module", params=("auto", "fp8"))
def engine(request, cuda):   # an FP8-weight engine per KV pool dtype, released (graphs and all) before the next is built
    eng = build(weight_dtype="fp8", kv_cache_dtype=request.param)
    yield eng
    del eng
    gc.collect()
    torch.cuda.empty_cache()


def eager_decode_step_calls(eng, monkeypatch):   # of a prefill above 128 rows and exactly ONE decode step
    calls = []
    for mod, name in ((ops, "gemm_decode_w8"), (ops._C_w8, "gemm_decode_w8"), (ops._C, "gemm_decode"),
                      (ops._C, "gemm_decode_argmax")):
        monkeypatch.setattr(mod, name, lambda *a, f=getattr(mod, name), n=f"{mod.__name__}.{name}", **k:
                            (calls.append(n), f(*a, **k))[1])
    monkeypatch.setattr(eng, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(eng.runner, "graphs", {})   # eager single steps
    eng.generate([[3 + (7 * i) % 900 for i in range(150)]], SamplingParams(max_tokens=2))
    return calls


def test_fp8_decode_step_streams_fp8_weights(engine, monkeypatch):
    eng, L, st = engine, engine.arch.num_layers, engine.get_stats()
    assert st["weight_dtype"] == "fp8" and st["fp8_tensors_quantized"] == 4 * L and eng.model.w8_plan is not None
    assert all(not lw.tiled for lw in eng.model.layers), "no tile-order or P13 copies of FP8 projections"
    calls = eager_decode_step_calls(eng, monkeypatch)
    # the decode step starts at the first W8 launch (the prefill before it runs bf16 GEMMs on the dequantised weights):
    # four W8 launches per layer, op and binding, and the bf16 decode GEMM once, for the LM head
    assert calls.count("src.ops.gemm_decode_w8") == calls.count("src._C_w8.gemm_decode_w8") == 4 * L
    step = calls[calls.index("src.ops.gemm_decode_w8"):]
    assert step.count("src._C.gemm_decode") + step.count("src._C.gemm_decode_argmax") == 1 and step[-1].startswith("src._C.")


def test_graph_windows_match_single_steps(engine, monkeypatch):
    ps = [[3 + (11 * i * (j + 1)) % 900 for i in range(5 + 43 * j)] for j in range(5)]
    windows = engine.generate(ps, SamplingParams(max_tokens=10))
    assert engine.runner.graphs, "decode hipGraphs should be captured"
    monkeypatch.setattr(engine, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(engine.runner, "graphs", {})
    assert engine.generate(ps, SamplingParams(max_tokens=10)) == windows


def test_default_engine_never_calls_the_w8_binding(monkeypatch):
    assert "src._C_w8.gemm_decode_w8" not in eager_decode_step_calls(build(capture=False), monkeypatch)


def test_same_model_as_bf16_on_the_dequantised_weights():
    m = mr.family_model("tiny", "cuda:0", torch.bfloat16)
    assert m.quantize_weights_fp8() == 4 * m.arch.num_layers
    for lw in m.layers:
        for name, (wr, kc, _) in m.w8_plan.items():
            q = ops.gd_unpack_weights_w8(lw.w8[name][0], wr, kc, silu=name == "gate_up")
            deq = ops.dequantize_weights_fp8(q, lw.w8[name][1]).to(torch.bfloat16)
            assert torch.equal(deq.view(torch.int16), getattr(lw, name).view(torch.int16)), name
    # 5 sequences, 3 decode steps after the prefill; the oracle and the tolerance's bf16 reference path from THESE weights
    script = mr.decode_script("tiny", 5)
    want = mr.Oracle(mr.Weights.from_model(m), None, 1).run(script)
    L = m.arch.num_layers
    ref_err = mr.row_errors(mr.run_paged(m.reference_copy("cpu", torch.bfloat16), script), want, L)
    got = mr.run_paged(m, script)
    for tap, e in mr.row_errors(got, want, L).items():
        tol = mr.MARGIN * float(ref_err[tap].max())
        print(f"fp8 weights  {tap:7s} worst row {float(e.max()):.4f}  tol {tol:.4f}")
        assert float(e.max()) <= tol, (tap, float(e.max()), tol)


def test_kv_pool_grows_by_the_copies_not_made(monkeypatch):
    """The bytes each engine asks the allocator for (its requested-bytes counter: exact, no rounding, no segments) differ
    by what decode_copy_bytes says the FP8 engine no longer copies, within one block; and the planner, given the same
    free HBM less those bytes, plans a pool that is larger by that many blocks, within one."""
    per_block = KVPool.bytes_per_block(2, 2, 16, 128, 2)
    free0, total = torch.cuda.mem_get_info()
    plan, copies, used = {}, {}, {}
    for wd in ("auto", "fp8"):
        gc.collect()   # dead engines are cycles: none is freed while this one is built
        before = torch.cuda.memory_stats()["requested_bytes.all.current"]
        eng = build(capture=False, weight_dtype=wd)
        used[wd] = torch.cuda.memory_stats()["requested_bytes.all.current"] - before
        copies[wd] = eng.model.decode_copy_bytes(eng.model.decode_buckets(8))
        monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None, u=used[wd]: (free0 - u, total))
        plan[wd] = plan_kv_blocks(eng.arch, eng.model, config(weight_dtype=wd), eng.device)
        del eng
    gone, grew = copies["auto"] - copies["fp8"], plan["fp8"] - plan["auto"]
    print(f"copies {copies}: {gone} B = {gone / per_block:.2f} blocks no longer made; requested {used}; planned {plan}")
    assert gone > 2 * per_block, "no pool that stayed as it was passes"
    assert abs((used["auto"] - used["fp8"]) - gone) <= per_block
    assert grew > 0 and abs(grew - gone / per_block) <= 1
