"""MXFP4 expert weights on MoE steps of 33 to 128 tokens, with ops.w4.W4_MOE_MAX_T set to 128 whatever value ships (the
path stays pinned here), as test_w8_moe_wide_gpu.py for the FP8 copies: ops.moe_apply with the experts' MXFP4 copies
against that file's float64 oracle on the dequantised weights (the tolerance is mr.MARGIN times the worst-row error of
the bf16 path, moe_apply without the copies on the same inputs), and an mxfp4_experts mixtral-tiny engine with 40
running sequences: a decode step calls the wide grouped W4 binding twice per layer and no other grouped GEMM, and its
hipGraph windows equal single eager steps."""

import gc

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cuda")]   # the fixture skips where there is no GPU

from src import ops  # noqa: E402
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.models.llama import CausalLM  # noqa: E402
from src.models.presets import get_preset  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402
from tests import model_reference as mr  # noqa: E402
from tests.test_w8_moe_wide_gpu import PROMPTS, N, oracle  # noqa: E402

WIDE = "gemm_decode_w4_grouped_wide"


@pytest.fixture(scope="module", autouse=True)
def w4_moe_up_to_128_tokens():
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops.w4, "W4_MOE_MAX_T", 128)   # the one place ops.moe_apply reads it
        yield


@pytest.fixture(scope="module")
def layer(cuda, w4_moe_up_to_128_tokens):
    """(arch, layer 0, its moe_apply `w4`) of a mixtral-tiny with quantised experts."""
    m = CausalLM(get_preset("mixtral-tiny"), "cuda:0", seed=3)
    assert m.quantize_expert_weights_mxfp4() == 2 * m.arch.num_layers
    return m.arch, m.layers[0], m._moe_w4(m.layers[0])


@pytest.mark.parametrize("resid", (False, True))
@pytest.mark.parametrize("t", (40, 128))
def test_moe_apply_reads_the_mxfp4_experts_above_32_tokens(layer, t, resid):
    arch, lw, w4 = layer
    g = torch.Generator().manual_seed(t)
    x = torch.randn(t, arch.hidden_size, generator=g).to(torch.bfloat16).cuda()
    # expert 0 is drawn four times as often: its group takes the 64-row (t = 40) or 128-row (t = 128) body, the others
    # the 16- / 32-row (t = 40) or 64-row (t = 128) bodies
    ids = torch.multinomial(torch.tensor([4.0, 1, 1, 1]).expand(t, -1), arch.top_k, generator=g).to(torch.int32).cuda()
    w = torch.softmax(torch.randn(t, arch.top_k, generator=g), -1).cuda()
    sizes = torch.bincount(ids.flatten().cpu(), minlength=arch.num_experts).tolist()
    assert max(sizes) > ops.W4_MAX_M and min(sizes) <= 64, sizes
    h0 = torch.randn(t, arch.hidden_size, generator=g).to(torch.bfloat16).cuda()
    want = oracle(x, lw.w13, lw.w2, w, ids) + (h0.double().cpu() if resid else 0)

    def worst_row(copies):
        if resid:
            got = h0.clone()
            ops.moe_apply(x, lw.w13, lw.w2, w, ids, arch.num_experts, residual=got,
                          ssp=torch.zeros(1, ops.SSP_LD, device="cuda"), w4=copies)
        else:
            got = ops.moe_apply(x, lw.w13, lw.w2, w, ids, arch.num_experts, w4=copies)
        got = got.double().cpu()
        return float(((got - want).norm(dim=-1) / want.norm(dim=-1)).max())

    err, ref_err = worst_row(w4), worst_row(None)
    print(f"moe_apply t={t} resid={resid} groups {sizes}: mxfp4 experts {err:.5f}  bf16 path {ref_err:.5f}")
    assert err <= mr.MARGIN * ref_err, (err, ref_err)


@pytest.fixture(scope="module")
def engine(cuda, w4_moe_up_to_128_tokens):
    cfg = EngineConfig(max_num_seqs=N, max_num_batched_tokens=512, max_latency_ms=0.0, graph_batch_sizes=[N],
                       num_kv_blocks=256, weight_dtype="mxfp4_experts")
    eng = LLMEngine.from_preset("mixtral-tiny", device="cuda:0", cfg=cfg, max_model_len=1024, capture=True)
    eng.eos_token_id = None
    yield eng
    del eng   # released (graphs and all) before the next module's engines are built
    gc.collect()
    torch.cuda.empty_cache()


def test_a_40_token_step_streams_mxfp4_experts_through_the_wide_kernel(engine, monkeypatch):
    calls, L = [], engine.arch.num_layers
    for mod, name in ((ops._C_w4, WIDE), (ops._C_w4, "gemm_decode_w4_grouped"), (ops._C, "gemm_decode_grouped")):
        monkeypatch.setattr(mod, name, lambda *a, f=getattr(mod, name), n=name, **k: (calls.append(n), f(*a, **k))[1])
    monkeypatch.setattr(engine, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(engine.runner, "graphs", {})   # eager: one prefill of all 40 prompts, then ONE decode step
    engine.generate(PROMPTS, SamplingParams(max_tokens=2))
    # the prefill (above 128 rows) runs the bf16 segments, but for its last layer, which is cut to the 40 kept rows
    # (a 40-token step itself: 2 calls); the decode step behind it is the wide binding alone, twice per layer
    assert calls[calls.index(WIDE):] == [WIDE] * (2 + 2 * L), calls
    assert set(calls[:calls.index(WIDE)]) == {"gemm_decode_grouped"}


def test_graph_windows_match_single_steps(engine, monkeypatch):
    windows = engine.generate(PROMPTS, SamplingParams(max_tokens=8))
    assert engine.runner.graphs, "decode hipGraphs should be captured"
    monkeypatch.setattr(engine, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(engine.runner, "graphs", {})
    assert engine.generate(PROMPTS, SamplingParams(max_tokens=8)) == windows
