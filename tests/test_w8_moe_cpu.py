"""weight_dtype="fp8_experts" off the GPU: what the engine accepts and refuses, and CausalLM.quantize_expert_weights_fp8
on a CPU mixtral-tiny: the kept FP8 copies are exactly the overwritten bf16 experts, quantising twice changes nothing,
and ops.moe_apply with the copies computes what it computes on the dequantised bf16 weights."""

from types import SimpleNamespace

import pytest
import torch

from src import ops
from src.config import EngineConfig, ModelConfig
from src.engine.backend import LLMBackend
from src.engine.llm_engine import check_weight_dtype
from src.models.llama import CausalLM
from src.models.presets import get_preset


def test_accepted_and_refused_configurations():
    def model(tp=False, moe=False):
        return SimpleNamespace(tp=SimpleNamespace(enabled=tp), arch=SimpleNamespace(is_moe=moe))

    experts = EngineConfig(weight_dtype="fp8_experts")
    assert check_weight_dtype(experts, model(moe=True))
    for cfg, m, what in ((experts, model(), "dense"), (experts, model(tp=True, moe=True), "tensor-parallel"),
                         (EngineConfig(weight_dtype="fp8_experts", kv_cache_dtype="fp8"), model(moe=True), "kv_cache_dtype"),
                         (EngineConfig(weight_dtype="fp8"), model(moe=True), "MoE.*fp8_experts")):
        with pytest.raises(ValueError, match=what):
            check_weight_dtype(cfg, m)
    with pytest.raises(ValueError, match="dense"):
        LLMBackend(ModelConfig("m", "", arch="llama", preset="llama-tiny", weight_dtype="fp8_experts",
                               overrides={"device": "cpu"}))


def test_quantised_experts_are_the_models_experts():
    m = CausalLM(get_preset("mixtral-tiny"), "cpu", seed=3)
    L = m.arch.num_layers
    assert m.quantize_expert_weights_fp8() == 2 * L and m.weight_dtype == "fp8_experts"
    (t13, t2), lw = m.w8_moe_tiles, m.layers[0]
    assert m.decode_copy_bytes(()) == L * sum(w.numel() + 4 * w.shape[0] * w.shape[1] for w in (lw.w13, lw.w2))
    for again in (False, True):   # quantising the quantised values again changes no value, of the weights or the copies
        before = [(lw.w13.clone(), lw.w2.clone()) for lw in m.layers]
        assert not again or m.quantize_expert_weights_fp8() == 2 * L
        for lw, (w13, w2) in zip(m.layers, before):
            assert not again or (torch.equal(lw.w13, w13) and torch.equal(lw.w2, w2))
            for name, tile, silu in (("w13", t13, True), ("w2", t2, False)):
                q, s = lw.w8[name]
                deq = ops.dequantize_weights_fp8(ops.gd_unpack_experts_w8(q, *tile, silu=silu), s).to(torch.bfloat16)
                assert torch.equal(deq.view(torch.int16), getattr(lw, name).view(torch.int16)), name
    # the CPU op with the copies reads THEM: it equals the op on the dequantised weights, also when w13 / w2 are junk
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, m.arch.hidden_size, generator=g).to(torch.bfloat16)
    w, ids = ops.moe_route(x, lw.router, m.arch.top_k)
    want = ops.moe_apply(x, lw.w13, lw.w2, w, ids, m.arch.num_experts)
    got = ops.moe_apply(x, torch.zeros_like(lw.w13), torch.zeros_like(lw.w2), w, ids, m.arch.num_experts, w8=m._moe_w8(lw))
    assert bool(want.any()) and torch.equal(got, want)
