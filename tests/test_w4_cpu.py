"""MXFP4 expert weights on the CPU: the quantiser's contract, the W4 packer against its inverse and against
csrc/kernels/gd_w4.h (through csrc/kernels/tests/gd_w4_dump.cpp), what the engine accepts and refuses, and
CausalLM.quantize_expert_weights_mxfp4 on a CPU mixtral-tiny."""

import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

from src import ops
from src.config import EngineConfig, ModelConfig
from src.engine.backend import LLMBackend
from src.engine.llm_engine import check_weight_dtype
from src.models.llama import CausalLM
from src.models.presets import get_preset
from src.ops import w4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quantiser_contract():
    # bf16 rows of very different magnitudes; then designed blocks in row 0 .. 3
    w = torch.randn(40, 128, generator=torch.Generator().manual_seed(0)) * torch.logspace(-30, 30, 40)[:, None]
    w[0, :32] = 0                                     # a block of zeros
    w[1, :32] = 0
    w[1, 0], w[1, 1] = 2.0 ** -124, -(2.0 ** -126)    # at the exponent floor: e = -126 is clamped to -125
    w[2, :32] = torch.tensor([6.0, 5.0, -7.9, 0.25, 0.75, 1.25, -1.75, 2.5, 3.5] + [0.0] * 23)   # e = 0: every tie
    w = w.to(torch.bfloat16)
    codes, sb = w4.quantize_weights_mxfp4(w)
    assert codes.dtype == sb.dtype == torch.uint8 and codes.shape == (40, 64) and sb.shape == (40, 4)
    assert int(sb.min()) >= w4.W4_MIN_EXP + 127 and int(sb.max()) <= 252
    d = w4.dequantize_weights_mxfp4(codes, sb)
    assert torch.equal(d.to(torch.bfloat16).float(), d), "bf16(dequant) is exact"
    c2, s2 = w4.quantize_weights_mxfp4(d.to(torch.bfloat16))
    assert torch.equal(c2, codes) and torch.equal(s2, sb), "requantising reproduces codes and scales"
    assert int(sb[0, 0]) == 127 and not bool(codes[0, :16].any())
    assert int(sb[1, 0]) == 2 and d[1, :2].tolist() == [2.0 ** -124, -(2.0 ** -126)]
    assert int(sb[2, 0]) == 127   # amax 7.9: floor(log2) = 2
    assert d[2, :9].tolist() == [6.0, 4.0, -6.0, 0.0, 1.0, 1.0, -2.0, 2.0, 4.0], "ties to even, 7.9 saturates"
    assert int(codes[2, 0]) == 7 | 6 << 4 and int(codes[2, 1]) == 15, "element 2 j in the low nibble"
    # every block: amax / 2^e is in [4, 8), where 4 and 6 are, unless the block is zero or e is at the floor
    blk = w.float().view(40, 4, 32).abs().amax(2)
    scaled = blk / torch.ldexp(torch.ones(40, 4), sb.int() - 127)
    assert bool(((blk == 0) | ((scaled >= 4) & (scaled < 8)) | (sb == w4.W4_MIN_EXP + 127)).all())


@pytest.mark.parametrize("silu", (False, True))
@pytest.mark.parametrize("wr,kc", w4.W4_TILES)
def test_pack_then_unpack_is_the_identity(wr, kc, silu):
    g = torch.Generator().manual_seed(wr)
    codes = torch.randint(0, 256, (2, 3 * wr, kc), dtype=torch.uint8, generator=g)     # K = 2 kc
    sb = torch.randint(1, 255, (2, 3 * wr, 2 * kc // 32), dtype=torch.uint8, generator=g)
    p = w4.gd_pack_experts_w4(codes, sb, wr, kc, silu=silu)
    assert p.shape == (2, 3 * wr, kc + 2 * kc // 32) and p.dtype == torch.uint8
    c2, s2 = w4.gd_unpack_experts_w4(p, wr, kc, silu=silu)
    assert torch.equal(c2, codes) and torch.equal(s2, sb)
    # a permutation of the bytes
    assert torch.equal(p.reshape(-1).sort().values, torch.cat([codes.reshape(-1), sb.reshape(-1)]).sort().values)
    # image row r = wr - 3 of tile 1, chunk 1: weight row wr + r, or with the pairing up row N_out + wr / 2 + (r - wr / 2)
    r, k = wr - 3, kc - 5
    row = 3 * (wr // 2) + r if silu else wr + r
    rec = p[1].reshape(3, 2, w4.record_bytes(wr, kc))[1, 1]
    assert int(rec[int(w4.w4_byte_off(wr, kc, torch.tensor(r), torch.tensor(k)))]) == int(codes[1, row, (kc + k) // 2])
    assert int(rec[int(w4.w4_scale_off(wr, kc, torch.tensor(r), torch.tensor(k // 32)))]) == int(sb[1, row, (kc + k) // 32])


def test_python_geometry_is_the_header(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gd_w4_dump")
    src = os.path.join(ROOT, "csrc", "kernels", "tests", "gd_w4_dump.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, src], check=True)
    lines = [line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    geo = [tuple(int(v) for v in ln[1:]) for ln in lines if ln[0] == "G"]
    tab = {(ln[0], int(ln[1]), int(ln[2])): torch.tensor([int(v) for v in ln[3:]]) for ln in lines if ln[0] != "G"}
    assert tuple(dict.fromkeys((wr, kc) for wr, kc, *_ in geo)) == w4.W4_TILES
    assert geo == [(wr, kc, xr, int(w4.w4_tile_valid(wr, kc, xr)), w4.ring_slots_w4(wr, kc, xr),
                    w4.lds_bytes_w4(wr, kc, xr), w4.slot_bytes_w4(wr, kc, xr))
                   for wr, kc in w4.W4_TILES for xr in w4.W4_IMAGES]
    assert all(g[3] for g in geo)
    for wr, kc in w4.W4_TILES:
        r, k = torch.arange(wr).view(-1, 1), torch.arange(kc).view(1, -1)
        assert torch.equal(w4.w4_byte_off(wr, kc, r, k).reshape(-1), tab[("O", wr, kc)])
        assert torch.equal((k & 1).expand(wr, kc).reshape(-1), tab[("N", wr, kc)])
        assert torch.equal(w4.w4_scale_off(wr, kc, r, torch.arange(kc // 32).view(1, -1)).reshape(-1), tab[("S", wr, kc)])
        ci, si = w4._record_index(wr, kc, "cpu")
        assert torch.equal(torch.cat([ci, si]).sort().values, torch.arange(w4.record_bytes(wr, kc)))


def test_accepted_and_refused_configurations():
    def model(tp=False, moe=False):
        return SimpleNamespace(tp=SimpleNamespace(enabled=tp), arch=SimpleNamespace(is_moe=moe))

    mx = EngineConfig(weight_dtype="mxfp4_experts")
    assert check_weight_dtype(mx, model(moe=True))
    start = "weight_dtype must be auto / fp8 / fp8_experts / mxfp4_experts"
    for cfg, m, what in ((mx, model(), "dense"), (mx, model(tp=True, moe=True), "tensor-parallel"),
                         (EngineConfig(weight_dtype="mxfp4_experts", kv_cache_dtype="fp8"), model(moe=True),
                          "kv_cache_dtype"), (EngineConfig(weight_dtype="mxfp4"), model(moe=True), start)):
        with pytest.raises(ValueError, match=what):
            check_weight_dtype(cfg, m)
    for kw, what in ((dict(weight_dtype="mxfp4_experts"), "dense"), (dict(weight_dtype="mxfp4"), start),
                     (dict(weight_dtype="mxfp4_experts", tp_size=2), "tensor-parallel")):
        with pytest.raises(ValueError, match=what):
            LLMBackend(ModelConfig("m", "", arch="llama", preset="llama-tiny", overrides={"device": "cpu"}, **kw))


def test_quantised_experts_are_the_models_experts():
    m = CausalLM(get_preset("mixtral-tiny"), "cpu", seed=3)
    L = m.arch.num_layers
    assert m.quantize_expert_weights_mxfp4() == 2 * L and m.weight_dtype == "mxfp4_experts"
    (t13, t2), lw = m.w4_moe_tiles, m.layers[0]
    assert m.decode_copy_bytes(()) == L * sum(w.numel() * 17 // 32 for w in (lw.w13, lw.w2))
    for again in (False, True):   # quantising the quantised values again changes no value, of the weights or the copies
        before = [(lw.w13.clone(), lw.w2.clone(), lw.w4["w13"].clone(), lw.w4["w2"].clone()) for lw in m.layers]
        assert not again or m.quantize_expert_weights_mxfp4() == 2 * L
        for lw, (w13, w2, q13, q2) in zip(m.layers, before):
            assert not again or (torch.equal(lw.w13, w13) and torch.equal(lw.w2, w2)
                                 and torch.equal(lw.w4["w13"], q13) and torch.equal(lw.w4["w2"], q2))
            for name, tile, silu in (("w13", t13, True), ("w2", t2, False)):
                deq = w4.dequantize_experts_w4(lw.w4[name], *tile, silu=silu).to(torch.bfloat16)
                assert torch.equal(deq.view(torch.int16), getattr(lw, name).view(torch.int16)), name
    # the CPU op with the copies reads THEM: it equals the op on the dequantised weights, also when w13 / w2 are junk
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, m.arch.hidden_size, generator=g).to(torch.bfloat16)
    w, ids = ops.moe_route(x, lw.router, m.arch.top_k)
    want = ops.moe_apply(x, lw.w13, lw.w2, w, ids, m.arch.num_experts)
    got = ops.moe_apply(x, torch.zeros_like(lw.w13), torch.zeros_like(lw.w2), w, ids, m.arch.num_experts, w4=m._moe_w4(lw))
    assert bool(want.any()) and torch.equal(got, want)
    with pytest.raises(ValueError, match="w8 and w4"):
        ops.moe_apply(x, lw.w13, lw.w2, w, ids, m.arch.num_experts, w8=(), w4=m._moe_w4(lw))
