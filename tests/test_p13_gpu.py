"""The decode GEMM on P13 weights (lossless 13-bit layout, csrc/kernels/gd_p13.h) on the MI355X: bit-identical to
the tile-order kernel on the same weights — gate/up with the row-norm SiLU epilogue, the LM head form with its
greedy candidates — at one and two column tiles, one K-chunk, fewer chunks than ring slots and a ring that wraps
twice, on both activation images; and an engine whose gate/up streams P13 generates the same greedy tokens."""

import pytest
import torch

from src import ops

pytestmark = pytest.mark.gpu

ROWS = (1, 7, 16, 17, 32)  # the 16-row image (<= 16) and the 32-row image
KS = (128, 384, 1024)      # 1 chunk, 3 (< 4 ring slots), 8 (the ring wraps twice)


def edge_weights(rows, k, seed):
    """N(0, 0.02)-like bf16 weights clamped into one window, with +0, -0, a denormal, e = 1 and the window's top
    and bottom exponents spread over the positions."""
    g = torch.Generator().manual_seed(seed)
    w = torch.empty(rows, k, dtype=torch.bfloat16).normal_(0.0, 0.02, generator=g)
    bits = w.view(torch.int16).to(torch.int32) & 0xFFFF
    e = (bits >> 7) & 0xFF
    bits = torch.where(e < 96, (bits & 0x807F) | (100 << 7), bits)   # everything inside h in 48..62
    bits = torch.where(e > 125, (bits & 0x807F) | (120 << 7), bits)
    edges = [0x0000, 0x8000, 0x0001, 0x807F, 0x0080, 0x80D5, (125 << 7) | 0x7F, 0x8000 | (124 << 7), 96 << 7,
             0x8000 | (97 << 7) | 0x2A]
    cls = (torch.arange(rows * k).view(rows, k) * 7 + seed) % 23
    for i, v in enumerate(edges):
        bits = torch.where(cls == i, torch.tensor(v), bits)
    bits = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)
    return bits.view(torch.bfloat16)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n_out", [64, 128])
def test_gate_up_p13_is_the_tile_order_kernel_bit_for_bit(n_out, k):
    dev = torch.device("cuda:0")
    w = edge_weights(2 * n_out, k, seed=n_out + k)
    got = ops.gd_pack_weights_p13(w, 128, 128, silu=True)
    assert got is not None
    packed, base7 = got[0].to(dev), got[1]
    assert base7 == 47
    assert torch.equal(ops.gd_unpack_weights_p13(packed, base7, silu=True).cpu().view(torch.int16), w.view(torch.int16))
    tiled = ops.gd_pack_weights(w.to(dev), 128, silu=True, kc=128)
    g = torch.Generator().manual_seed(5)
    for m in ROWS:
        x = torch.randn(m, k, generator=g).to(torch.bfloat16).to(dev)
        ssp = (torch.rand(3, ops.SSP_LD, generator=g) * k / 3).to(dev)
        ref = ops.linear_silu_mul_rownorm(x, tiled, ssp, 1e-5, 128, tiled=True, kc=128)
        out = ops.linear_silu_mul_rownorm(x, packed, ssp, 1e-5, 128, kc=128, p13_base7=base7)
        assert out.shape == ref.shape == (m, n_out)
        assert bool(ref.float().abs().sum() > 0)
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), (m, n_out, k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [128, 256])
def test_lm_head_p13_is_the_tile_order_kernel_bit_for_bit(n, k):
    dev = torch.device("cuda:0")
    w = edge_weights(n, k, seed=3 * n + k)
    packed, base7 = ops.gd_pack_weights_p13(w, 128, 128)
    packed = packed.to(dev)
    tiled = ops.gd_pack_weights(w.to(dev), 128, kc=128)
    g = torch.Generator().manual_seed(6)
    for m in ROWS:
        x = torch.randn(m, k, generator=g).to(torch.bfloat16).to(dev)
        am_ref = torch.full((m, n // 128, 2), -1, dtype=torch.int32, device=dev)
        am_out = torch.full((m, n // 128, 2), -2, dtype=torch.int32, device=dev)
        ref = ops.linear_tiled_argmax(x, tiled, 128, 128, am_ref)
        out = ops.linear_p13_argmax(x, packed, base7, am_out)
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), (m, n, k)
        assert torch.equal(am_out, am_ref), (m, n, k)
        plain = ops.gemm_decode(x, packed, ops.MODE_BF16 | ops.p13_mode(base7), 128, kc=128)
        assert torch.equal(plain.view(torch.int16), ref.view(torch.int16))


def test_launcher_refuses_p13_outside_its_tile_and_modes():
    dev = torch.device("cuda:0")
    w = edge_weights(128, 256, seed=9)
    packed, base7 = ops.gd_pack_weights_p13(w, 128, 128)
    packed = packed.to(dev)
    x = torch.zeros(4, 256, dtype=torch.bfloat16, device=dev)
    flags = ops.p13_mode(base7)
    with pytest.raises(RuntimeError):  # nt = false
        ops.gemm_decode(x, packed, ops.MODE_BF16 | flags, 128, kc=128, nt=False)
    with pytest.raises(RuntimeError):  # a split-K mode
        ops.gemm_decode(x, packed, ops.MODE_SLAB | flags, 128, kc=128)
    with pytest.raises(RuntimeError):  # more rows than the 32-row bucket
        ops.gemm_decode(torch.zeros(33, 256, dtype=torch.bfloat16, device=dev), packed, ops.MODE_BF16 | flags, 128,
                        kc=128)
    with pytest.raises(RuntimeError):  # also TILED
        ops.gemm_decode(x, packed, ops.MODE_BF16 | flags | ops.TILED, 128, kc=128)
    torch.cuda.synchronize()


def _greedy_tokens(monkeypatch, p13_on):
    from src.config import EngineConfig
    from src.engine import LLMEngine
    from src.preproc import SamplingParams

    monkeypatch.setenv("DIE_P13", "1" if p13_on else "0")
    # llama-mini's gate/up (2048 x 1024) on the tile with a P13 kernel
    monkeypatch.setitem(ops.DECODE_TILE_CFG, (2048, 1024, ops.MODE_SILU_NORM, 32), (128, 128, 1))
    cfg = EngineConfig(max_num_seqs=4, max_num_batched_tokens=512, num_kv_blocks=256, graph_batch_sizes=[1, 2, 4])
    eng = LLMEngine.from_preset("llama-mini", device="cuda:0", cfg=cfg, max_model_len=512)
    eng.eos_token_id = None
    assert eng.model.decode_plan(32)["gate_up"] == (128, 128)
    outs = eng.generate([[1, 5, 9, 13] * 20, [1, 2, 3], [7] * 33], SamplingParams(max_tokens=12, temperature=0.0))
    torch.cuda.synchronize()
    return outs, eng.get_stats()


def test_engine_greedy_tokens_are_the_same_with_p13_on_and_off(monkeypatch):
    off, st_off = _greedy_tokens(monkeypatch, False)
    on, st_on = _greedy_tokens(monkeypatch, True)
    assert st_off["p13_tensors_packed"] == 0 and st_off["p13_tensors_raw"] == 0
    # every layer's gate/up is accounted for, and the 13-bit path ran for the packed ones
    assert st_on["p13_tensors_packed"] + st_on["p13_tensors_raw"] == 4
    assert st_on["p13_tensors_packed"] >= 1, st_on
    assert [len(o) for o in on] == [12, 12, 12]
    assert on == off
