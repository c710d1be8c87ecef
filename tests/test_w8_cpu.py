"""FP8 (e4m3) weights on the CPU: the quantiser's contract, the W8 packer against its inverse and against
csrc/kernels/gd_w8.h (through csrc/kernels/tests/gd_w8_dump.cpp), and the configurations refused at engine build."""

import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

from src.config import EngineConfig, ModelConfig
from src.engine.backend import LLMBackend
from src.engine.llm_engine import check_weight_dtype
from src.ops import reference as ref
from src.ops import w8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quantiser_contract():
    # bf16 rows of very different magnitudes, one all-zero row, one row whose amax is exactly 448 * 2^-3
    w = torch.randn(96, 512, generator=torch.Generator().manual_seed(0)) * torch.logspace(-6, 4, 96)[:, None]
    w[5] = 0
    w[7, 0] = 56.0
    w[7, 1:] = w[7, 1:].clamp(-56, 56)
    w = w.to(torch.bfloat16)
    q, s = ref.quantize_weights_fp8(w)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and s.shape == (w.shape[0],)
    m, _ = torch.frexp(s)
    assert bool((m == 0.5).all()), "scales are powers of two"
    amax = w.float().abs().amax(1)
    assert bool((amax / s <= 448).all()) and bool(((amax / (s / 2) > 448) | (amax == 0)).all()), "the smallest such"
    assert float(s[5]) == 1.0 and float(s[7]) == 0.125
    want = (w.float() / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(q.view(torch.uint8), want.view(torch.uint8))
    assert not bool(((q.view(torch.uint8) & 0x7F) == 0x7F).any()), "no 0x7f / 0xff byte"
    d = ref.dequantize_weights_fp8(q, s)
    assert torch.equal(d.to(torch.bfloat16).float(), d), "bf16(q * s) is exact"
    assert torch.equal(ref.dequantize_weights_fp8(*ref.quantize_weights_fp8(d.to(torch.bfloat16))), d), "idempotent"


@pytest.mark.parametrize("silu", (False, True))
@pytest.mark.parametrize("wr,kc", w8.W8_TILES)
def test_pack_then_unpack_is_the_identity(wr, kc, silu):
    q = torch.randint(0, 256, (3 * wr, 2 * kc), dtype=torch.uint8, generator=torch.Generator().manual_seed(wr))
    p = w8.gd_pack_weights_w8(q, wr, kc, silu=silu)
    assert p.shape == q.shape and p.dtype == torch.uint8
    assert torch.equal(w8.gd_unpack_weights_w8(p, wr, kc, silu=silu), q)
    # image row r = wr - 3 of tile 1, chunk 1: weight row wr + r, or with the pairing up row N_out + wr / 2 + (r - wr / 2)
    r, k = wr - 3, kc - 5
    row = 3 * (wr // 2) + r if silu else wr + r
    off = int(w8.w8_byte_off(wr, kc, torch.tensor(r), torch.tensor(k)))
    assert int(p.view(3, 2, wr * kc)[1, 1, off]) == int(q[row, kc + k])


def test_python_geometry_is_the_header(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gd_w8_dump")
    src = os.path.join(ROOT, "csrc", "kernels", "tests", "gd_w8_dump.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, src], check=True)
    lines = [line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    geo = [tuple(int(v) for v in ln[1:]) for ln in lines if ln[0] == "G"]
    off = {(int(ln[1]), int(ln[2])): torch.tensor([int(v) for v in ln[3:]]) for ln in lines if ln[0] == "O"}
    assert tuple(dict.fromkeys((wr, kc) for wr, kc, *_ in geo)) == w8.W8_TILES
    assert geo == [(wr, kc, xr, int(w8.w8_tile_valid(wr, kc, xr)), w8.ring_slots_w8(wr, kc, xr),
                    w8.lds_bytes_w8(wr, kc, xr)) for wr, kc in w8.W8_TILES for xr in w8.W8_IMAGES]
    assert all(v for *_, v, _, _ in geo)
    for wr, kc in w8.W8_TILES:
        mine = w8._chunk_index(wr, kc, "cpu")
        assert torch.equal(mine, off[(wr, kc)]) and torch.equal(mine.sort().values, torch.arange(wr * kc))


def test_refused_configurations():
    def model(tp=False, moe=False):
        return SimpleNamespace(tp=SimpleNamespace(enabled=tp), arch=SimpleNamespace(is_moe=moe))

    fp8 = EngineConfig(weight_dtype="fp8")
    assert check_weight_dtype(fp8, model()) and not check_weight_dtype(EngineConfig(), model())
    for cfg, m, what in ((fp8, model(tp=True), "tensor-parallel"), (fp8, model(moe=True), "MoE"),
                         (EngineConfig(weight_dtype="int4"), model(), "auto / fp8")):
        with pytest.raises(ValueError, match=what):
            check_weight_dtype(cfg, m)
    for kw, what in ((dict(weight_dtype="fp8", tp_size=2), "tensor-parallel"), (dict(weight_dtype="int4"), "auto / fp8")):
        with pytest.raises(ValueError, match=what):
            LLMBackend(ModelConfig("m", "", arch="llama", preset="llama-tiny", **kw))
