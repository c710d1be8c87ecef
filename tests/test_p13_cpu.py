"""The decode GEMM's lossless 13-bit weight layout ("P13", src/ops/p13.py, csrc/kernels/gd_p13.h) without a GPU: the
packer and its inverse are exact on every edge of the format, a tensor outside the exponent window is refused, the
packed size is 13/16, and a host replay of the kernel's consumer loop (its read offsets and its in-register unpack,
from the header the kernel includes) rebuilds the tile image from the packer's bytes."""

import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from src import ops
from src.ops import p13

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_TOP = 62  # e >> 1 of the largest exponent pair in the test tensors: base7 = 47, the window is h in 48..62


def _bits(sign, e, m):
    return (sign << 15) | (e << 7) | m


# +0, -0, the smallest and the largest denormal, e = 1 (h = 0 with the low byte's top bit set), the top and the
# bottom exponent of the window (both parities, both signs)
EDGES = [_bits(0, 0, 0), _bits(1, 0, 0), _bits(0, 0, 1), _bits(1, 0, 0x7F), _bits(0, 1, 0), _bits(1, 1, 0x55),
         _bits(0, 2 * H_TOP + 1, 0x7F), _bits(1, 2 * H_TOP, 0), _bits(0, 2 * (H_TOP - 14), 0),
         _bits(1, 2 * (H_TOP - 14) + 1, 0x2A)]


def window_tensor(rows, k, shift, seed=0):
    """bf16 [rows, k] with random in-window values (always one at the top pair) and every EDGES value walking
    over the positions: element (r, c) is edge (r * k + c + shift) % (len(EDGES) + 3), so over the shifts every
    position of a tile — every (MFMA tile, lane, element) of a fragment — sees every edge value."""
    g = torch.Generator().manual_seed(seed)
    n = rows * k
    h = torch.randint(H_TOP - 14, H_TOP + 1, (n,), generator=g)
    bits = (torch.randint(0, 2, (n,), generator=g) << 15) | (h << 8) | torch.randint(0, 256, (n,), generator=g)
    cls = (torch.arange(n) + shift) % (len(EDGES) + 3)
    for i, e in enumerate(EDGES):
        bits = torch.where(cls == i, torch.tensor(e), bits)
    bits = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)
    return bits.view(rows, k).view(torch.bfloat16)


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("silu", [False, True])
def test_pack_unpack_is_exact_on_every_edge_at_every_position(silu):
    for shift in range(len(EDGES) + 3):
        w = window_tensor(256, 256, shift, seed=shift)
        got = ops.gd_pack_weights_p13(w, 128, 128, silu)
        assert got is not None
        packed, base7 = got
        assert base7 == H_TOP - 15
        assert packed.dtype == torch.bfloat16 and packed.shape == (256 * 13 // 16, 256)
        assert packed.numel() * 16 == w.numel() * 13  # exactly 13/16 of the bytes
        assert same_bits(ops.gd_unpack_weights_p13(packed, base7, 128, 128, silu), w)


def test_one_element_below_the_window_is_refused():
    w = window_tensor(128, 128, 0)
    assert ops.gd_pack_weights_p13(w, 128, 128) is not None
    for e in (2 * (H_TOP - 15) + 1, 2 * (H_TOP - 15), 2):  # just below the window, and the lowest h = 1
        bad = w.clone()
        bad.view(torch.int16)[77, 91] = _bits(0, e, 3)
        assert ops.gd_pack_weights_p13(bad, 128, 128) is None
        assert ops.p13_base7(bad) is None


def test_base7_clamps_at_zero_and_all_zero_packs():
    w = torch.zeros(128, 128, dtype=torch.bfloat16)
    packed, base7 = ops.gd_pack_weights_p13(w, 128, 128)
    assert base7 == 0 and same_bits(ops.gd_unpack_weights_p13(packed, 0), w)
    w.view(torch.int16)[3, 5] = _bits(0, 2 * 9 + 1, 1)  # h = 9 <= 15: base7 stays 0, codes are h itself
    packed, base7 = ops.gd_pack_weights_p13(w, 128, 128)
    assert base7 == 0 and same_bits(ops.gd_unpack_weights_p13(packed, 0), w)


def test_normal_weights_fit_the_window():
    w = torch.empty(256, 1024, dtype=torch.bfloat16).normal_(0.0, 0.02, generator=torch.Generator().manual_seed(1))
    got = ops.gd_pack_weights_p13(w, 128, 128, silu=True)
    assert got is not None and same_bits(ops.gd_unpack_weights_p13(*got, silu=True), w)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("gd_p13")
    exe = str(d / "gd_p13_unpack")
    src = os.path.join(ROOT, "csrc", "kernels", "tests", "gd_p13_unpack.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, src], check=True)

    def run(packed, base7):
        pin, pout = str(d / "packed.bin"), str(d / "image.bin")
        packed.contiguous().view(torch.uint8).numpy().tofile(pin)
        subprocess.run([exe, pin, str(base7), pout], check=True)
        return torch.from_numpy(np.fromfile(pout, dtype=np.int16))

    return run


@pytest.mark.parametrize("silu", [False, True])
def test_kernel_index_arithmetic_rebuilds_the_tile_image(replay, silu):
    """What each (wave, lane, MFMA tile) of the kernel reads and unpacks (gd_p13.h) is the B fragment the tile-order
    kernel reads: image row 16 nt + (lane & 15), chunk columns 32 wave + 8 (lane >> 4) + 0..7."""
    rows, k = 256, 384
    for shift in (0, 5, 11):
        w = window_tensor(rows, k, shift, seed=40 + shift)
        packed, base7 = ops.gd_pack_weights_p13(w, 128, 128, silu)
        img = replay(packed, base7).view(rows // 128, k // 128, 128, 128)  # [tile][chunk][image row][k]
        want = w[p13._tile_rows(rows, silu, w.device)].view(torch.int16).view(rows // 128, 128, k // 128, 128)
        assert torch.equal(img, want.permute(0, 2, 1, 3))


def test_layout_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "csrc", "kernels", "gd_p13.h")).read()
    assert f"CHUNK_BYTES = {p13.P13_CHUNK_BYTES};" in hdr and "WR = 128, KC = 128;" in hdr
    assert p13.P13_TILE == (128, 128) and p13.P13_CHUNK_BYTES * 16 == 128 * 128 * 2 * 13
    assert ops.P13 == 128 and ops.P13 & (ops.TILED | ops.HALF_RING | ops.MODE_MASK) == 0
    assert ops.p13_mode(47) == 128 | 47 << 8
