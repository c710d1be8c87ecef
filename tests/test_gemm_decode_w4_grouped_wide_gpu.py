"""The wide grouped (MoE) W4A16 decode GEMM (csrc/kernels/gemm_decode_w4_grouped_wide.hip: groups of up to 128 rows on
the 32-row kernel's packed MXFP4 bytes) through its binding, against float64 torch on the exact integer family of
test_gemm_decode_w4_grouped_gpu.py: fp32 accumulation is exact in any order, so bf16 outputs must equal RNE(oracle) bit
for bit and the SiLU form is within silu_mul's derived bound. The groups reach all four bodies (16-, 32-, 64- and
128-row images, full and partial, and an idle expert); K is one chunk (fewer slots than the ring primes) and
S // 2 + 1 chunks of the deepest wide ring S (more half-chunk slots than the ring holds: it wraps). Outputs sit in
sentinel frames."""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cuda")]   # the fixture skips where there is no GPU

from src import ops  # noqa: E402
from tests.gemm_decode_reference import silu_mul  # noqa: E402
from tests.test_gemm_decode_w4_grouped_gpu import E, TOPK, case, rows_that_differ  # noqa: E402
from tests.test_gemm_decode_w8_gpu import NAN, SENT, poisoned  # noqa: E402

GROUPS = ((33, 0, 64, 15), (128, 65, 32, 17))
NAME = "gemm_decode_w4_grouped_wide"


def launch(x, rows, codes, sb, off, mode, wr, kc):
    """Run the binding on poisoned copies; returns the output [R, .], everything around it checked untouched."""
    silu = mode == ops.W4_SILU
    r = x.shape[0] if rows is None else rows.numel()
    packed = ops.gd_pack_experts_w4(codes, sb, wr, kc, silu=silu)
    ov, obuf = poisoned(torch.full((r, codes.shape[1] // 2 if silu else codes.shape[1]), SENT, dtype=torch.bfloat16), SENT)
    ops.gemm_decode_w4_grouped_wide(poisoned(x, NAN)[0], poisoned(packed, 0x77)[0], off.cuda(), mode, wr, kc,
                                    rows=None if rows is None else rows.cuda(), k=TOPK if silu else 1, out=ov)
    torch.cuda.synchronize()
    got = ov.cpu()
    ov.fill_(SENT)
    assert bool((obuf == SENT).all()), "written outside [0, off[E])"
    return got   # an element left unwritten is SENT: it fails the comparison with the oracle


def deepest_ring(wr):
    return max(ops.ring_slots_w4_wide(wr, xr) for xr in ops.w4.W4_WIDE_IMAGES)


def test_ring_mirror():
    for wr, _ in ops.W4_TILES:
        for xr in ops.w4.W4_WIDE_IMAGES:
            assert ops.ring_slots_w4_wide(wr, xr) == ops._C_w4.ring_slots_wide(wr, xr), (wr, xr)


@pytest.mark.parametrize("sizes", GROUPS)
@pytest.mark.parametrize("mode", (ops.W4_BF16, ops.W4_SILU))
@pytest.mark.parametrize("wr,kc", ops.W4_TILES)
def test_integer_groups(wr, kc, mode, sizes):
    for tch in (1, deepest_ring(wr) // 2 + 1):
        assert tch <= 4   # K <= 1024: case's mass bound holds
        x, rows, codes, sb, off, y = case(wr, kc, tch, sizes, mode)
        got = launch(x, rows, codes, sb, off, mode, wr, kc)
        if mode == ops.W4_BF16:
            assert not rows_that_differ(got, y), (tch, "rows", rows_that_differ(got, y))
        else:
            o, _, tol = silu_mul(y[:, :wr], y[:, wr:], 1.0)
            err = (got.double() - o).abs()
            print(f"silu {wr}x{kc} groups {sizes} tch={tch}: worst err / tol {float((err / tol).max()):.3f}")
            assert bool((err <= tol).all()), (tch, (err > tol).any(1).nonzero().flatten().tolist())


@pytest.mark.parametrize("wr,kc", ops.W4_TILES)
def test_scale_bytes_at_the_floor_and_large(wr, kc):
    # even rows 2^-125 (the quantiser's floor), odd rows 2^100: the wide body finds a scale byte by another address
    x, rows, codes, sb, off, y = case(wr, kc, 2, GROUPS[0], ops.W4_BF16, scale_bytes=(2, 227))
    assert bool((y[:, 0::2].abs() < 2.0 ** -110).all()) and float(y[:, 1::2].abs().max()) > 2.0 ** 100
    got = launch(x, rows, codes, sb, off, ops.W4_BF16, wr, kc)
    assert not rows_that_differ(got, y), rows_that_differ(got, y)


@pytest.mark.parametrize("what", ("max_rows", "k", "tile", "wq"))
def test_refused_calls_raise_and_write_nothing(what):
    wr, kc, k = 32 if what == "tile" else 64, 256, 384 if what == "k" else 256
    x, _ = poisoned(torch.ones(32, k, dtype=torch.bfloat16), NAN)
    wq = torch.full((E, 128, k // 2 + (0 if what == "wq" else k // 32)), 0x22, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 8, 16, 24, 32], dtype=torch.int32, device="cuda")
    ov, obuf = poisoned(torch.full((32, 128), SENT, dtype=torch.bfloat16), SENT)
    with pytest.raises(RuntimeError, match=NAME):
        ops.gemm_decode_w4_grouped_wide(x, wq, off, ops.W4_BF16, wr, kc, max_rows=129 if what == "max_rows" else 128,
                                        out=ov)
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all()) and bool((ov == SENT).all())
