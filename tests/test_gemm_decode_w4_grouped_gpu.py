"""The grouped (MoE) W4A16 decode GEMM on MXFP4 weights (csrc/kernels/gemm_decode_w4_grouped.hip) through its binding,
against float64 torch, on the integer family of test_gemm_decode_w8_grouped_gpu.py: x = +-1, codes drawn uniformly from
all 16, block exponents (n + 3 block) % 4 - 1 with n running over all experts' rows. Every product is a multiple of the
row's smallest grid step and sum |x w| / step < 2^24 (asserted), so fp32 accumulation is exact in any order and bf16
outputs must equal RNE(oracle) bit for bit, which also decides the nibble order and the scale byte's place; the SiLU
form is within silu_mul's derived bound. Groups, K and the gather as in the W8 test; outputs sit in sentinel frames."""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cuda")]   # the fixture skips where there is no GPU

from src import ops  # noqa: E402
from tests.gemm_decode_reference import silu_mul  # noqa: E402
from tests.test_gemm_decode_w8_gpu import NAN, SENT, poisoned  # noqa: E402

E, TOPK = 4, 2
GROUPS = ((0, 1, 16, 15), (17, 0, 32, 3))


def case(wr, kc, tch, sizes, mode, scale_bytes=None):
    """(x, rows or None, codes [E, 2 wr, K / 2], sb [E, 2 wr, K / 32], off, the float64 oracle [R, 2 wr]).
    scale_bytes: (even rows', odd rows') scale byte in place of the family's exponents."""
    g = torch.Generator().manual_seed(100 * wr + 10 * tch + sum(sizes) + mode)
    k, n, r = tch * kc, 2 * wr, sum(sizes)
    pm1 = lambda shape: (torch.randint(0, 2, shape, generator=g) * 2 - 1).to(torch.bfloat16)  # noqa: E731
    codes = torch.randint(0, 256, (E, n, k // 2), generator=g).to(torch.uint8)
    row, blk = torch.arange(E * n).view(E, n, 1), torch.arange(k // 32).view(1, 1, -1)
    if scale_bytes is None:
        sb = ((row + 3 * blk) % 4 - 1 + 127).to(torch.uint8)
    else:
        sb = torch.where(row % 2 == 0, scale_bytes[0], scale_bytes[1]).expand(E, n, k // 32).to(torch.uint8)
    off = torch.tensor((0,) + sizes).cumsum(0).to(torch.int32)
    if mode == ops.W4_SILU:   # token order, gathered through the sorted order's shuffled (token, slot) indices
        x, rows = pm1((r // TOPK, k)), torch.randperm(r, generator=g).to(torch.int32)
        xs = x[rows.long() // TOPK]
    else:
        x, rows = pm1((r, k)), None
        xs = x
    wd = ops.dequantize_weights_mxfp4(codes, sb).double()
    step = torch.ldexp(torch.full((E, n), 0.5, dtype=torch.float64), sb.int().amin(2) - 127)
    y = torch.cat([xs[off[e]:off[e + 1]].double() @ wd[e].T for e in range(E)])
    mass = torch.cat([xs[off[e]:off[e + 1]].double().abs() @ (wd[e].abs() / step[e][:, None]).T for e in range(E)])
    assert float(mass.max()) < 2 ** 24
    return x, rows, codes, sb, off, y


def launch(x, rows, codes, sb, off, mode, wr, kc, max_rows=32):
    """Run the binding on poisoned copies; returns the output [R, .], everything around it checked untouched."""
    silu = mode == ops.W4_SILU
    r = x.shape[0] if rows is None else rows.numel()
    packed = ops.gd_pack_experts_w4(codes, sb, wr, kc, silu=silu)
    ov, obuf = poisoned(torch.full((r, codes.shape[1] // 2 if silu else codes.shape[1]), SENT, dtype=torch.bfloat16), SENT)
    ops.gemm_decode_w4_grouped(poisoned(x, NAN)[0], poisoned(packed, 0x77)[0], off.cuda(), mode, wr, kc,
                               rows=None if rows is None else rows.cuda(), k=TOPK if silu else 1, max_rows=max_rows,
                               out=ov)
    torch.cuda.synchronize()
    got = ov.cpu()
    ov.fill_(SENT)
    assert bool((obuf == SENT).all()), "written outside [0, off[E])"
    return got   # an element left unwritten is SENT: it fails the comparison with the oracle


def rows_that_differ(got, y):
    return (got.view(torch.int16) != y.to(torch.bfloat16).view(torch.int16)).any(1).nonzero().flatten().tolist()


@pytest.mark.parametrize("sizes", GROUPS)
@pytest.mark.parametrize("mode", (ops.W4_BF16, ops.W4_SILU))
@pytest.mark.parametrize("wr,kc", ops.W4_TILES)
def test_integer_groups(wr, kc, mode, sizes):
    for tch in (1, ops.ring_slots_w4(wr, kc, 16) + 1):
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
    # even rows 2^-125 (the quantiser's floor: products down to 2^-126, sums of normal floats), odd rows 2^100
    x, rows, codes, sb, off, y = case(wr, kc, 2, GROUPS[1], ops.W4_BF16, scale_bytes=(2, 227))
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
    with pytest.raises(RuntimeError, match="gemm_decode_w4_grouped"):
        ops.gemm_decode_w4_grouped(x, wq, off, ops.W4_BF16, wr, kc, max_rows=33 if what == "max_rows" else 32, out=ov)
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all())
