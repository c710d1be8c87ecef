"""The wide grouped (MoE) W8A16 decode GEMM (csrc/kernels/gemm_decode_w8_grouped_wide.hip, groups of up to 128 rows)
through its binding, against float64 torch, on the integer family and with the helpers of
test_gemm_decode_w8_grouped_gpu.py (`case` asserts sum |x q| < 2^24 and |y| <= 256 s on the CPU; its seeds hold at these
shapes): bf16 outputs equal RNE(oracle) bit for bit, the SiLU form is within silu_mul's derived bound. Group sizes
(33, 0, 128, 95) run the bodies 64, idle, 128, 128 (R = 256: T = 128 tokens with k = 2); (64, 65, 17, 2) run 64, 128,
32, 16 (R = 148), every body boundary crossed from both sides at offsets that are no multiples of 16. K of one chunk (two
half-chunk slots) and of ring_slots_w8(wr, kc, 16) + 1 chunks, which wraps the deepest narrow ring and every wide one."""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cuda")]   # the fixture skips where there is no GPU

from src import ops  # noqa: E402
from tests.gemm_decode_reference import silu_mul  # noqa: E402
from tests.test_gemm_decode_w8_gpu import NAN, SENT, poisoned  # noqa: E402
from tests.test_gemm_decode_w8_grouped_gpu import E, case, launch  # noqa: E402

GROUPS = ((33, 0, 128, 95), (64, 65, 17, 2))


@pytest.fixture(autouse=True)
def wide_binding(monkeypatch):
    """`launch` calls ops.gemm_decode_w8_grouped: here that name is the wide form, which takes the same arguments."""
    monkeypatch.setattr(ops, "gemm_decode_w8_grouped", ops.gemm_decode_w8_grouped_wide)


@pytest.mark.parametrize("sizes", GROUPS)
@pytest.mark.parametrize("mode", (ops.W8_BF16, ops.W8_SILU))
@pytest.mark.parametrize("wr,kc", ops.W8_TILES)
def test_integer_groups(wr, kc, mode, sizes):
    for tch in (1, ops.ring_slots_w8(wr, kc, 16) + 1):
        x, rows, q, s, off, y = case(wr, kc, tch, sizes, mode)
        got = launch(x, rows, q, s, off, mode, wr, kc, max_rows=128)
        o, tol = (y, 0.0) if mode == ops.W8_BF16 else silu_mul(y[:, :wr], y[:, wr:], 1.0)[::2]
        # the sentinel is a bf16 value an output may take (at R = 148 one case's oracle does, twice): only an element
        # whose oracle is not the sentinel shows by it that it was not written
        stale = (got == SENT) & ((o.to(torch.bfloat16).double() - SENT).abs() > tol)
        assert not bool(stale.any()), "an element of [0, off[E]) was not written"
        if mode == ops.W8_BF16:
            bad = (got.view(torch.int16) != y.to(torch.bfloat16).view(torch.int16)).any(1).nonzero().flatten().tolist()
            assert not bad, (tch, "rows", bad)
        else:
            err = (got.double() - o).abs()
            print(f"silu {wr}x{kc} groups {sizes} tch={tch}: worst err / tol {float((err / tol).max()):.3f}")
            assert bool((err <= tol).all()), (tch, (err > tol).any(1).nonzero().flatten().tolist())


@pytest.mark.parametrize("what", ("max_rows", "k", "scales"))
def test_refused_calls_raise_and_write_nothing(what):
    wr, kc, k = 64, 256, 384 if what == "k" else 256
    x, _ = poisoned(torch.ones(128, k, dtype=torch.bfloat16), NAN)
    wq = torch.full((E, 2 * wr, k), 0x38, dtype=torch.uint8, device="cuda")
    s = torch.ones((E * 2 * wr,) if what == "scales" else (E, 2 * wr), device="cuda")
    off = torch.tensor([0, 40, 40, 110, 128], dtype=torch.int32, device="cuda")
    ov, obuf = poisoned(torch.full((128, 2 * wr), SENT, dtype=torch.bfloat16), SENT)
    with pytest.raises(RuntimeError, match="gemm_decode_w8_grouped_wide"):
        ops.gemm_decode_w8_grouped_wide(x, wq, s, off, ops.W8_BF16, wr, kc, max_rows=129 if what == "max_rows" else 128,
                                        out=ov)
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all())
