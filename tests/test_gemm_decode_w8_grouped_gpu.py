"""The grouped (MoE) W8A16 decode GEMM (csrc/kernels/gemm_decode_w8_grouped.hip) through its binding, against float64
torch: Y[off[e]:off[e + 1]] = (Xrows q[e]^T) * s[e]. The integer family of test_gemm_decode_w8_gpu.py (x = +-1,
q = +-{1..a}, scales 2^(n mod 7 - 3) with n running over all experts' rows, sum |x q| < 2^24 and |y| <= 256 s, both
asserted): bf16 outputs equal RNE(oracle) bit for bit, the SiLU form is within silu_mul's derived bound. E = 4 experts
of two column tiles, group sizes with an empty group, a 1-row group and groups on both sides of 16 at offsets that are
no multiples of 16, K of one chunk and of one wrap of the 16-row ring (deeper than the 32-row ring: both bodies wrap).
Mode 1 gathers token-order rows through a shuffled `rows` with k = 2, mode 0 reads the sorted rows. Outputs sit in
sentinel frames: every row of [0, off[E]) is written, nothing else."""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cuda")]   # the fixture skips where there is no GPU

from src import ops  # noqa: E402
from tests.gemm_decode_reference import silu_mul  # noqa: E402
from tests.test_gemm_decode_w8_gpu import NAN, SENT, poisoned  # noqa: E402

E, TOPK, E4M3 = 4, 2, torch.float8_e4m3fn
GROUPS = ((0, 1, 16, 15), (17, 0, 32, 3))


def case(wr, kc, tch, sizes, mode):
    """(x, rows or None, q [E, 2 wr, K], s [E, 2 wr], off, the float64 oracle [R, 2 wr])."""
    g = torch.Generator().manual_seed(100 * wr + 10 * tch + sum(sizes) + mode)
    k, n, r = tch * kc, 2 * wr, sum(sizes)
    signed = lambda shape, hi: (torch.randint(1, hi + 1, shape, generator=g)  # noqa: E731
                                * (torch.randint(0, 2, shape, generator=g) * 2 - 1))
    q = signed((E, n, k), 3 if k <= 256 else 1).float().to(E4M3)
    s = torch.ldexp(torch.ones(E * n), torch.arange(E * n) % 7 - 3).view(E, n)
    off = torch.tensor((0,) + sizes).cumsum(0).to(torch.int32)
    if mode == ops.W8_SILU:   # token order, gathered through the sorted order's shuffled (token, slot) indices
        x, rows = signed((r // TOPK, k), 1).to(torch.bfloat16), torch.randperm(r, generator=g).to(torch.int32)
        xs = x[rows.long() // TOPK]
    else:
        x, rows = signed((r, k), 1).to(torch.bfloat16), None
        xs = x
    grp = torch.repeat_interleave(torch.arange(E), torch.tensor(sizes))
    qd = q.float().double()
    assert float(torch.einsum("rk,rnk->rn", xs.double().abs(), qd[grp].abs()).max()) < 2 ** 24
    y = torch.einsum("rk,rnk->rn", xs.double(), qd[grp]) * s.double()[grp]
    assert bool((y.abs() <= 256 * s.double()[grp]).all()), "a bf16 output would not be exact"
    return x, rows, q, s, off, y


def launch(x, rows, q, s, off, mode, wr, kc, max_rows=32):
    """Run the binding on poisoned copies; returns the output [R, .], everything around it checked untouched."""
    silu = mode == ops.W8_SILU
    r = x.shape[0] if rows is None else rows.numel()
    packed = ops.gd_pack_experts_w8(q.view(torch.uint8), wr, kc, silu=silu)
    ov, obuf = poisoned(torch.full((r, q.shape[1] // 2 if silu else q.shape[1]), SENT, dtype=torch.bfloat16), SENT)
    ops.gemm_decode_w8_grouped(poisoned(x, NAN)[0], poisoned(packed, 0x7F)[0], poisoned(s, NAN)[0], off.cuda(), mode, wr,
                               kc, rows=None if rows is None else rows.cuda(), k=TOPK if silu else 1,
                               max_rows=max_rows, out=ov)
    torch.cuda.synchronize()
    got = ov.cpu()
    ov.fill_(SENT)
    assert bool((obuf == SENT).all()), "written outside [0, off[E])"
    return got


@pytest.mark.parametrize("sizes", GROUPS)
@pytest.mark.parametrize("mode", (ops.W8_BF16, ops.W8_SILU))
@pytest.mark.parametrize("wr,kc", ops.W8_TILES)
def test_integer_groups(wr, kc, mode, sizes):
    for tch in (1, ops.ring_slots_w8(wr, kc, 16) + 1):
        x, rows, q, s, off, y = case(wr, kc, tch, sizes, mode)
        got = launch(x, rows, q, s, off, mode, wr, kc)
        assert not bool((got == SENT).any()), "an element of [0, off[E]) was not written"
        if mode == ops.W8_BF16:
            bad = (got.view(torch.int16) != y.to(torch.bfloat16).view(torch.int16)).any(1).nonzero().flatten().tolist()
            assert not bad, (tch, "rows", bad)
        else:
            o, _, tol = silu_mul(y[:, :wr], y[:, wr:], 1.0)
            err = (got.double() - o).abs()
            print(f"silu {wr}x{kc} groups {sizes} tch={tch}: worst err / tol {float((err / tol).max()):.3f}")
            assert bool((err <= tol).all()), (tch, (err > tol).any(1).nonzero().flatten().tolist())


@pytest.mark.parametrize("what", ("max_rows", "k", "scales"))
def test_refused_calls_raise_and_write_nothing(what):
    wr, kc, k = 64, 256, 384 if what == "k" else 256
    x, _ = poisoned(torch.ones(32, k, dtype=torch.bfloat16), NAN)
    wq = torch.full((E, 2 * wr, k), 0x38, dtype=torch.uint8, device="cuda")
    s = torch.ones((E * 2 * wr,) if what == "scales" else (E, 2 * wr), device="cuda")
    off = torch.tensor([0, 8, 16, 24, 32], dtype=torch.int32, device="cuda")
    ov, obuf = poisoned(torch.full((32, 2 * wr), SENT, dtype=torch.bfloat16), SENT)
    with pytest.raises(RuntimeError, match="gemm_decode_w8_grouped"):
        ops.gemm_decode_w8_grouped(x, wq, s, off, ops.W8_BF16, wr, kc, max_rows=33 if what == "max_rows" else 32, out=ov)
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all())
