"""The wide W8A16 decode GEMM (csrc/kernels/gemm_decode_w8_wide.hip, 33 to 128 rows) against float64 torch on the tensors
as given: test_gemm_decode_w8_gpu.py's families, frames (sentinel around the output, NaN around the operands) and
bounds, at the wide kernel's images (64 rows: M = 64 and 33; 128 rows: M = 128 and 65) and ring depths. The ring holds
half chunks, so its depth in whole chunks is S = ceil(slots / 2) and K / 256 in {1, S, S + 1, 2 S + 1} is the first fill,
a full ring and two wraps."""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("cuda")]   # the fixture skips where there is no GPU

from src import ops  # noqa: E402
from src.ops import reference as ref  # noqa: E402
from tests.gemm_decode_reference import C_SILU, U23, half_ulp_bf16, partials, silu_mul, slices  # noqa: E402
from tests.test_gemm_decode_w8_gpu import E4M3, NAN, NTILES, SENT, poisoned  # noqa: E402

IMAGES = ((64, (64, 33)), (128, (128, 65)))   # image -> (its top M, the smallest M that selects it)
TILE_IMAGES = [(wr, kc, xr, ms) for wr, kc in ops.W8_TILES for xr, ms in IMAGES]


def launch(x, q, s, mode, wr, kc, sk=1, m=None):
    """Run the kernel on poisoned copies of (x[:m], q, s); returns the output, everything around it checked."""
    m = x.shape[0] if m is None else m
    n = q.shape[0] // 2 if mode == ops.W8_SILU else q.shape[0]
    packed = ops.gd_pack_weights_w8(q.view(torch.uint8), wr, kc, silu=mode == ops.W8_SILU)
    blank = torch.empty((sk, m, n), dtype=torch.float32) if mode == ops.W8_SLAB else torch.empty((m, n), dtype=x.dtype)
    ov, obuf = poisoned(blank.fill_(SENT), SENT)
    out = ops.gemm_decode_w8_wide(poisoned(x[:m], NAN)[0], poisoned(packed, 0x7F)[0], poisoned(s, NAN)[0], mode, wr, kc,
                                  sk, out=ov)
    torch.cuda.synchronize()
    got = ov.cpu()
    assert out.data_ptr() == ov.data_ptr() and not bool((got == SENT).any()), "an element of [M, N] was not written"
    ov.fill_(SENT)
    assert bool((obuf == SENT).all()), "written outside [M, N]"
    return got


def integer_case(wr, tch, kc, a, seed=0):
    """x [128, K] of +-1, q [3 wr, K] e4m3 of +-{1..a}, scales 2^(n mod 7 - 3)."""
    g = torch.Generator().manual_seed(1000 * wr + 10 * tch + a + seed)
    k, n = tch * kc, NTILES * wr
    signed = lambda shape, hi: (torch.randint(1, hi + 1, shape, generator=g)  # noqa: E731
                                * (torch.randint(0, 2, shape, generator=g) * 2 - 1))
    x = signed((128, k), 1).to(torch.bfloat16)
    q = signed((n, k), a).float().to(E4M3)
    assert float((x.double().abs() @ q.float().double().abs().T).max()) < 2 ** 24
    return x, q, torch.ldexp(torch.ones(n), torch.arange(n) % 7 - 3)


def ring_chunks(wr, xr):
    s = (ops.ring_slots_w8_wide(wr, xr) + 1) // 2
    return (1, s, s + 1, 2 * s + 1)


def test_code_table_is_exact():
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    for n, (wr, kc) in ((NTILES * t[0], t) for t in ops.W8_TILES):
        q = codes[(torch.arange(kc)[None, :] + 37 * torch.arange(n)[:, None]) % 254].view(E4M3)
        hot = (torch.arange(128) * 61 + 7) % kc
        x = torch.zeros(128, kc, dtype=torch.bfloat16)
        x[torch.arange(128), hot] = 1
        for m in (128, 64):
            assert set(q[:, hot[:m]].view(torch.uint8).flatten().tolist()) == set(codes.tolist()), "every code is an output"
            got = launch(x, q, torch.ones(n), ops.W8_SLAB, wr, kc, m=m)[0]
            want = (x[:m].double() @ q.float().double().T).float()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (wr, m)
            assert torch.equal(want, q[:, hot[:m]].float().T), "the oracle is the decoded value"


@pytest.mark.parametrize("wr,kc,xr,ms", TILE_IMAGES)
def test_integer_slabs_over_the_ring(wr, kc, xr, ms):
    """One slice over the ring's chunk counts; uneven split slices (2 over 3 chunks, 3 over 5), run twice."""
    for sk, tch in [(1, t) for t in ring_chunks(wr, xr)] + [(2, 3), (3, 5)]:
        x, q, s = integer_case(wr, tch, kc, 16 if tch * kc <= 256 else 3)
        for m in ms:
            want = (partials(x[:m].double(), q.float().double(), kc, sk) * s.double()).float()
            got = launch(x, q, s, ops.W8_SLAB, wr, kc, sk, m=m)
            assert torch.equal(got, want), (sk, tch, m, float((got - want).abs().max()))
            if sk > 1:
                assert torch.equal(launch(x, q, s, ops.W8_SLAB, wr, kc, sk, m=m).view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("wr,kc,xr,ms", TILE_IMAGES)
def test_integer_bf16_and_silu(wr, kc, xr, ms):
    for tch in ring_chunks(wr, xr):
        x, q, s = integer_case(wr, tch, kc, 3 if tch * kc <= 512 else 1)
        y = (x.double() @ q.float().double().T) * s.double()
        assert bool((y.abs() <= 256 * s.double()).all()), "a bf16 output would not be exact"
        for m in ms:
            assert torch.equal(launch(x, q, s, ops.W8_BF16, wr, kc, m=m), y[:m].to(torch.bfloat16)), (tch, m)
        x, q, s = integer_case(wr, tch, kc, 3 if tch * kc <= 320 else 1, seed=1)
        y = (x.double() @ q.float().double().T) * s.double()
        o, _, tol = silu_mul(y[:, :y.shape[1] // 2], y[:, y.shape[1] // 2:], 1.0)
        for m in ms:
            err = (launch(x, q, s, ops.W8_SILU, wr, kc, m=m).double() - o[:m]).abs()
            print(f"silu {wr}x{kc} m={m} tch={tch}: worst err / tol {float((err / tol[:m]).max()):.3f}")
            assert bool((err <= tol[:m]).all()), (tch, m)


@pytest.mark.parametrize("mode,sk", ((ops.W8_BF16, 1), (ops.W8_SILU, 1), (ops.W8_SLAB, 4)))
@pytest.mark.parametrize("scale_mul", (1.0, 1.37))
def test_random_family(mode, sk, scale_mul):
    wr, kc, k, m = 64, 256, 8 * 256, 128
    g = torch.Generator().manual_seed(7 + mode)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16)
    q, s = ref.quantize_weights_fp8((torch.randn(NTILES * wr, k, generator=g) / k ** 0.5).to(torch.bfloat16))
    s = s * scale_mul
    xd, w = x.double(), q.float().double() * s.double()[:, None]
    got = launch(x, q, s, mode, wr, kc, sk).double()
    if mode == ops.W8_SLAB:
        for by, (lo, hi) in enumerate(slices(k, kc, sk)):
            o = xd[:, lo:hi] @ w[:, lo:hi].T
            tol = (k + sk) * 2.0 ** -24 * (xd[:, lo:hi].abs() @ w[:, lo:hi].abs().T) + 2.0 ** -24 * o.abs()
            print(f"random slab {by} x{scale_mul}: worst err / tol {float(((got[by] - o).abs() / tol).max()):.3f}")
            assert bool(((got[by] - o).abs() <= tol).all()), by
        return
    y = xd @ w.T
    big = (k + sk) * 2.0 ** -24 * (xd.abs() @ w.abs().T) + 2.0 ** -24 * y.abs()
    if mode == ops.W8_BF16:
        tol, o = big + half_ulp_bf16(y.abs() + big), y
    else:
        n = y.shape[1] // 2
        o, z, _ = silu_mul(y[:, :n], y[:, n:], 1.0)
        eg, eu = big[:, :n], big[:, n:]
        prop = 1.1 * eg * y[:, n:].abs() + (z / (1 + torch.exp(-z))).abs() * eu + 1.1 * eg * eu
        tol = prop + C_SILU * U23 * (1 + z.abs() + eg) * (o.abs() + prop) + half_ulp_bf16(o.abs() + prop)
    err = (got - o).abs()
    print(f"random mode {mode} x{scale_mul}: worst err / tol {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("m,k,n", ((32, 256, 192), (129, 256, 192), (64, 384, 192), (64, 256, 200)))
def test_refused_shapes_raise_and_write_nothing(m, k, n):
    x, _ = poisoned(torch.ones(m, k, dtype=torch.bfloat16), NAN)
    wq = torch.full((n, k), 0x38, dtype=torch.uint8, device="cuda")
    ov, obuf = poisoned(torch.full((1, m, n), SENT), SENT)
    with pytest.raises(RuntimeError, match="gemm_decode_w8_wide"):
        ops.gemm_decode_w8_wide(x, wq, torch.ones(n, device="cuda"), ops.W8_SLAB, 64, 256, 1, out=ov)
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all())
