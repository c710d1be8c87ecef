"""The FP8 (e4m3) KV-cache writers (rope_cache_kv8_kernel, rope_cache_slab_kv8_kernel) on designed rows: zeros,
subnormals of the stored format, exact ties between two codes, values beyond 448 * scale and a skipped slot.

V rows are not rotated: with a power-of-two scale their bytes must equal the CPU conversion (nearest-even; it turns
overflow into NaN, hence the clamp) exactly. K rows are dequantised and compared with a float64 RoPE of the same
inputs: half an e4m3 step at that magnitude (2^-4 |x| for normals, 2^-10 for subnormals, in stored units) plus four
fp32 ulps of |a cos| + |b sin| for the rotation; beyond 448 the result is exactly +-448. No NaN byte anywhere; q as
the bf16 writer leaves it."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.ops import reference as ref  # noqa: E402

D, BS, HQ, HKV, T, NB = 128, 16, 4, 2, 9, 4
SCALES = [(1.0, 1.0), (0.25, 4.0)]
F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), "HIP extension must be built for GPU tests"
    return torch.device("cuda:0")


def designed(scale, gen):
    """[T, HKV, D] bf16-exact rows in units of `scale`: zeros, subnormals, ties, the top of the range and beyond."""
    codes = torch.arange(0, 127, dtype=torch.uint8).view(F8).float()             # every finite non-negative e4m3
    ties = (codes[:-1] + codes[1:]) / 2                                           # midpoints, exact in bf16
    pool = torch.cat([torch.zeros(8), codes[:9], ties[:24], ties[40:], 2.0 ** -6 * torch.rand(32, generator=gen),
                      torch.tensor([440.0, 448.0, 464.0, 480.0, 1000.0, 3.0e4]), 8 * torch.randn(64, generator=gen)])
    x = pool[torch.randint(len(pool), (T, HKV, D), generator=gen)]
    x = x * torch.where(torch.rand(T, HKV, D, generator=gen) < 0.5, -1.0, 1.0)
    return (x * scale).to(torch.bfloat16)


def inputs(scales, gen):
    q = torch.randn(T, HQ, D, generator=gen).to(torch.bfloat16)
    k, v = designed(scales[0], gen), designed(scales[1], gen)
    qkv = torch.cat([q, k, v], 1).reshape(T, -1)
    pos = torch.randint(0, 4096, (T,), generator=gen)
    pos[0] = 0                                      # no rotation: the K row's ties and subnormals arrive as designed
    slots = torch.randperm(NB * BS, generator=gen)[:T]
    slots[3] = -1
    return qkv, pos, slots


def check(kc, vc, qkv, pos, slots, scales, cs, rs=None):
    kc, vc = kc.cpu(), vc.cpu()
    for c in (kc, vc):
        assert not bool(((c.view(torch.uint8) & 0x7f) == 0x7f).any()), "a NaN byte was written"
    ok = slots >= 0
    blk, off = slots[ok] // BS, slots[ok] % BS
    untouched = torch.ones(NB, BS, dtype=torch.bool)
    untouched[blk, off] = False
    for c in (kc, vc):
        assert bool((c.view(torch.uint8).permute(0, 2, 1, 3)[untouched] == 0).all()), "a skipped or foreign slot was written"
    x = qkv.double().reshape(T, HQ + 2 * HKV, D)
    r = torch.ones(T, dtype=torch.float64) if rs is None else rs.double()
    # V: exact bytes (power-of-two scale; the row scale, where given, is a power of two as well)
    want_v = ref.quantize_kv8((x[:, HQ + HKV:] * r[:, None, None]).float(), scales[1])
    assert torch.equal(vc.view(torch.uint8)[blk, :, off], want_v.view(torch.uint8)[ok]), "V bytes differ"
    # K: float64 rotation, half a step of the stored format plus the rotation's fp32 error
    t = cs.double()[pos][:, None, :]
    a, b, co, si = x[:, HQ:HQ + HKV, :64], x[:, HQ:HQ + HKV, 64:], t[..., :64], t[..., 64:]
    y = torch.cat([a * co - b * si, b * co + a * si], -1) * r[:, None, None] / scales[0]
    mag = torch.cat([(a * co).abs() + (b * si).abs(), (b * co).abs() + (a * si).abs()], -1) * r[:, None, None] / scales[0]
    got = kc.view(F8)[blk, :, off].double()
    y, mag = y[ok], mag[ok]
    rot = 4 * 2.0 ** -23 * mag
    bound = torch.where(y.abs() < 2.0 ** -6, torch.full_like(y, 2.0 ** -10), 2.0 ** -4 * y.abs()) + rot
    over = y.abs() - rot > 448
    assert torch.equal(got[over], 448 * y[over].sign()), "beyond the range: not saturated"
    err = (got - y).abs()[~over] / bound[~over]
    print(f"K worst err/bound {float(err.max()):.3f}; {int(over.sum())} saturated")
    assert float(err.max()) <= 1.0
    assert float(got.abs().max()) <= 448


@pytest.mark.parametrize("scales", SCALES, ids=lambda s: f"k{s[0]}v{s[1]}")
@pytest.mark.parametrize("row_scale", [False, True])
def test_prefill_writer(dev, scales, row_scale):
    gen = torch.Generator().manual_seed(11)
    cs = ref.rope_cos_sin(4096, D, 500000.0)
    qkv, pos, slots = inputs(scales, gen)
    rs = torch.tensor([1.0, 0.5, 2.0, 1.0, 0.25, 4.0, 1.0, 0.5, 2.0]) if row_scale else None
    kc, vc = (torch.zeros(NB, HKV, BS, D, dtype=torch.uint8, device=dev) for _ in range(2))
    g = qkv.to(dev)
    ops.rope_and_cache_kv8(g, pos.to(dev), cs.to(dev), slots.to(dev), kc, vc, HQ, HKV, D, scales[0], scales[1],
                           rot_q=not row_scale, row_scale=None if rs is None else rs.to(dev))
    # q as the bf16 writer leaves it (rotated in place, or untouched with rot_q off)
    b = qkv.to(dev)
    bk, bv = (torch.zeros(NB, HKV, BS, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
    ops.rope_and_cache(b, pos.to(dev), cs.to(dev), slots.to(dev), bk, bv, HQ, HKV, D, rot_q=not row_scale,
                       row_scale=None if rs is None else rs.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(g[:, : HQ * D], b[:, : HQ * D]), "q differs from the bf16 writer's"
    assert torch.equal(g[:, HQ * D:].cpu(), qkv[:, HQ * D:]), "the k / v input columns were modified"
    check(kc, vc, qkv, pos, slots, scales, cs, rs)


@pytest.mark.parametrize("scales", SCALES, ids=lambda s: f"k{s[0]}v{s[1]}")
@pytest.mark.parametrize("sk", [1, 3])
def test_slab_writer(dev, scales, sk):
    gen = torch.Generator().manual_seed(13)
    cs = ref.rope_cos_sin(4096, D, 500000.0)
    qkv, pos, slots = inputs(scales, gen)
    # split-K slabs whose fp32 sum is the bf16 row exactly: power-of-two shares
    share = torch.tensor([[1.0], [0.5, 0.5], [0.5, 0.25, 0.25]][sk - 1])
    slab = (share[:, None, None] * qkv.float()[None]).contiguous()
    kc, vc = (torch.zeros(NB, HKV, BS, D, dtype=torch.uint8, device=dev) for _ in range(2))
    rows = torch.zeros_like(slab[0])   # the kernel's sum starts from +0: a row of -0 shares is +0, as in IEEE
    for i in range(sk):
        rows = rows + slab[i]
    assert torch.equal(rows, qkv.float())
    q8 = ops.rope_and_cache_slab_kv8(slab.to(dev), pos.to(dev), cs.to(dev), slots.to(dev), kc, vc, HQ, HKV, D,
                                     scales[0], scales[1])
    bk, bv = (torch.zeros(NB, HKV, BS, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
    qb = ops.rope_and_cache_slab(slab.to(dev), pos.to(dev), cs.to(dev), slots.to(dev), bk, bv, HQ, HKV, D)
    torch.cuda.synchronize()
    assert torch.equal(q8, qb), "q differs from the bf16 writer's"
    check(kc, vc, rows, pos, slots, scales, cs)


def test_block_moves_on_a_one_byte_pool(dev):
    """Copy, gather and scatter of blocks on the FP8 pool (moved as half as many bf16 elements per row) against the
    same ops on CPU tensors."""
    gen = torch.Generator().manual_seed(17)
    pool = torch.randint(0, 256, (4, 6, HKV, BS, D), generator=gen, dtype=torch.uint8)
    pairs, ids = torch.tensor([[0, 3], [5, 1]]), torch.tensor([4, 0, 2])
    g = pool.to(dev)
    ops.copy_blocks(g, pairs.to(dev))
    ops.copy_blocks(pool, pairs)
    buf = ops.gather_blocks(g, ids.to(dev))
    assert buf.dtype == torch.uint8 and torch.equal(buf.cpu(), ops.gather_blocks(pool, ids))
    ops.scatter_blocks(g, torch.tensor([1, 3, 5], device=dev), buf)
    ops.scatter_blocks(pool, torch.tensor([1, 3, 5]), buf.cpu())
    torch.cuda.synchronize()
    assert torch.equal(g.cpu(), pool)


def test_slab_sum_order_matches_the_bf16_writer(dev):
    """Random fp32 slabs, whose sum depends on the order of the additions: q bit for bit as the bf16 slab writer's."""
    gen = torch.Generator().manual_seed(19)
    cs = ref.rope_cos_sin(4096, D, 500000.0).to(dev)
    slab = torch.randn(3, T, (HQ + 2 * HKV) * D, generator=gen).to(dev)
    pos, slots = torch.randint(0, 4096, (T,), generator=gen).to(dev), torch.arange(T).to(dev)
    kc, vc = (torch.zeros(NB, HKV, BS, D, dtype=torch.uint8, device=dev) for _ in range(2))
    bk, bv = (torch.zeros(NB, HKV, BS, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
    q8 = ops.rope_and_cache_slab_kv8(slab, pos, cs, slots, kc, vc, HQ, HKV, D, 1.0, 1.0)
    qb = ops.rope_and_cache_slab(slab, pos, cs, slots, bk, bv, HQ, HKV, D)
    torch.cuda.synchronize()
    assert torch.equal(q8, qb)
    # V is not rotated: the bytes are the conversion of the fp32 sums in the kernel's order (0 + s0 + s1 + s2)
    v = ((slab[0] + slab[1]) + slab[2]).cpu().reshape(T, -1, D)[:, HQ + HKV:]
    assert torch.equal(vc.cpu()[slots.cpu() // BS, :, slots.cpu() % BS], ref.quantize_kv8(v, 1.0).view(torch.uint8))
