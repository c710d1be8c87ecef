"""Decode and prefill attention over the FP8 (e4m3) KV cache against the float64 oracle of attention_reference.py.

The case's bf16 caches are quantised on the CPU (src.ops.reference.quantize_kv8) and dequantised again; the oracle and
its derived tolerance run on the dequantised values (exact in bf16 at these power-of-two scales), the kernel gets the
bytes and the scales. Dequantisation is exact, so the bf16 kernels' tolerance applies unchanged. Poison blocks and the
rows past a context stay NaN bytes: a kernel that reads one shows it."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.ops import reference as ref  # noqa: E402
from tests import attention_reference as ar  # noqa: E402

SCALES = [(1.0, 1.0), (0.5, 2.0)]
DECODE_SHAPES = [(1, 4), (4, 8), (8, 1)]          # (G, kv heads)
DECODE_BOUND = 2048                               # static bound: parts of 3, 6 and 1 chunks at the shapes above
PREFILL_PAIRS = [(1, 1), (37, 37), (33, 161), (128, 300), (257, 700)]
assert set(PREFILL_PAIRS) <= set(ar.PREFILL_PAIRS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), "HIP extension must be built for GPU tests"
    return torch.device("cuda:0")


def quantised(c, k_scale, v_scale):
    """(k bytes, v bytes, c): the caches of the freshly made case c (nothing derived from them yet) are replaced by
    the dequantised values."""
    kq, vq = ref.quantize_kv8(c.kc, k_scale), ref.quantize_kv8(c.vc, v_scale)
    c.kc, c.vc = ref.dequantize_kv8(kq, k_scale).to(ar.BF16), ref.dequantize_kv8(vq, v_scale).to(ar.BF16)
    assert torch.equal(c.kc.float().nan_to_num(7.0), ref.dequantize_kv8(kq, k_scale).nan_to_num(7.0)), "inexact"
    return kq, vq, c


def check(out, c8, what):
    exp = c8.expected()
    got = out.detach().cpu().double().reshape(exp.o.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - exp.o).abs()
    worst, tight = float((err / exp.tol).max()), float((err / exp.tight).max())
    print(f"{what}: worst err/tol {worst:.3f} (tight {tight:.3f})")
    assert worst <= 1.0 and tight <= 1.0, f"{what}: err/tol {worst:.3f}, tight {tight:.3f}"


@pytest.mark.parametrize("scales", SCALES, ids=lambda s: f"k{s[0]}v{s[1]}")
@pytest.mark.parametrize("family", ["witness", "random"])
@pytest.mark.parametrize("g,hkv", DECODE_SHAPES)
def test_decode(dev, g, hkv, family, scales):
    # the smallest contexts that span two and three parts of the kernel's plan at this launch shape
    n = len(ar.BOUNDARY) + 2
    pk = ops.attn_decode_kv8_part_keys(n, hkv, DECODE_BOUND)
    ctxs = ar.BOUNDARY + [pk + 1, 2 * pk + 1]
    name = f"{family}-kv8-g{g}x{hkv}"
    c = ar.make_case(name, family, [1] * n, ctxs, g, hkv, max_ctx=DECODE_BOUND, seed=ar._seed(name))
    kq, vq, c8 = quantised(c, *scales)
    out = ops.attn_decode_kv8(c.q.to(dev), kq.to(dev), vq.to(dev), c.bt.to(dev),
                              torch.tensor(c.ctxs, dtype=torch.int32, device=dev), c.max_ctx, c.hq, c.hkv, c.scale,
                              scales[0], scales[1])
    torch.cuda.synchronize()
    check(out, c8, f"{name} parts of {pk} keys, scales {scales}")


@pytest.mark.parametrize("fz", ["", "+cs+qs"])
@pytest.mark.parametrize("scales", SCALES, ids=lambda s: f"k{s[0]}v{s[1]}")
@pytest.mark.parametrize("family", ["witness", "random"])
@pytest.mark.parametrize("g", [1, 4, 8])
@pytest.mark.parametrize("size", ["small", "large"])   # max q len 128 / 257: the launcher's two shapes
def test_prefill(dev, size, g, family, scales, fz):
    pairs = [p for p in PREFILL_PAIRS if size == "large" or p[0] <= 256]
    name = f"{family}-kv8-pf-{size}-g{g}{fz}"
    c = ar.make_case(name, family, [p[0] for p in pairs], [p[1] for p in pairs], g, 2, seed=ar._seed(name), stride=1)
    if fz:
        ar.add_rope(c, q_scale=True, seed=ar._seed(name))
    kq, vq, c8 = quantised(c, *scales)
    out = ops.attn_prefill_kv8(c.q.to(dev), kq.to(dev), vq.to(dev), c.bt.to(dev), c.cu.to(dev),
                               torch.tensor(c.ctxs, dtype=torch.int32, device=dev), max(c.qlens), c.hq, c.hkv, c.scale,
                               scales[0], scales[1], cos_sin=c.cs.to(dev) if fz else None,
                               q_scale=c.q_scale.to(dev) if fz else None)
    torch.cuda.synchronize()
    check(out, c8, f"{name} scales {scales}")
