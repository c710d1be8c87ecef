"""The fused-prologue decode attention over the FP8 (e4m3) KV cache against attention_reference.py's float64 models,
on test_kv8_attention_gpu.py's decode case with add_fused's operands; rows 0 and 6 (contexts 1, 129) are padded.
1. The new rows' bytes against fused_step's k / v in stored units: half an e4m3 step (test_kv8_write_gpu.py's rule)
   plus fused_step's fp32 allowance over the scale; no NaN byte; no other byte of either cache changes.
2. The output against the oracle on fused_step's q and the caches with the new rows as written (bounded in 1.). A
   padded row's bytes exist nowhere: the float64 values quantised on the CPU stand in, and its elements within the fp32
   allowance of an e4m3 midpoint (the random family's bf16 values sit on them) may flip by one step: e4m3_flip. Without
   that 11 of 36 cases missed, by up to 16 x. 3. kv_once True / False / True: equal bits, tickets at zero."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.ops import reference as ref  # noqa: E402
from tests import attention_reference as ar  # noqa: E402
from tests.test_kv8_attention_gpu import DECODE_BOUND, DECODE_SHAPES, SCALES, dev, quantised  # noqa: E402,F401


def e4m3_flip(x, delta):
    """ar.flip_move in the cache's format: one step (2^-3 of the binade, 2^-9 below 2^-6) within delta of a midpoint."""
    u = torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -6))) - 3)
    fr = x.abs() / u - torch.floor(x.abs() / u)
    return torch.where((fr - 0.5).abs() * u <= delta, u, torch.zeros_like(u))


@pytest.mark.parametrize("scales", SCALES, ids=lambda s: f"k{s[0]}v{s[1]}")
@pytest.mark.parametrize("family", ["witness", "random"])
@pytest.mark.parametrize("sk,tiles", [(2, 4), (3, 256), (4, 130)])   # odd slab-row counts at G = 1, 40 rows at G = 8
@pytest.mark.parametrize("g,hkv", DECODE_SHAPES)
def test_fused_decode(dev, g, hkv, sk, tiles, family, scales):  # noqa: F811
    n = len(ar.BOUNDARY) + 2
    pk, name = ops.attn_decode_kv8_part_keys(n, hkv, DECODE_BOUND), f"{family}-kv8f-g{g}x{hkv}-sk{sk}-t{tiles}"
    c = ar.make_case(name, family, [1] * n, ar.BOUNDARY + [pk + 1, 2 * pk + 1], g, hkv, max_ctx=DECODE_BOUND,
                     seed=ar._seed(name))
    f = ar.add_fused(quantised(c, *scales)[2], sk=sk, tiles=tiles, padded=(0, 6), seed=ar._seed(name)).fused
    q0 = [ref.quantize_kv8(f.kc0, scales[0]), ref.quantize_kv8(f.vc0, scales[1])]   # the stale rows included
    po = torch.empty(n * c.hq * (c.max_ctx // 128) * ar.D, device=dev)
    pm, cnt = torch.empty(po.numel() // 64, device=dev), torch.zeros(n * hkv, dtype=torch.int32, device=dev)
    args = [t.to(dev) for t in (f.slab, f.ssp, f.pos, f.cs, f.slots)]
    tail = (c.bt.to(dev), torch.tensor(c.ctxs, dtype=torch.int32, device=dev), c.max_ctx, c.hq, hkv, c.scale, ar.EPS,
            ar.HID, po, pm, cnt)
    runs = []
    for kv_once in (True, False, True):
        kc, vc = q0[0].to(dev), q0[1].to(dev)
        out = ops.attn_decode_fused(*args, kc, vc, *tail, kv_once=kv_once, kv_scales=scales)
        assert int(cnt.abs().sum()) == 0, "merge tickets not re-armed"
        runs.append((out.cpu().view(torch.int16), kc.cpu().view(torch.uint8), vc.cpu().view(torch.uint8)))
    assert all(torch.equal(a, b) for other in runs[1:] for a, b in zip(runs[0], other)), "launches differ"
    blk, off, ok, fs = f.real // 16, f.real % 16, (f.slots >= 0)[:, None, None], ar.fused_step(c)
    att, mv = [f.kc0.clone(), f.vc0.clone()], []
    for j, (x64, delta) in enumerate(((fs.k64, fs.k_delta), (fs.v64, fs.v_delta))):
        s, got, x = scales[j], runs[0][1 + j], x64 / scales[j]
        b = got[blk, :, off]                      # [n, hkv, D]; a padded row still holds the stale bytes
        assert not bool((((b & 0x7f) == 0x7f) & ok).any()), f"{name}: NaN byte in a new row of cache {j}"
        bound = torch.where(x.abs() < 2.0 ** -6, torch.full_like(x, 2.0 ** -10), 2.0 ** -4 * x.abs()) + delta / s
        worst = float(((ref.dequantize_kv8(b, 1.0).double() - x).abs() / bound * ok).max())
        same = got == q0[j].view(torch.uint8)
        same[blk, :, off] |= ok                   # the stored rows may differ; a padded row's slot may not
        assert worst <= 1.0 and bool(same.all()), f"{name}: cache {j}: new rows {worst:.3f} or other bytes changed"
        att[j][blk, :, off] = torch.where(ok, ref.dequantize_kv8(b, s),
                                          ref.dequantize_kv8(ref.quantize_kv8(x.float(), 1.0), s)).to(ar.BF16)
        mv.append(e4m3_flip(x, delta / s) * s * ~ok)
    o, a, sl, fl = ar.oracle(fs.q, att[0], att[1], c.bt, c.cu, c.ctxs, c.hq, hkv, c.scale, slack=True,
                             moves=(fs.moves[0], mv[0], mv[1]))
    got = runs[0][0].view(ar.BF16).double().reshape(o.shape)
    worst, tight = (float(((got - o).abs() / ar.tolerance(o, a, t)).max()) for t in (sl + fl, fl))
    print(f"{name}: parts of {pk} keys, worst err/tol {worst:.3f} (tight {tight:.3f})")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0 and tight <= 1.0, f"{name}: {worst:.3f}, tight {tight:.3f}"
