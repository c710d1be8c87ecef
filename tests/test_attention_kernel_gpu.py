"""The paged-attention kernels (csrc/kernels/attention.hip) element by element against the float64 oracle of
tests/attention_reference.py, at its derived tolerance and on its input families, where every key counts:
test_attention_reference_cpu.py proves for every case used here that a dropped key, chunk, part or tile moves the
oracle by at least four tolerances. Every comparison is |kernel - oracle| <= tol per element (both the tolerance
with the all-elements slack of the fused paths and the tighter one with only the elements that can flip), every
output is finite, and each test prints its worst err / tol."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from tests import attention_reference as ar  # noqa: E402

D = ar.D


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), "HIP extension must be built for GPU tests"
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int16)


def _judge(name, label, out, e):
    o = out.cpu().double().reshape(e.o.shape)
    assert bool(torch.isfinite(o).all()), f"{name}: non-finite output"
    err = (o - e.o).abs()
    r, rt = err / e.tol, err / e.tight
    print(f"{name} [{label}]: worst err/tol {float(r.max()):.3f} (flip-aware tol: {float(rt.max()):.3f})")
    i = int(rt.argmax())
    assert float(rt.max()) <= 1 and float(r.max()) <= 1, \
        f"{name}: {int((rt > 1).sum())} elements off; worst at flat index {i}: got {o.flatten()[i]:.6g}, " \
        f"oracle {e.o.flatten()[i]:.6g}, tol {e.tight.flatten()[i]:.3g}"


def _strided_q(c, dev):
    """q rows as in the model: views into a [T, (hq + 2 hkv) * 128] tensor; what is not q is NaN."""
    wide = torch.full((c.q.shape[0], (c.hq + 2 * c.hkv) * D), float("nan"), dtype=torch.bfloat16, device=dev)
    wide[:, : c.hq * D] = c.q.to(dev)
    return wide[:, : c.hq * D]


def _dev_case(c, dev):
    return (c.kc.to(dev), c.vc.to(dev), c.bt.to(dev), torch.tensor(c.ctxs, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("name", ar.DECODE_CASES)
def test_decode_v3(dev, name):
    """attn_decode_v3_kernel, plain entry: all four families at the block / chunk boundaries for four (G, kv heads),
    the few-pair split (2, 8, 9, 16 one-chunk parts), the 4 x 8 case at both static bounds (one-chunk and 4-chunk
    parts) and 32 x 8 with one part per pair. Both cache policies and a second launch give the same bits, the
    tickets are back at zero after every launch, the caches are untouched."""
    c = ar.case(name)
    q = _strided_q(c, dev)
    kc, vc, bt, ctx = _dev_case(c, dev)
    cnt = torch.zeros(c.n * c.hkv, dtype=torch.int32, device=dev)
    outs = []
    for kv_once in (True, False, True):
        outs.append(ops.attn_decode(q, kc, vc, bt, ctx, c.max_ctx, c.hq, c.hkv, c.scale, counters=cnt, kv_once=kv_once))
        assert int(cnt.abs().sum()) == 0, "merge tickets not re-armed"
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "kv_once changed the result"
    assert torch.equal(_bits(outs[0]), _bits(outs[2])), "a second launch changed the result"
    assert torch.equal(_bits(kc.cpu()), _bits(c.kc)) and torch.equal(_bits(vc.cpu()), _bits(c.vc))
    _judge(name, "decode v3", outs[0], c.expected())


@pytest.mark.parametrize("name", ar.FUSED_CASES)
def test_decode_v3_fused(dev, name):
    """The fused prologue (slab sum, norm scale from 4 / 130 / 256 statistics tiles, RoPE at ctx - 1, KV write) in
    front of the same kernel: split-K 1 - 4 (odd slab-row counts at G = 1), padded rows (slot -1) at a one-key
    context and at 129. The caches after the step equal the oracle's bit for bit except where the exact new k / v
    lies within fp32 error of a rounding midpoint (there: the other neighbour), padded rows wrote nothing, the NaN
    block is still all NaN."""
    c = ar.case(name)
    f, fs, e = c.fused, ar.fused_step(c), c.expected()
    _, _, bt, ctx = _dev_case(c, dev)
    maxp = ops.decode_partials(c.max_ctx)
    po = torch.empty(c.n * c.hq * maxp * D, device=dev)
    pm = torch.empty(c.n * c.hq * maxp * 2, device=dev)
    cnt = torch.zeros(c.n * c.hkv, dtype=torch.int32, device=dev)
    slab, ssp, cs = f.slab.to(dev), f.ssp.to(dev), f.cs.to(dev)
    pos, slots = f.pos.to(dev), f.slots.to(dev)
    runs = []
    for kv_once in (True, False, True):
        kc, vc = f.kc0.to(dev), f.vc0.to(dev)
        out = ops.attn_decode_fused(slab, ssp, pos, cs, slots, kc, vc, bt, ctx, c.max_ctx, c.hq, c.hkv, c.scale,
                                    ar.EPS, ar.HID, po, pm, cnt, kv_once=kv_once)
        assert int(cnt.abs().sum()) == 0, "merge tickets not re-armed"
        runs.append((out, kc.cpu(), vc.cpu()))
    for other in runs[1:]:
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(runs[0], other)), "launches differ"
    out, kc, vc = runs[0]
    _judge(name, f"decode v3 fused sk={f.sk} tiles={f.tiles}", out, e)
    for got, want, x64, delta, what in ((kc, fs.k_after, fs.k64, fs.k_delta, "k"),
                                        (vc, fs.v_after, fs.v64, fs.v_delta, "v")):
        same = _bits(got) == _bits(want)
        flips = 0
        for i, slot in enumerate(f.slots.tolist()):
            if slot < 0:
                continue
            y = got[slot // 16, :, slot % 16]
            assert bool(ar.rounds_to(y, x64[i], delta[i]).all()), f"{name}: new {what} row of sequence {i} is off"
            flips += int((~same[slot // 16, :, slot % 16]).sum())
            same[slot // 16, :, slot % 16] = True
        assert bool(same.all()), f"{name}: {what} cache changed outside the new tokens' rows"
        print(f"{name}: {flips} new {what} elements differ from the oracle's bits, all within the allowance")
        assert bool(torch.isnan(got[c.poison].float()).all())


@pytest.mark.parametrize("name", ar.TWO_LAUNCH_CASES)
def test_decode_two_launch(dev, name):
    """attn_decode_kernel + attn_decode_reduce_kernel: forced by merge_kernel=True, and chosen by the launcher at
    block_size 32; G = 16 exists only here. Contexts 1, 64, 65, 300, 2,049 (17 partials)."""
    c = ar.case(name)
    q = _strided_q(c, dev)
    kc, vc, bt, ctx = _dev_case(c, dev)
    a = ops.attn_decode(q, kc, vc, bt, ctx, c.max_ctx, c.hq, c.hkv, c.scale, merge_kernel=True)
    b = ops.attn_decode(q, kc, vc, bt, ctx, c.max_ctx, c.hq, c.hkv, c.scale, merge_kernel=True)
    assert torch.equal(_bits(a), _bits(b)), "a second launch changed the result"
    if c.bs == 32 or c.g == 16:  # not the v3 kernel's shapes: the launcher takes this path by itself
        cnt = torch.zeros(c.n * c.hkv, dtype=torch.int32, device=dev)
        b = ops.attn_decode(q, kc, vc, bt, ctx, c.max_ctx, c.hq, c.hkv, c.scale, counters=cnt)
        assert torch.equal(_bits(a), _bits(b)) and int(cnt.abs().sum()) == 0
    _judge(name, f"decode two-launch bs={c.bs}", a, c.expected())


@pytest.mark.parametrize("name", ar.PREFILL_CASES)
def test_prefill(dev, name):
    """attn_prefill_kernel, both instances: (NW, NS) = (4, 1) at max_q_len 256, the largest that selects it, and
    (8, 2) at 257, the smallest, with ragged lengths, cached prefixes off the 32- and 64-key stage grid (pos0 = 443) and partly empty
    last q tiles. flat: row i is the exact key counts of [0, pos0 + i] (causal mask of every row, unmasked-tile
    shortcut); witness: keys at pos0 - 1, pos0 and rows' own positions; staircase: the lazy rescale on raw scores;
    random with RoPE-on-load and q_scale."""
    c = ar.case(name)
    q = _strided_q(c, dev)
    kc, vc, bt, ctx = _dev_case(c, dev)
    cu = c.cu.to(dev)
    cs = c.cs.to(dev) if c.cs is not None else None
    qs = c.q_scale.to(dev) if c.q_scale is not None else None
    a = ops.attn_prefill(q, kc, vc, bt, cu, ctx, c.max_q_len, c.hq, c.hkv, c.scale, cos_sin=cs, q_scale=qs)
    b = ops.attn_prefill(q, kc, vc, bt, cu, ctx, c.max_q_len, c.hq, c.hkv, c.scale, cos_sin=cs, q_scale=qs)
    assert torch.equal(_bits(a), _bits(b)), "a second launch changed the result"
    kernel = "(4, 1)" if c.max_q_len <= 256 else "(8, 2)"
    _judge(name, f"prefill {kernel}", a, c.expected())
