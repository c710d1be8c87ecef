"""Decode attention (attn_decode_v3_kernel): the K/V chunk stream under both cache policies and the task entry —
block ids read speculatively (clamped to the table row, never to the context), parts that start past chunk 0,
the prologue's staged slab rows. Small shapes on both sides of every block (16 keys) and chunk (128 keys)
boundary, against the fp32 reference with test_kernels_gpu.py's tolerances."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.ops import reference as ref  # noqa: E402

BS, D, HID = 16, 128, 1024
BOUNDARY_CTXS = [1, 15, 16, 17, 127, 128, 129, 255, 257]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), "HIP extension must be built for GPU tests"
    torch.manual_seed(0)
    return torch.device("cuda:0")


def close(a, b, atol, rtol):
    assert bool(torch.isfinite(a.float()).all()), "non-finite output"
    d = (a.float() - b.float()).abs()
    bad = (d > atol + rtol * b.float().abs()).sum().item()
    assert bad == 0, f"{bad} elements off; max abs err {d.max().item():.4g}"


def _case(dev, ctxs, g, hkv, max_ctx=None, share=0):
    """Scattered (non-monotonic) block ids; the table row is exactly as long as the longest sequence needs unless
    max_ctx asks for more, and every entry past a sequence's context names a poison block full of NaN. share: the
    first `share` blocks of sequence 1 are sequence 0's (a prefix-cache hit)."""
    n, hq = len(ctxs), hkv * g
    need = [(c + BS - 1) // BS for c in ctxs]
    cols = max(need) if max_ctx is None else max(max_ctx // BS, max(need))
    total = sum(need) + 1
    perm = torch.randperm(total).tolist()
    poison = perm.pop()
    bt = torch.full((n, cols), poison, dtype=torch.int32)
    for i, nb in enumerate(need):
        bt[i, :nb] = torch.tensor([perm.pop() for _ in range(nb)], dtype=torch.int32)
    if share:
        assert share < min(need[0], need[1])  # the last block of a sequence takes its new token: never shared
        bt[1, :share] = bt[0, :share]
    kc = torch.randn(total, hkv, BS, D, device=dev, dtype=torch.bfloat16)
    vc = torch.randn(total, hkv, BS, D, device=dev, dtype=torch.bfloat16)
    kc[poison] = float("nan")
    vc[poison] = float("nan")
    return dict(n=n, hq=hq, hkv=hkv, g=g, ctxs=ctxs, bt=bt.to(dev), kc=kc, vc=vc, poison=poison,
                ctx=torch.tensor(ctxs, dtype=torch.int32, device=dev), max_ctx=max_ctx or cols * BS,
                cu=torch.arange(n + 1, dtype=torch.int32, device=dev), scale=1 / math.sqrt(D))


def _plain(c, dev, kv_once=True, q=None):
    """(kernel output, fp32 reference) of the plain path; q rows strided as in the model."""
    if q is None:
        q = torch.randn(c["n"], (c["hq"] + 2 * c["hkv"]) * D, device=dev, dtype=torch.bfloat16)[:, : c["hq"] * D]
    cnt = torch.zeros(c["n"] * c["hkv"], dtype=torch.int32, device=dev)
    out = ops.attn_decode(q, c["kc"], c["vc"], c["bt"], c["ctx"], c["max_ctx"], c["hq"], c["hkv"], c["scale"],
                          counters=cnt, kv_once=kv_once)
    assert int(cnt.abs().sum()) == 0  # merge tickets re-armed
    r = ref.attention(q, c["kc"], c["vc"], c["bt"], c["cu"], c["ctx"], c["hq"], c["hkv"], c["scale"])
    return out, r.reshape(c["n"], -1), q


def _fused_inputs(c, dev, padded=(), sk=2, tiles=4):
    n, hq, hkv = c["n"], c["hq"], c["hkv"]
    slab = torch.randn(sk, n, (hq + 2 * hkv) * D, device=dev) * 0.7
    ssv = (torch.rand(n, device=dev) + 0.5) * HID
    ssp = torch.zeros(tiles, ops.SSP_LD, device=dev)
    ssp[:, :n] = (ssv / tiles)[None, :]
    real = torch.tensor([int(c["bt"][i, (x - 1) // BS]) * BS + (x - 1) % BS for i, x in enumerate(c["ctxs"])],
                        dtype=torch.long, device=dev)
    slots = real.clone()
    for i in padded:
        slots[i] = -1  # a padded graph row: attends to its new token, writes no cache
    return dict(slab=slab, ssv=ssv, ssp=ssp, real=real, slots=slots, pos=(c["ctx"] - 1).long(),
                cs=ref.rope_cos_sin(4096, D, 500000.0, dev))


def _fused(c, f, dev, kv_once=True):
    """Kernel output and the caches it wrote (the case's own caches stay as they were)."""
    kc, vc = c["kc"].clone(), c["vc"].clone()
    maxp = ops.decode_partials(c["max_ctx"])
    po = torch.empty(c["n"] * c["hq"] * maxp * D, device=dev)
    pm = torch.empty(c["n"] * c["hq"] * maxp * 2, device=dev)
    cnt = torch.zeros(c["n"] * c["hkv"], dtype=torch.int32, device=dev)
    out = ops.attn_decode_fused(f["slab"], f["ssp"], f["pos"], f["cs"], f["slots"], kc, vc, c["bt"], c["ctx"],
                                c["max_ctx"], c["hq"], c["hkv"], c["scale"], 1e-5, HID, po, pm, cnt, kv_once=kv_once)
    assert int(cnt.abs().sum()) == 0
    return out, kc, vc


def _fused_ref(c, f):
    """fp32 reference of the fused path: (attention output, caches after the step)."""
    hq, hkv = c["hq"], c["hkv"]
    rn = torch.rsqrt(f["ssv"] / HID + 1e-5)
    qkv = (f["slab"].sum(0) * rn[:, None]).to(torch.bfloat16)
    ka, va = c["kc"].clone(), c["vc"].clone()   # what the step attends to: every row's new token
    ref.rope_and_cache(qkv.clone(), f["pos"].cpu(), f["cs"], f["real"].cpu(), ka, va, hq, hkv, D)
    kw, vw = c["kc"].clone(), c["vc"].clone()   # what the step leaves in the cache: padded rows write nothing
    q = qkv.clone()
    ref.rope_and_cache(q, f["pos"].cpu(), f["cs"], f["slots"].cpu(), kw, vw, hq, hkv, D)
    r = ref.attention(q[:, : hq * D], ka, va, c["bt"], c["cu"], c["ctx"], hq, hkv, c["scale"])
    return r.reshape(c["n"], -1), kw, vw


def _check_fused(c, f, dev, kv_once=True):
    out, kc, vc = _fused(c, f, dev, kv_once)
    r, kw, vw = _fused_ref(c, f)
    close(out, r, atol=3e-2, rtol=3e-2)
    live = torch.ones(kc.shape[0], dtype=torch.bool, device=dev)
    live[c["poison"]] = False
    close(kc[live], kw[live], atol=3e-2, rtol=2e-2)
    close(vc[live], vw[live], atol=3e-2, rtol=2e-2)
    assert bool(torch.isnan(kc[c["poison"]].float()).all())  # nothing was written past a context
    return out


@pytest.mark.parametrize("g,hkv", [(1, 4), (4, 8), (8, 1)])
@pytest.mark.parametrize("fused", [False, True])
def test_block_and_chunk_boundaries(dev, g, hkv, fused):
    """Contexts on both sides of a block and of a chunk boundary in one batch. The table row is exactly as long as
    the longest sequence needs (its last entry is live) and the shorter sequences' unused entries name a NaN
    block: the speculative ids past a context are loaded clamped to the row and never used. The fused path has
    padded graph rows (slot -1) at a one-key context and at a chunk boundary."""
    c = _case(dev, BOUNDARY_CTXS, g, hkv)
    assert c["bt"].shape[1] == 17 and int(c["bt"][-1, -1]) != c["poison"]
    if fused:
        _check_fused(c, _fused_inputs(c, dev, padded=(0, 5)), dev)
    else:
        out, r, _ = _plain(c, dev)
        close(out, r, atol=2.5e-2, rtol=2e-2)


@pytest.mark.parametrize("fused", [False, True])
def test_few_pair_parts_start_past_chunk_0(dev, fused):
    """A tensor-parallel shard's few (sequence, kv head) pairs: one-chunk parts, one workgroup each, so the
    speculative ids belong to chunks c0 > 0 and the parts past a context exit at once."""
    c = _case(dev, [130, 300, 600, 300], 8, 1, max_ctx=2048)
    if fused:
        _check_fused(c, _fused_inputs(c, dev, padded=(3,)), dev)
    else:
        out, r, _ = _plain(c, dev)
        close(out, r, atol=2.5e-2, rtol=2e-2)


@pytest.mark.parametrize("sk,g,hkv", [(1, 1, 4), (3, 1, 4), (3, 4, 8)])
def test_fused_odd_slab_rows(dev, sk, g, hkv):
    """The slab rows are staged two per DMA instruction: with an odd number of q rows (split-K 1 or 3 at G = 1) one
    pair straddles the last q row and the first k row, or, in a part without the new token, repeats the last."""
    c = _case(dev, [1, 17, 128, 129, 257], g, hkv)
    _check_fused(c, _fused_inputs(c, dev, padded=(1,), sk=sk), dev)


def test_multi_chunk_parts(dev):
    """Parts of several chunks merged by tickets: few sequences, long contexts, ends on both sides of a chunk
    boundary."""
    c = _case(dev, [640, 1023, 1025, 2048], 4, 8, max_ctx=2048)
    out, r, _ = _plain(c, dev)
    close(out, r, atol=2.5e-2, rtol=2e-2)
    _check_fused(c, _fused_inputs(c, dev), dev)


@pytest.mark.parametrize("share", [0, 8])
def test_kv_policy_is_bit_identical(dev, share):
    """The K/V stream's cache policy changes where the bytes are cached, never their values: the same inputs give
    the same bits under both, also when two sequences share their prefix blocks (share = 8: 128 keys)."""
    c = _case(dev, [257, 200, 129, 600], 4, 8, share=share)
    a, r, q = _plain(c, dev, kv_once=True)
    b, _, _ = _plain(c, dev, kv_once=False, q=q)
    assert torch.equal(a, b)
    close(a, r, atol=2.5e-2, rtol=2e-2)
    f = _fused_inputs(c, dev, padded=(2,))
    fa = _check_fused(c, f, dev, kv_once=True)
    fb, _, _ = _fused(c, f, dev, kv_once=False)
    assert torch.equal(fa, fb)
