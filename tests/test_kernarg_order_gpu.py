"""The decode kernels' argument lists are ordered for kernarg preload (what a wave reads before its first load comes
first, the by-value structs' early fields are passed as separate leading arguments, small ones packed into one
`head` word). These tests guard against an argument landing in the wrong slot: every reordered or packed field
gets a value that no other field has (rows != columns != K != the row strides, tiled and row-major weights, split
counts, statistics tile counts, a grouped call with empty groups, fused and plain attention, the sampling advance),
at the smallest shapes that reach it, against the fp32 references and tolerances of tests/test_kernels_gpu.py.
GPU only."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.ops import reference as ref  # noqa: E402
from tests import sampling_reference as sr  # noqa: E402

N, K, LDX = 256, 512, 640     # the 256 x 512 weight; activation rows are views of a wider buffer (ldx != K)
WR, KC = 64, 128              # 4 column tiles x 4 K slots
ROWS = [1, 7, 32]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), "HIP extension must be built for GPU tests"
    torch.manual_seed(0)
    return torch.device("cuda:0")


def close(a, b, atol, rtol=0.0):
    d = (a.float() - b.float()).abs()
    lim = atol + rtol * b.float().abs()
    bad = (d > lim).sum().item()
    assert bad == 0, f"{bad} elements off; max abs err {d.max().item():.4g}"


@pytest.fixture(scope="module")
def gemm_inputs(dev):
    """Shared, never modified: x rows (strided), the weight (row-major and both tile orders), fp32 product."""
    g = torch.Generator(device=dev).manual_seed(3)
    big = torch.randn(32, LDX, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    return {"big": big, "w": w, "wt": ops.gd_pack_weights(w, WR, kc=KC),
            "wt_silu": ops.gd_pack_weights(w, WR, silu=True, kc=KC),
            "ref": big[:, :K].float() @ w.float().t()}


def _w(gi, tiled, silu=False):
    return (gi["wt_silu"] if silu else gi["wt"]) if tiled else gi["w"]


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("m", ROWS)
def test_mode0_bf16(dev, gemm_inputs, m, tiled):
    x = gemm_inputs["big"][:m, :K]
    y = ops.gemm_decode(x, _w(gemm_inputs, tiled), mode=ops.MODE_BF16 | (ops.TILED if tiled else 0), wr=WR, kc=KC)
    close(y, gemm_inputs["ref"][:m], atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("m", ROWS)
def test_mode2_slabs(dev, gemm_inputs, m, tiled):
    x = gemm_inputs["big"][:m, :K]
    s = ops.gemm_decode(x, _w(gemm_inputs, tiled), mode=ops.MODE_SLAB | (ops.TILED if tiled else 0), wr=WR, sk=2, kc=KC)
    assert s.shape == (2, m, N)
    # each slab is its own half of K (fp32 sums of exact bf16 products: 2e-3 as test_gemm_decode_uneven_split_slabs)
    w = gemm_inputs["w"].float()
    for i in range(2):
        close(s[i], x[:, i * K // 2:(i + 1) * K // 2].float() @ w[:, i * K // 2:(i + 1) * K // 2].t(), atol=2e-3, rtol=2e-3)


def _mode3(gi, dev, m, tiled, sk):
    x = gi["big"][:m, :K]
    g = torch.Generator(device=dev).manual_seed(m + sk)
    res = torch.randn(m, N + 64, device=dev, generator=g).to(torch.bfloat16)[:, :N]  # ld_resid != N
    r0 = res.clone()
    t = N // WR
    ssp = torch.full((t, ops.SSP_LD), -1.0, device=dev)
    cnt = torch.zeros(t, dtype=torch.int32, device=dev)
    ops.linear_slab_residual(x, _w(gi, tiled), res, ssp, cnt, WR, sk, tiled=tiled, kc=KC)
    close(res, (r0.float() + gi["ref"][:m]).to(torch.bfloat16), atol=3e-2, rtol=1e-2)
    close(ssp[:, :m], res.float().pow(2).view(m, t, WR).sum(-1).t(), atol=1e-2, rtol=1e-3)
    assert torch.all(ssp[:, m:32] == 0) and int(cnt.abs().sum()) == 0


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("m", ROWS)
def test_mode3_residual(dev, gemm_inputs, m, tiled):
    _mode3(gemm_inputs, dev, m, tiled, sk=4)


def test_mode3_residual_two_slices(dev, gemm_inputs):
    _mode3(gemm_inputs, dev, 7, True, sk=2)


def _silu_ref(gi, m, ssp):
    r = torch.rsqrt(ssp[:, :m].sum(0) / K + 1e-5)[:, None]
    y = gi["ref"][:m] * r
    return torch.nn.functional.silu(y[:, :N // 2]) * y[:, N // 2:]


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("m", ROWS)
def test_mode4_rownorm_silu(dev, gemm_inputs, m, tiled):
    x = gemm_inputs["big"][:m, :K]
    ss = x.float().pow(2)
    ssp = torch.zeros(3, ops.SSP_LD, device=dev)   # 3 statistics tiles (uneven shares of the row's sum)
    ssp[:, :m] = torch.stack([ss[:, :100].sum(-1), ss[:, 100:300].sum(-1), ss[:, 300:].sum(-1)])
    y = ops.linear_silu_mul_rownorm(x, _w(gemm_inputs, tiled, silu=True), ssp, 1e-5, WR, tiled=tiled, kc=KC)
    close(y, _silu_ref(gemm_inputs, m, ssp), atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("m", ROWS)
def test_mode6_split_k_silu(dev, gemm_inputs, m, tiled):
    x = gemm_inputs["big"][:m, :K]
    ss = x.float().pow(2)
    ssp = torch.zeros(2, ops.SSP_LD, device=dev)
    ssp[:, :m] = torch.stack([ss[:, :200].sum(-1), ss[:, 200:].sum(-1)])
    slab = torch.empty(2 * m * N, dtype=torch.float32, device=dev)
    cnt = torch.zeros(N // WR, dtype=torch.int32, device=dev)
    y = ops.linear_silu_mul_rownorm(x, _w(gemm_inputs, tiled, silu=True), ssp, 1e-5, WR, tiled=tiled, kc=KC, sk=2,
                                    slab=slab, counters=cnt)
    close(y, _silu_ref(gemm_inputs, m, ssp), atol=3e-2, rtol=3e-2)
    assert int(cnt.abs().sum()) == 0


def test_grouped_with_empty_groups(dev):
    """8 tokens routed to experts 0 and 1 of 8: six empty groups; the gate/up call gathers its rows through the
    sorted order (fz.grp_rows), the down call reads them in place."""
    t, h, inter, e = 8, 1024, 512, 8
    x = torch.randn(t, h, device=dev, dtype=torch.bfloat16)
    w13 = torch.randn(e, 2 * inter, h, device=dev, dtype=torch.bfloat16) / math.sqrt(h)
    w2 = torch.randn(e, h, inter, device=dev, dtype=torch.bfloat16) / math.sqrt(inter)
    ids = torch.tensor([[0, 1]] * t, device=dev, dtype=torch.int32)
    w = torch.softmax(torch.randn(t, 2, device=dev), -1)
    close(ops.moe_apply(x, w13, w2, w, ids, e), ref.moe_experts(x, w13, w2, w, ids), atol=3e-2, rtol=3e-2)


# ---------------------------------------------------------------------------------------------- decode attention
G, HKV, BS, D = 4, 2, 16, 128
CTX_PAIRS = [(1, 129), (16, 1), (17, 16), (129, 17)]   # every context as sequence 0 and as sequence 1


def _seqs(ctxs, dev):
    nb = [(c + BS - 1) // BS for c in ctxs]
    total = sum(nb) + 4
    perm = torch.randperm(total).tolist()
    bt = torch.zeros(len(ctxs), max(nb) + 1, dtype=torch.int32)
    p = 0
    for i, n in enumerate(nb):
        bt[i, :n] = torch.tensor(perm[p:p + n], dtype=torch.int32)
        p += n
    kc = torch.randn(total, HKV, BS, D, device=dev, dtype=torch.bfloat16)
    vc = torch.randn(total, HKV, BS, D, device=dev, dtype=torch.bfloat16)
    return kc, vc, bt.to(dev), torch.tensor(ctxs, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("ctxs", CTX_PAIRS)
def test_attn_decode_plain(dev, ctxs):
    hq, max_ctx = HKV * G, 512
    kc, vc, bt, ctx = _seqs(ctxs, dev)
    q = torch.randn(2, (hq + 2 * HKV) * D, device=dev, dtype=torch.bfloat16)[:, : hq * D]  # q_stride != hq * D
    bt_wide = torch.zeros(2, max_ctx // BS, dtype=torch.int32, device=dev)
    bt_wide[:, : bt.shape[1]] = bt
    cnt = torch.zeros(2 * HKV, dtype=torch.int32, device=dev)
    scale = 1 / math.sqrt(D)
    out = ops.attn_decode(q, kc, vc, bt_wide, ctx, max_ctx, hq, HKV, scale, counters=cnt)
    cu = torch.arange(3, dtype=torch.int32, device=dev)
    close(out, ref.attention(q, kc, vc, bt, cu, ctx, hq, HKV, scale).reshape(2, -1), atol=2.5e-2, rtol=2e-2)
    assert int(cnt.abs().sum()) == 0


@pytest.mark.parametrize("ctxs", CTX_PAIRS)
def test_attn_decode_fused(dev, ctxs):
    """As tests/test_kernels_gpu.py::test_attn_decode_fused: 3 qkv slabs, 5 statistics tiles."""
    hq, max_ctx, hid, sk, tiles = HKV * G, 512, 1024, 3, 5
    width = (hq + 2 * HKV) * D
    kc, vc, bt, ctx = _seqs(ctxs, dev)
    bt_wide = torch.zeros(2, max_ctx // BS, dtype=torch.int32, device=dev)
    bt_wide[:, : bt.shape[1]] = bt
    slab = torch.randn(sk, 2, width, device=dev) * 0.6
    ssv = (torch.rand(2, device=dev) + 0.5) * hid
    ssp = torch.zeros(tiles, ops.SSP_LD, device=dev)
    ssp[:, :2] = (ssv / tiles)[None, :]
    slots = torch.tensor([int(bt[i, (c - 1) // BS]) * BS + (c - 1) % BS for i, c in enumerate(ctxs)],
                         dtype=torch.long, device=dev)
    pos = (ctx - 1).long()
    cs = ref.rope_cos_sin(1024, D, 500000.0, dev)
    maxp = ops.decode_partials(max_ctx)
    po = torch.empty(2 * hq * maxp * D, device=dev)
    pm = torch.empty(2 * hq * maxp * 2, device=dev)
    cnt = torch.zeros(2 * HKV, dtype=torch.int32, device=dev)
    kr, vr = kc.clone(), vc.clone()
    scale = 1 / math.sqrt(D)
    out = ops.attn_decode_fused(slab, ssp, pos, cs, slots, kc, vc, bt_wide, ctx, max_ctx, hq, HKV, scale, 1e-5, hid,
                                po, pm, cnt)
    rn = torch.rsqrt(ssv / hid + 1e-5)
    qkv = (slab.sum(0) * rn[:, None]).to(torch.bfloat16)
    ref.rope_and_cache(qkv, pos.cpu(), cs, slots.cpu(), kr, vr, hq, HKV, D)
    cu = torch.arange(3, dtype=torch.int32, device=dev)
    r = ref.attention(qkv[:, : hq * D], kr, vr, bt, cu, ctx, hq, HKV, scale).reshape(2, -1)
    close(out, r, atol=3e-2, rtol=3e-2)
    close(kc, kr, atol=3e-2, rtol=2e-2)
    close(vc, vr, atol=3e-2, rtol=2e-2)
    assert int(cnt.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------- sampling + advance
def test_sample_advance_two_rows(dev):
    """Row 0 greedy from the LM head's candidates, row 1 a top-k / top-p draw (the float64 oracle's token, at a
    draw whose winner leads by far more than fp32 rounding), then the step's advance and the next embedding rows."""
    vocab, tile, bs, width, kmax, hidden = 512, 64, 16, 4, 4, 64
    rng = np.random.default_rng(7)
    lg = torch.tensor(rng.normal(size=(2, vocab)) * 2, dtype=torch.float32).to(torch.bfloat16)
    lg[0, 300] = 9.0
    logits = lg.to(dev)
    tiles = lg.float().view(2, vocab // tile, tile)
    parts = torch.stack([tiles.max(-1).values.view(torch.int32),
                         (tiles.argmax(-1) + torch.arange(0, vocab, tile)).to(torch.int32)], -1).contiguous().to(dev)
    temp = torch.tensor([0.0, 0.7], device=dev)
    topk = torch.tensor([0, 20], dtype=torch.int32, device=dev)
    topp = torch.tensor([1.0, 0.9], device=dev)
    seeds = torch.tensor([11, 12], dtype=torch.long, device=dev)
    state = {"out": torch.zeros(2, dtype=torch.long), "ids": torch.tensor([5, 6]), "pos": torch.tensor([14, 15]),
             "ctx": torch.tensor([15, 16], dtype=torch.int32), "slots": torch.zeros(2, dtype=torch.long),
             "bt": torch.tensor(rng.integers(0, 100, size=(2, width)), dtype=torch.int32),
             "step": torch.tensor([3, 4]), "tokens": torch.full((kmax, 2), -1, dtype=torch.long),
             "cnt": torch.tensor([1], dtype=torch.int32), "n_real": torch.tensor([2], dtype=torch.int32)}
    pred = sr.predict(lg[1], 0.7, 20, float(np.float32(0.9)), [12], [4])
    # fp32 against float64: the kernel's masses and scores are off by ~1e-6 relative, the oracle's margins are 1e-3
    assert pred.gap[0] > 1e-3 and min(pred.margin_hi, pred.margin_lo) > 1e-3, "draw or top-p cut too close: reseed"
    want = dict(state)
    want["out"] = torch.tensor([300, int(pred.token[0])])
    want = sr.advance_model(want, 2, bs)
    d = {k: v.to(dev) for k, v in state.items()}
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    table = torch.randn(vocab, hidden, device=dev).to(torch.bfloat16)
    h_out = torch.zeros(2, hidden, dtype=torch.bfloat16, device=dev)
    ssp_out = torch.zeros(ops.SSP_LD, device=dev)
    ops.sample_advance(logits, temp, topk, topp, seeds, d["step"], d["out"], parts, d["ids"], d["pos"], d["ctx"],
                       d["slots"], d["bt"], d["tokens"], d["cnt"], d["n_real"], bs, ticket,
                       embed=(table, h_out, ssp_out))
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(d[k].cpu(), want[k]), k
    assert int(ticket.item()) == 0
    rows = table[want["ids"].to(dev)]
    assert torch.equal(h_out, rows)
    close(ssp_out[:2], rows.float().pow(2).sum(-1), atol=0, rtol=1e-5)
