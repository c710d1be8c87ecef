"""
"W8": FP8 (OCP e4m3fn) weights for the W8A16 decode GEMM (csrc/kernels/gemm_decode_w8.hip). A quantised
projection is ``W[n, k] = q[n, k] * s[n]``: q one e4m3 byte, s one fp32 scale per output row. This module has the
kernel's tiles and their geometry (a mirror of csrc/kernels/gd_w8.h, compared with it by tests/test_w8_cpu.py), the
packer into the kernel's fragment order with its exact inverse, and the tile choice. The quantiser and the CPU
semantics are in :mod:`src.ops.reference`. Pure torch.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from .reference import dequantize_weights_fp8, quantize_weights_fp8  # noqa: F401  (re-exported)

# the decode GEMM's W8 modes (_C_w8.gemm_decode_w8)
W8_BF16, W8_SILU, W8_SLAB = 0, 1, 2
# The instantiated (wr, kc) tiles, in the order of gd_w8.h's GD_W8_TILES: weight rows per workgroup and K columns
# per LDS ring slot.
W8_TILES = ((32, 256), (64, 256), (128, 256))
W8_MAX_M = 32            # activation images of 16 and 32 rows
W8_IMAGES = (16, 32)
RING_BYTES = 147456      # LDS for the ring (144 KiB)
MAX_SLOTS = 8


def w8_image(m: int) -> int:
    """The activation image of a launch of m rows."""
    return 16 if m <= 16 else 32


def slot_bytes(wr: int, kc: int, xr: int) -> int:
    """A ring slot: the chunk's wr x kc weight bytes, then the bf16 activation image."""
    return wr * kc + xr * kc * 2


def ring_slots_w8(wr: int, kc: int, xr: int) -> int:
    """LDS ring depth: the deepest that fits RING_BYTES, MAX_SLOTS and the 6-bit vmcnt."""
    per_wave = slot_bytes(wr, kc, xr) // 1024 // 4
    s = min(MAX_SLOTS, RING_BYTES // slot_bytes(wr, kc, xr))
    while s > 2 and (s - 1) * per_wave > 63:
        s -= 1
    return s


def lds_bytes_w8(wr: int, kc: int, xr: int) -> int:
    """LDS bytes of one launch: the ring; the fp32 partials [4, 32, wr] reuse it after the loop."""
    return max(ring_slots_w8(wr, kc, xr) * slot_bytes(wr, kc, xr), 4 * 32 * wr * 4)


def w8_tile_valid(wr: int, kc: int, xr: int) -> bool:
    """A (wr, kc) tile has an xr-row form (mirror of gd_w8.h valid)."""
    return (wr % 32 == 0 and kc % 128 == 0 and xr in W8_IMAGES and (wr * kc // 1024) % 4 == 0
            and (xr * kc * 2 // 1024) % 4 == 0 and ring_slots_w8(wr, kc, xr) >= 2
            and lds_bytes_w8(wr, kc, xr) <= RING_BYTES)


def w8_byte_off(wr: int, kc: int, r: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """Byte offset in its chunk of the weight at image row r, chunk column k (gd_w8.h byte_off): wave k // (kc / 4),
    k-step of 32, tile pair, lane (k group of 8, row in the 16-row tile), tile of the pair, byte."""
    w, step, kg, nt = k // (kc // 4), (k % (kc // 4)) // 32, (k % 32) // 8, r // 16
    group = (w * (kc // 128) + step) * (wr // 32) + nt // 2
    return (group * 64 + kg * 16 + r % 16) * 16 + (nt & 1) * 8 + k % 8


def _tile_rows(rows: int, wr: int, silu: bool, device) -> torch.Tensor:
    """Weight row of every (tile, image row): a tile is wr rows, or wr / 2 gate rows then the matching up rows."""
    no = wr // 2 if silu else wr
    n_out = rows // 2 if silu else rows
    t = torch.arange(n_out // no, device=device).view(-1, 1) * no
    j = torch.arange(no, device=device).view(1, no)
    return (torch.cat([t + j, n_out + t + j], 1) if silu else t + j).reshape(-1)


def _chunk_index(wr: int, kc: int, device) -> torch.Tensor:
    """[wr * kc] position in the packed chunk of element (r, k) of the row-major chunk."""
    r = torch.arange(wr, device=device).view(wr, 1)
    k = torch.arange(kc, device=device).view(1, kc)
    return w8_byte_off(wr, kc, r, k).reshape(-1)


def gd_pack_weights_w8(q: torch.Tensor, wr: int, kc: int = 256, silu: bool = False) -> torch.Tensor:
    """Re-lay the e4m3 bytes q [rows, K] (uint8 or float8_e4m3fn) in the W8 kernel's order: column tile, then
    K-chunk, then the chunk's wr x kc bytes in fragment order (gd_w8.h), so that every 1-KiB LDS-DMA piece is one
    linear read. silu: q = [gate; up] and a tile holds wr / 2 gate rows then the matching up rows. The result is a
    uint8 tensor of q's shape; the scales stay a separate [rows] tensor in q's row order."""
    assert (wr, kc) in W8_TILES and q.dim() == 2 and q.element_size() == 1
    rows, k = q.shape
    no = wr // 2 if silu else wr
    assert (rows // 2 if silu else rows) % no == 0 and k % kc == 0 and (not silu or rows % 2 == 0)
    nt, nch = rows // wr, k // kc
    b = q.contiguous().view(torch.uint8)[_tile_rows(rows, wr, silu, q.device)]
    b = b.view(nt, wr, nch, kc).permute(0, 2, 1, 3).reshape(nt, nch, wr * kc)
    out = torch.empty_like(b)
    out[:, :, _chunk_index(wr, kc, q.device)] = b
    return out.view(rows, k)


def gd_unpack_weights_w8(packed: torch.Tensor, wr: int, kc: int = 256, silu: bool = False) -> torch.Tensor:
    """Exact inverse of :func:`gd_pack_weights_w8`: the row-major [rows, K] bytes (uint8)."""
    assert (wr, kc) in W8_TILES and packed.dtype == torch.uint8
    rows, k = packed.shape
    nt, nch = rows // wr, k // kc
    b = packed.contiguous().view(nt, nch, wr * kc)[:, :, _chunk_index(wr, kc, packed.device)]
    b = b.view(nt, nch, wr, kc).permute(0, 2, 1, 3).reshape(rows, k)
    q = torch.empty_like(b)
    q[_tile_rows(rows, wr, silu, packed.device)] = b
    return q


# (N, K, silu) -> (wr, kc, sk): the measured W8 tiles (MI355X, 32 rows, cold weights: bench/micro_gemm_decode.py 32
# --w8, profiles/w8_micro_and_engine.jsonl; us, against the bf16 kernel's tuned tile). Thin evidence: ONE sweep of
# every tile x split in one session on one card, the best of three replays each, never repeated; entries within a
# few per cent of their runner-up may flip on another day. A second sweep should confirm the table before anyone
# tunes on top of it; the 70B rows serve no engine yet (a tensor-parallel FP8 engine is refused).
W8_TILE_CFG = {
    (6144, 4096, False): (128, 256, 4),    # Llama-3-8B qkv      10.96 vs bf16 11.28 (the rule's (32, 256, 1): 16.17)
    (4096, 4096, False): (64, 256, 4),     # 8B o                 7.78 vs 9.00
    (14336, 4096, True): (128, 256, 1),    # 8B gate/up + SiLU   35.24 vs 46.61
    (4096, 14336, False): (128, 256, 8),   # 8B down             18.31 vs 22.24
    (1280, 8192, False): (64, 256, 8),     # 70B TP=8 qkv         6.96 vs 7.75
    (8192, 1024, False): (64, 256, 2),     # 70B TP=8 o           5.10 vs 6.26
    (3584, 8192, True): (32, 256, 1),      # 70B TP=8 gate/up    31.44 vs 26.35: loses
    (8192, 3584, False): (64, 256, 2),     # 70B TP=8 down       11.47 vs 13.29
}


# The wide W8 decode GEMM (csrc/kernels/gemm_decode_w8_wide.hip, geometry in gd_w8_wide.h): 33 to W8_WIDE_MAX_M rows
# on the same packed bytes and tiles, activation images of 64 and 128 rows, ring slots of half a chunk (128 columns).
W8_WIDE_MAX_M = 128
W8_WIDE_IMAGES = (64, 128)
W8_WIDE_GRAIN = 128
# The row buckets above 32 at which an FP8-weight engine runs the wide kernel (CausalLM._w8_path); a bucket not listed
# runs the bf16 kernels on the dequantised weights, as every step above 32 rows did before the wide kernel existed.
# EMPTY, because both buckets measured slower in the engine (MI355X, Llama-3-8B shapes, one wave of batch x (512 -> 128),
# bench/w8_wide_engine_cost.py, profiles/w8_wide_micro_and_engine.jsonl; two engines each, alternating, two waves each):
# batch 64: 0.954 - 0.960 s with the bucket on against 0.898 - 0.919 s with it off (bf16 engine 0.878);
# batch 128: 1.565 - 1.571 s against 1.470 - 1.485 s (bf16 engine 1.465 - 1.471).
# Thin evidence (one session, one card), but the smallest gap (0.035 s, 0.080 s) exceeds the largest spread seen between
# like engines (0.021 s, 0.015 s). (64, 128) switches both on.
W8_WIDE_BUCKETS: tuple = ()


def ring_slots_w8_wide(wr: int, xr: int) -> int:
    """LDS ring depth of the wide kernel, in slots of W8_WIDE_GRAIN columns (mirror of gd_w8_wide.h ring_slots, whose
    static_asserts pin the six values)."""
    slot = wr * W8_WIDE_GRAIN + xr * W8_WIDE_GRAIN * 2
    s = min(MAX_SLOTS, RING_BYTES // slot)
    while s > 2 and (s - 1) * (slot // 1024 // 4) > 63:
        s -= 1
    return s


# (N, K, row bucket) -> sk of the wide kernel's slab launches where a measurement replaced decode_sk_w8's rule. Empty:
# on the Llama-3-8B shapes at the plan's tiles the rule's sk was also the fastest of (1, 2, 4, 8) at 64 and at 128 rows
# (qkv (128, 256) sk 4, o (64, 256) sk 4, down (128, 256) sk 8; one sweep, bench/micro_gemm_decode_large.py --w8).
W8_WIDE_SK_CFG: dict = {}


def decode_sk_w8(n: int, k: int, wr: int, kc: int, sk: int, bucket: int, max_sk: int = 8) -> int:
    """Split-K of a slab projection [n, k] of an FP8 plan at steps of ``bucket`` rows. The plan's tile (wr, kc) is fixed
    (the bytes are packed for it); sk is a launch parameter. Up to 32 rows: the plan's own ``sk``. Above:
    W8_WIDE_SK_CFG's measured entry, else :func:`decode_tile_w8`'s rule on that tile - the sk of (1, 2, 4, 8) that
    brings the grid closest (in log2) to 256 workgroups, the smaller on a tie (a slab is bucket x n fp32 per slice,
    written and read once: it grows with the rows where the weight stream does not)."""
    if bucket <= W8_MAX_M:
        return sk
    c = W8_WIDE_SK_CFG.get((n, k, bucket))
    if c is not None and c <= max_sk:
        return c
    best, score = 1, 1e9
    for cand in (1, 2, 4, 8):
        if cand > max_sk or cand > k // kc:
            continue
        sc = abs(math.log2((n // wr) * cand / 256.0))
        if sc < score - 1e-9:
            best, score = cand, sc
    return best


def gd_pack_experts_w8(q: torch.Tensor, wr: int, kc: int = 256, silu: bool = False) -> torch.Tensor:
    """:func:`gd_pack_weights_w8` per expert: q [E, rows, K] -> the stacked packed images [E, rows, K] (uint8) that
    the grouped W8 GEMM reads, expert e's image at byte e * rows * K."""
    return torch.stack([gd_pack_weights_w8(q[e], wr, kc, silu=silu) for e in range(q.shape[0])])


def gd_unpack_experts_w8(packed: torch.Tensor, wr: int, kc: int = 256, silu: bool = False) -> torch.Tensor:
    """Exact inverse of :func:`gd_pack_experts_w8`."""
    return torch.stack([gd_unpack_weights_w8(packed[e], wr, kc, silu=silu) for e in range(packed.shape[0])])


# (hidden, inter) -> ((wr, kc) of the grouped gate/up + SiLU GEMM, (wr, kc) of the grouped down GEMM): the measured
# tiles of the grouped W8 GEMM (MI355X, cold weights, top-2 of 8 routing from seed 0: bench/micro_gemm_decode.py M moe
# --w8, profiles/w8_moe_micro_and_engine.jsonl; us at 32 / 8 tokens, against the grouped bf16 kernel's tuned tile).
# Thin evidence: ONE sweep of the three tiles in one session on one card, one routing draw per token count, the best
# of five alternating replays each, never repeated. Here the widest tile won by 25 % and more at both token counts,
# so it should not flip; a second sweep should still confirm it before anyone tunes on top of it.
W8_MOE_TILE_CFG = {
    # Mixtral-8x7B: gate/up 188.7 / 181.6 vs bf16 308.6 / 271.7 ((64, 256): 241.5 / 220.8, (32, 256): 352.5 / 308.6);
    #               down     100.0 /  98.4 vs bf16 155.8 / 137.1 ((64, 256): 127.4 / 121.9, (32, 256): 184.8 / 179.4)
    # at 64 / 128 tokens (the wide grouped kernel on the same bytes; profiles/w8_moe_wide_micro_and_engine.jsonl):
    #               gate/up 201.5 / 253.8 vs bf16 342.9 / 449.7 ((64, 256): 259.0 / 339.1, (32, 256): 395.8 / 538.1);
    #               down    109.6 / 161.9 vs bf16 247.6 / 303.6 ((64, 256): 133.3 / 185.5, (32, 256): 199.9 / 269.2)
    # the same tile wins at every token count: the packed bytes serve all of them at their best tile
    (4096, 14336): ((128, 256), (128, 256)),
}
# The largest token count at which ops.moe_apply runs the grouped W8 launches on the experts' FP8 copies: up to W8_MAX_M
# tokens the 32-row grouped kernel, above it the wide grouped one (csrc/kernels/gemm_decode_w8_grouped_wide.hip, groups
# of up to 128 rows on the same packed bytes); above W8_MOE_MAX_T the bf16 grouped GEMM on the dequantised experts.
# 32, 64 or 128; ops.moe_apply reads it here at every call (a decode hipGraph keeps what it read at capture).
# 128, because the engine measured faster with it at both batches (MI355X, Mixtral-8x7B shapes, fp8_experts engines of
# 128 sequences, one wave of batch x (512 -> 128), bench/w8_moe_wide_engine_cost.py,
# profiles/w8_moe_wide_micro_and_engine.jsonl; two engines each, alternating, two waves each; 32 runs what every
# fp8_experts engine ran above 32 tokens before the wide grouped kernel existed):
# batch 64: 2.248 - 2.252 s per wave with 128 against 3.311 - 3.314 s with 32 (28.4 against 19.3 req/s);
# batch 128: 3.462 - 3.479 s against 4.675 - 4.687 s (36.9 against 27.3 req/s).
# Thin evidence (one session, one card), but the smallest gap (1.06 s, 1.20 s) is 60 times the largest spread seen
# between like engines (0.004 s, 0.017 s). Rule: 128 if faster at both batches by more than that spread, 64 if only at
# batch 64, else 32.
W8_MOE_MAX_T = 128
MOE_ACTIVE_EXPERTS = 8   # groups with rows in a decode step, as the rule counts them (Mixtral at batch 32: all 8)


def moe_decode_tiles_w8(hdim: int, inter: int, experts: int = MOE_ACTIVE_EXPERTS):
    """((wr, kc) of the grouped W8 gate/up GEMM, (wr, kc) of the down one) for experts of [2 inter, hdim] and
    [hdim, inter], or None when no W8 tile divides one of them: W8_MOE_TILE_CFG's measured entry, else
    :func:`decode_tile_w8`'s rule (the grid closest in log2 to 256 workgroups, the wider tile on a tie) with the
    grid multiplied by the ``experts`` expected to have rows."""
    c = W8_MOE_TILE_CFG.get((hdim, inter))
    if c is not None:
        return c

    def rule(n, k, silu):
        best, score = None, 1e9
        for wr, kc in reversed(W8_TILES):
            cols = wr // 2 if silu else wr
            if n % cols or k % kc:
                continue
            sc = abs(math.log2((n // cols) * max(1, experts) / 256.0))
            if sc < score - 1e-9:
                best, score = (wr, kc), sc
        return best

    t13, t2 = rule(inter, hdim, True), rule(hdim, inter, False)
    return None if t13 is None or t2 is None else (t13, t2)


def decode_tile_w8(n: int, k: int, silu: bool = False, split: bool = False,
                   max_sk: int = 8) -> Optional[Tuple[int, int, int]]:
    """(wr, kc, sk) of the W8 decode GEMM for an [n, k] projection (silu: n (gate, up) pairs; split: the slab mode,
    split-K allowed): W8_TILE_CFG's measured entry, else the tile of W8_TILES x sk in (1, 2, 4, 8) that divides the
    shape and brings the grid closest (in log2) to 256 workgroups, one per CU; the wider tile wins a tie (the
    activation image is re-read once per column tile: at wr = 32 it is twice the weight bytes). None when no tile
    divides. The rule is not a measurement: on the shapes of the table it chose tiles up to 50 % slower than the best."""
    c = W8_TILE_CFG.get((n, k, silu))
    if c is not None and (split or c[2] == 1) and c[2] <= max_sk:
        return c
    best, score = None, 1e9
    for wr, kc in reversed(W8_TILES):
        cols = wr // 2 if silu else wr
        if n % cols or k % kc:
            continue
        for sk in ((1, 2, 4, 8) if split else (1,)):
            if sk > max_sk or sk > k // kc:
                continue
            sc = abs(math.log2((n // cols) * sk / 256.0))
            if sc < score - 1e-9:
                best, score = (wr, kc, sk), sc
    return best
