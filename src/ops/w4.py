"""
"W4": OCP MXFP4 weights for the grouped W4A16 decode GEMM (csrc/kernels/gemm_decode_w4_grouped.hip). A quantised
projection is ``W[n, k] = e2m1(code[n, k]) * 2^(sb[n, k // 32] - 127)``: a 4-bit code per weight and one e8m0 scale
byte per block of 32 k of a row. This module has the kernel's tiles and their geometry (a mirror of
csrc/kernels/gd_w4.h, compared with it by tests/test_w4_cpu.py), the packer into the kernel's record order with its
exact inverse, and the tile choice. The quantiser and the CPU semantics are in :mod:`src.ops.reference`. Pure torch.
"""

from __future__ import annotations

import math

import torch

from .reference import (W4_BLOCK, W4_MIN_EXP, dequantize_weights_mxfp4,  # noqa: F401  (re-exported)
                        quantize_weights_mxfp4)
from .w8 import MAX_SLOTS, MOE_ACTIVE_EXPERTS, RING_BYTES, _tile_rows

# the grouped GEMM's W4 modes (_C_w4.gemm_decode_w4_grouped)
W4_BF16, W4_SILU = 0, 1
# The instantiated (wr, kc) tiles, in the order of gd_w4.h's GD_W4_TILES: weight rows per workgroup and K columns
# per LDS ring slot. (256, 256) is not built: its 32-row slot is 50 KiB, a ring of 2 slots.
W4_TILES = ((64, 256), (128, 256))
W4_MAX_M = 32            # activation images of 16 and 32 rows
W4_IMAGES = (16, 32)
SCALE_LDS = 1024         # the scale area of a ring slot: 256 bytes per wave
# the wide grouped kernel (_C_w4.gemm_decode_w4_grouped_wide, csrc/kernels/gd_w4_wide.h): groups of up to 128 rows on the
# same packed bytes, in activation images of 64 and 128 rows next to the two above
W4_WIDE_MAX_M = 128
W4_WIDE_IMAGES = (64, 128)


def chunk_bytes(wr: int, kc: int) -> int:
    """The nibble image of a chunk."""
    return wr * kc // 2


def record_bytes(wr: int, kc: int) -> int:
    """A chunk in memory: its nibble image, then its wr * kc / 32 scale bytes."""
    return chunk_bytes(wr, kc) + wr * kc // W4_BLOCK


def row_bytes(k: int) -> int:
    """Packed bytes per weight row."""
    return k // 2 + k // W4_BLOCK


def slot_bytes_w4(wr: int, kc: int, xr: int) -> int:
    """A ring slot: the chunk's nibble image, the scale area, the bf16 activation image."""
    return chunk_bytes(wr, kc) + SCALE_LDS + xr * kc * 2


def per_wave_w4(wr: int, kc: int, xr: int) -> int:
    """Vector-memory instructions a wave issues per chunk: its share of the 1-KiB pieces and its own scale piece."""
    return (chunk_bytes(wr, kc) + xr * kc * 2) // 1024 // 4 + 1


def ring_slots_w4(wr: int, kc: int, xr: int) -> int:
    """LDS ring depth: the deepest that fits RING_BYTES, MAX_SLOTS and the 6-bit vmcnt."""
    s = min(MAX_SLOTS, RING_BYTES // slot_bytes_w4(wr, kc, xr))
    while s > 2 and (s - 1) * per_wave_w4(wr, kc, xr) > 63:
        s -= 1
    return s


def ring_slots_w4_wide(wr: int, xr: int) -> int:
    """LDS ring depth of the wide grouped kernel's xr-row body (mirror of gd_w4_wide.h ring_slots): a slot is half a
    chunk, wr * 64 nibble bytes, the scale area and xr rows of 256 bytes; a wave issues a quarter of the slot's 1-KiB
    pieces and one scale piece."""
    slot = wr * 64 + SCALE_LDS + xr * 256
    per_wave = (wr * 64 + xr * 256) // 1024 // 4 + 1
    s = min(MAX_SLOTS, RING_BYTES // slot)
    while s > 2 and (s - 1) * per_wave > 63:
        s -= 1
    return s


def lds_bytes_w4(wr: int, kc: int, xr: int) -> int:
    """LDS bytes of one launch: the ring; the fp32 partials [4, 32, wr] reuse it after the loop."""
    return max(ring_slots_w4(wr, kc, xr) * slot_bytes_w4(wr, kc, xr), 4 * 32 * wr * 4)


def w4_tile_valid(wr: int, kc: int, xr: int) -> bool:
    """A (wr, kc) tile has an xr-row form (mirror of gd_w4.h valid)."""
    return (wr % 64 == 0 and kc == 256 and xr in W4_IMAGES and 2 * wr <= SCALE_LDS // 4
            and (chunk_bytes(wr, kc) // 1024) % 4 == 0 and (xr * kc * 2 // 1024) % 4 == 0
            and ring_slots_w4(wr, kc, xr) >= 3 and lds_bytes_w4(wr, kc, xr) <= RING_BYTES)


def w4_byte_off(wr: int, kc: int, r: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """Byte offset in its chunk's record of the nibble pair holding the weight at image row r, chunk column k (gd_w4.h
    byte_off): wave k // 64, k-step of 32, group of four tiles, lane (k group of 8, row in the 16-row tile), the tile's
    dword, byte. The nibble is k & 1 (0: low)."""
    w, step, kg, nt = k // (kc // 4), (k % (kc // 4)) // 32, (k % 32) // 8, r // 16
    group = (w * (kc // 128) + step) * (wr // 64) + nt // 4
    return (group * 64 + kg * 16 + r % 16) * 16 + (nt & 3) * 4 + (k % 8) // 2


def w4_scale_off(wr: int, kc: int, r: torch.Tensor, blk: torch.Tensor) -> torch.Tensor:
    """Byte offset in its chunk's record of the scale of image row r, block blk of the chunk (gd_w4.h scale_off):
    after the nibble image, [wave][row in the 16-row tile][tile][k-step]."""
    w, step = blk // (kc // 128), blk % (kc // 128)
    return chunk_bytes(wr, kc) + w * (2 * wr) + ((r % 16) * (wr // 16) + r // 16) * (kc // 128) + step


def _record_index(wr: int, kc: int, device):
    """(position in the record of byte (r, j) of the row-major [wr, kc / 2] code bytes, of scale (r, blk) of the
    row-major [wr, kc / 32] scale bytes), both flattened."""
    r = torch.arange(wr, device=device).view(wr, 1)
    j = torch.arange(kc // 2, device=device).view(1, -1)
    b = torch.arange(kc // W4_BLOCK, device=device).view(1, -1)
    return w4_byte_off(wr, kc, r, 2 * j).reshape(-1), w4_scale_off(wr, kc, r, b).reshape(-1)


def gd_pack_weights_w4(codes: torch.Tensor, sb: torch.Tensor, wr: int, kc: int = 256,
                       silu: bool = False) -> torch.Tensor:
    """Re-lay MXFP4 codes [rows, K / 2] and scale bytes [rows, K / 32] (uint8) in the W4 kernel's order: column tile,
    then K-chunk, then the chunk's record (gd_w4.h): wr * kc / 2 nibble bytes in fragment order, so that every 1-KiB
    LDS-DMA piece is one linear read, then the chunk's scale bytes. A byte keeps its two nibbles. silu: the rows are
    [gate; up] and a tile holds wr / 2 gate rows then the matching up rows. Returns uint8 [rows, K / 2 + K / 32]."""
    assert (wr, kc) in W4_TILES and codes.dtype == torch.uint8 and sb.dtype == torch.uint8
    rows, k = codes.shape[0], codes.shape[1] * 2
    no = wr // 2 if silu else wr
    assert sb.shape == (rows, k // W4_BLOCK) and k % kc == 0 and (not silu or rows % 2 == 0)
    assert (rows // 2 if silu else rows) % no == 0
    nt, nch = rows // wr, k // kc
    perm = _tile_rows(rows, wr, silu, codes.device)
    ci, si = _record_index(wr, kc, codes.device)
    out = torch.empty(nt, nch, record_bytes(wr, kc), dtype=torch.uint8, device=codes.device)
    out[:, :, ci] = codes[perm].view(nt, wr, nch, kc // 2).permute(0, 2, 1, 3).reshape(nt, nch, -1)
    out[:, :, si] = sb[perm].view(nt, wr, nch, kc // W4_BLOCK).permute(0, 2, 1, 3).reshape(nt, nch, -1)
    return out.view(rows, row_bytes(k))


def gd_unpack_weights_w4(packed: torch.Tensor, wr: int, kc: int = 256, silu: bool = False):
    """Exact inverse of :func:`gd_pack_weights_w4`: (codes [rows, K / 2], sb [rows, K / 32])."""
    assert (wr, kc) in W4_TILES and packed.dtype == torch.uint8
    rows, k = packed.shape[0], packed.shape[1] * 32 // 17
    nt, nch = rows // wr, k // kc
    perm = _tile_rows(rows, wr, silu, packed.device)
    ci, si = _record_index(wr, kc, packed.device)
    rec = packed.contiguous().view(nt, nch, record_bytes(wr, kc))
    codes = torch.empty(rows, k // 2, dtype=torch.uint8, device=packed.device)
    codes[perm] = rec[:, :, ci].view(nt, nch, wr, kc // 2).permute(0, 2, 1, 3).reshape(rows, k // 2)
    sb = torch.empty(rows, k // W4_BLOCK, dtype=torch.uint8, device=packed.device)
    sb[perm] = rec[:, :, si].view(nt, nch, wr, kc // W4_BLOCK).permute(0, 2, 1, 3).reshape(rows, k // W4_BLOCK)
    return codes, sb


def gd_pack_experts_w4(codes: torch.Tensor, sb: torch.Tensor, wr: int, kc: int = 256,
                       silu: bool = False) -> torch.Tensor:
    """:func:`gd_pack_weights_w4` per expert: codes [E, rows, K / 2], sb [E, rows, K / 32] -> the stacked packed images
    [E, rows, K / 2 + K / 32] (uint8) that the grouped W4 GEMM reads."""
    return torch.stack([gd_pack_weights_w4(codes[e], sb[e], wr, kc, silu=silu) for e in range(codes.shape[0])])


def gd_unpack_experts_w4(packed: torch.Tensor, wr: int, kc: int = 256, silu: bool = False):
    """Exact inverse of :func:`gd_pack_experts_w4`: (codes [E, rows, K / 2], sb [E, rows, K / 32])."""
    parts = [gd_unpack_weights_w4(packed[e], wr, kc, silu=silu) for e in range(packed.shape[0])]
    return torch.stack([c for c, _ in parts]), torch.stack([s for _, s in parts])


def dequantize_experts_w4(packed: torch.Tensor, wr: int, kc: int = 256, silu: bool = False) -> torch.Tensor:
    """fp32 [E, rows, K] of packed expert images: unpack, then :func:`dequantize_weights_mxfp4`."""
    return dequantize_weights_mxfp4(*gd_unpack_experts_w4(packed, wr, kc, silu=silu))


# (hidden, inter) -> ((wr, kc) of the grouped gate/up + SiLU GEMM, (wr, kc) of the grouped down GEMM): the measured
# tiles of the grouped W4 GEMM (MI355X, cold weights, top-2 of 8 routing from seed 0: bench/micro_gemm_decode.py M moe
# --w4, profiles/w4_moe_micro_and_engine.jsonl; us at 32 / 8 tokens, against the grouped W8 and bf16 kernels at their
# tuned tiles in the same alternation). Thin evidence: ONE sweep of the two tiles in one session on one card, one routing
# draw per token count, the best of five alternating replays each, never repeated. The wider tile won by 20 % and more
# at both token counts; a second sweep should still confirm it before anyone tunes on top of it.
W4_MOE_TILE_CFG = {
    # Mixtral-8x7B: gate/up 141.4 / 135.2 vs W8 187.9 / 181.0 vs bf16 306.5 / 269.4 ((64, 256): 190.3 / 171.0);
    #               down     72.3 /  70.1 vs W8  99.4 /  98.5 vs bf16 156.0 / 137.4 ((64, 256): 100.5 /  98.9)
    (4096, 14336): ((128, 256), (128, 256)),
}
# The largest token count at which ops.moe_apply runs the grouped W4 launches on the experts' MXFP4 copies: up to W4_MAX_M
# tokens the 32-row grouped kernel, above it the wide grouped one (csrc/kernels/gemm_decode_w4_grouped_wide.hip, groups
# of up to 128 rows on the same packed bytes); above W4_MOE_MAX_T the bf16 grouped GEMM on the dequantised experts.
# 128, and not 32, by measurement (Mixtral-8x7B, random weights, one MI355X, one session, mxfp4_experts engines of 128
# sequences, one wave of batch x (512 -> 128), bench/w8_moe_wide_engine_cost.py ... mxfp4_experts,
# profiles/w4_moe_wide_micro_and_engine.jsonl; two engines each, alternating with an fp8_experts engine, two waves each;
# 32 runs what every mxfp4_experts engine ran above 32 tokens before the wide grouped kernel existed):
# batch 64: 1.966 - 1.972 s per wave with 128 against 3.305 - 3.313 s with 32 (32.5 against 19.3 req/s; FP8 experts 2.249
# - 2.257 s); batch 128: 3.321 - 3.329 s against 4.672 - 4.687 s (38.5 against 27.4 req/s; FP8 experts 3.484 - 3.495 s).
# Thin evidence (one session, one card), but the gaps (1.33 s, 1.34 s) are more than 80 times the largest spread seen
# between like engines (0.008 s, 0.015 s). W8_MOE_MAX_T's rule: 128 if faster at both batches by more than that spread,
# 64 if only at batch 64, else 32. At 64 / 128 tokens the kernel itself ((128, 256), us, `M moe --w4`): gate/up 154.0 /
# 209.3 vs W8 199.8 / 252.5 vs bf16 339.5 / 451.2 ((64, 256): 215.6 / 304.9); down 83.4 / 150.3 vs W8 108.3 / 162.1 vs
# bf16 245.3 / 303.6 ((64, 256): 110.5 / 171.1): W4_MOE_TILE_CFG's tile wins at every token count.
W4_MOE_MAX_T = 128


def moe_decode_tiles_w4(hdim: int, inter: int, experts: int = MOE_ACTIVE_EXPERTS):
    """((wr, kc) of the grouped W4 gate/up GEMM, (wr, kc) of the down one) for experts of [2 inter, hdim] and
    [hdim, inter], or None when no W4 tile divides one of them: W4_MOE_TILE_CFG's measured entry, else
    moe_decode_tiles_w8's rule (the grid closest in log2 to 256 workgroups, the wider tile on a tie) with the grid
    multiplied by the ``experts`` expected to have rows."""
    c = W4_MOE_TILE_CFG.get((hdim, inter))
    if c is not None:
        return c

    def rule(n, k, silu):
        best, score = None, 1e9
        for wr, kc in reversed(W4_TILES):
            cols = wr // 2 if silu else wr
            if n % cols or k % kc:
                continue
            sc = abs(math.log2((n // cols) * max(1, experts) / 256.0))
            if sc < score - 1e-9:
                best, score = (wr, kc), sc
        return best

    t13, t2 = rule(inter, hdim, True), rule(hdim, inter, False)
    return None if t13 is None or t2 is None else (t13, t2)
