"""
"P13": the decode GEMM's lossless 13-bit weight layout for its (128, 128) tile (csrc/kernels/gd_p13.h has the
byte-level picture and the kernel's index arithmetic; this is the packer and its exact inverse, pure torch).

A bf16 ``s | e[7:0] | m[6:0]`` is stored as its low byte ``(e & 1) << 7 | m`` raw, its sign bit, and a 4-bit code
for ``h = e >> 1``: 0 for h = 0 (zeros, denormals, e = 1), c = 1..15 for h = base7 + c with one ``base7 =
max(h) - 15`` (clamped at 0) per tensor. A tensor is packable iff every element has h = 0 or base7 < h: 30 binades
below its top exponent pair. Anything else stays in the plain tile order (the caller's fallback, per tensor).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

P13_TILE = (128, 128)       # (wr, kc): the one tile with a P13 kernel
P13_CHUNK_BYTES = 26624     # 16 KiB low bytes + 8 KiB codes + 2 KiB signs per (128 x 128) K-chunk
P13_NUM, P13_DEN = 13, 16   # packed bytes / bf16 bytes


def _tile_rows(rows: int, silu: bool, device) -> torch.Tensor:
    """Weight row of every (tile, image row): a tile is 128 rows, or 64 gate rows then the matching 64 up rows."""
    wr = P13_TILE[0]
    no = wr // 2 if silu else wr
    n_out = rows // 2 if silu else rows
    t = torch.arange(n_out // no, device=device).view(-1, 1) * no
    j = torch.arange(no, device=device).view(1, no)
    return (torch.cat([t + j, n_out + t + j], 1) if silu else t + j).reshape(-1)


def p13_base7(w: torch.Tensor) -> Optional[int]:
    """The tensor's base7, or None when an exponent lies below the window."""
    h = (w.contiguous().view(torch.int16).to(torch.int32) >> 8) & 0x7F
    base7 = max(int(h.max()) - 15, 0)
    return base7 if bool(((h == 0) | (h > base7)).all()) else None


def gd_pack_weights_p13(w: torch.Tensor, wr: int = 128, kc: int = 128,
                        silu: bool = False) -> Optional[Tuple[torch.Tensor, int]]:
    """(packed, base7) of a [rows, K] bf16 projection weight in the P13 layout — tile bx, then K-chunk c,
    contiguous, three planes per chunk — or None when the tensor is not packable. ``packed`` is a bf16-typed
    [rows * 13 / 16, K] tensor (its bytes are the planes); pass it with mode | P13 and ``base7`` to the decode GEMM.
    silu: w = [gate; up], a tile holds 64 gate rows then the matching 64 up rows."""
    assert (wr, kc) == P13_TILE and w.dtype == torch.bfloat16 and w.dim() == 2
    rows, k = w.shape
    no = wr // 2 if silu else wr
    assert (rows // 2 if silu else rows) % no == 0 and k % kc == 0
    base7 = p13_base7(w)
    if base7 is None:
        return None
    nt, nch = rows // wr, k // kc
    # [T, C, nt8, fr, w, kg, j]: image row 16 nt8 + fr, chunk column 32 w + 8 kg + j
    bits = (w[_tile_rows(rows, silu, w.device)].contiguous().view(torch.int16).to(torch.int32) & 0xFFFF)
    bits = bits.reshape(nt, 8, 16, nch, 4, 4, 8).permute(0, 3, 1, 2, 4, 5, 6)
    h = (bits >> 8) & 0x7F
    code = torch.where(h == 0, h, h - base7)
    sign = bits >> 15
    u8 = torch.uint8
    # low: [T, C, w, pair, kg, fr, odd, j]
    low = (bits & 0xFF).reshape(nt, nch, 4, 2, 16, 4, 4, 8).permute(0, 1, 5, 2, 6, 4, 3, 7).to(u8)
    # codes: byte i of a tile's dword = code[i] | code[4 + i] << 4; [T, C, w, quad, kg, fr, nt & 3, i]
    cb = (code[..., :4] | (code[..., 4:] << 4)).reshape(nt, nch, 2, 4, 16, 4, 4, 4).permute(0, 1, 5, 2, 6, 4, 3, 7).to(u8)
    # signs: byte jj of dword nt8 / 4 = sum over (nt8 & 3, half) of s << (7 - 2 (nt8 & 3) - half)
    sh = (7 - 2 * torch.arange(4, device=w.device).view(4, 1, 1) - torch.arange(2, device=w.device).view(1, 2, 1))
    s = sign.reshape(nt, nch, 2, 4, 16, 4, 4, 2, 4)                    # [T, C, dword, n3, fr, w, kg, half, jj]
    s = (s << sh.view(1, 1, 1, 4, 1, 1, 1, 2, 1)).sum(dim=(3, 7))   # [T, C, dword, fr, w, kg, jj]
    sb = s.permute(0, 1, 4, 5, 3, 2, 6).to(u8)                      # [T, C, w, kg, fr, dword, jj]
    packed = torch.cat([low.reshape(nt, nch, -1), cb.reshape(nt, nch, -1), sb.reshape(nt, nch, -1)], 2)
    assert packed.shape[2] == P13_CHUNK_BYTES
    return packed.contiguous().view(torch.bfloat16).view(rows * P13_NUM // P13_DEN, k), base7


def gd_unpack_weights_p13(packed: torch.Tensor, base7: int, wr: int = 128, kc: int = 128,
                          silu: bool = False) -> torch.Tensor:
    """Exact inverse of :func:`gd_pack_weights_p13`: the row-major [rows, K] bf16 weight."""
    assert (wr, kc) == P13_TILE and packed.dtype == torch.bfloat16
    k = packed.shape[1]
    rows = packed.shape[0] * P13_DEN // P13_NUM
    nt, nch = rows // wr, k // kc
    i32 = torch.int32
    raw = packed.contiguous().view(torch.uint8).view(nt, nch, P13_CHUNK_BYTES)
    # back to [T, C, nt8, fr, w, kg, j]
    low = raw[..., :16384].reshape(nt, nch, 4, 4, 4, 16, 2, 8).permute(0, 1, 3, 6, 5, 2, 4, 7).reshape(
        nt, nch, 8, 16, 4, 4, 8).to(i32)
    cb = raw[..., 16384:24576].reshape(nt, nch, 4, 2, 4, 16, 4, 4).permute(0, 1, 3, 6, 5, 2, 4, 7).reshape(
        nt, nch, 8, 16, 4, 4, 4).to(i32)
    code = torch.cat([cb & 0xF, cb >> 4], -1)
    sb = raw[..., 24576:].reshape(nt, nch, 4, 4, 16, 2, 4).to(i32)     # [T, C, w, kg, fr, dword, jj]
    sh = (7 - 2 * torch.arange(4, device=packed.device).view(4, 1) - torch.arange(2, device=packed.device).view(1, 2))
    s = (sb.unsqueeze(-2).unsqueeze(-2) >> sh.view(4, 2, 1)) & 1    # [T, C, w, kg, fr, dword, n3, half, jj]
    sign = s.permute(0, 1, 5, 6, 4, 2, 3, 7, 8).reshape(nt, nch, 8, 16, 4, 4, 8)
    h = torch.where(code == 0, code, code + base7)
    bits = (sign << 15) | (h << 8) | low
    img = bits.permute(0, 2, 3, 1, 4, 5, 6).reshape(rows, k)        # rows in tile order
    bits16 = torch.where(img >= 32768, img - 65536, img).to(torch.int16)
    w = torch.empty(rows, k, dtype=torch.bfloat16, device=packed.device)
    w[_tile_rows(rows, silu, packed.device)] = bits16.view(torch.bfloat16)
    return w
