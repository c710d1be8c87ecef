// "W4": the layout of OCP MXFP4 weights for the grouped W4A16 decode GEMM (gemm_decode_w4_grouped.hip; packed by
// src/ops/w4.py, which mirrors this file and is compared with it through csrc/kernels/tests/gd_w4_dump.cpp).
// A quantised projection is W[n, k] = e2m1(code[n, k]) * 2^(sb[n, k / 32] - 127): a 4-bit code per weight (sign << 3 |
// magnitude index into {0, 0.5, 1, 1.5, 2, 3, 4, 6}) and one e8m0 scale byte per block of 32 consecutive k of a row.
//
// The bytes are stored per column tile (WR image rows), then per K-chunk (KC = 256 columns): a chunk is one contiguous
// RECORD of WR * 128 nibble bytes in the order the consumer loop reads them, followed by the chunk's WR * 8 scale
// bytes. The scales are part of the stream: there is no separate tensor, and a packed [rows, K] projection is
// [rows, K / 2 + K / 32] bytes.
//
// Nibble bytes. Wave w takes the chunk's columns [64 w, 64 w + 64) in two k-steps of 32; in a k-step its lane
// (fr = lane & 15, kg = lane >> 4) needs, for each 16-row MFMA column tile nt, the 8 weights of image row 16 nt + fr at
// columns 8 kg + 0..7 of the step (the B fragment of v_mfma_f32_16x16x32_bf16): one dword, element 2 j in the low
// nibble of byte j and element 2 j + 1 in the high one (what v_cvt_scalef32_pk_bf16_fp4 reads with byte_sel j). One
// 16-byte read carries that for the tiles 4 p .. 4 p + 3:
//   [w][step][p = nt / 4][lane] 16 B = the dwords of tiles 4 p, 4 p + 1, 4 p + 2, 4 p + 3
// Each [w][step][p] group is 64 lanes x 16 B = 1 KiB: one LDS-DMA piece, one linear global read, lane-linear in LDS,
// and read back lane-linear by ds_read_b128 - no bank conflict and no swizzle. Hence WR % 64 == 0.
//
// Scale bytes. A k-step of 32 is exactly one MX block of a row, so lane (fr, kg) needs the byte of (row 16 nt + fr,
// block 2 w + step). The chunk's scale bytes are [w][fr][nt][step]: a wave's scales are 2 WR contiguous bytes and a
// lane's scales for the whole chunk one contiguous read of 2 WR / 16 bytes (16 at WR = 128).
//
// The SiLU form pairs gate and up rows inside a tile: image rows [0, WR / 2) are gate rows, [WR / 2, WR) the matching
// up rows (as gd_w8.h).
// Plain C++17, no HIP constructs: the host compiler reads it too.
#pragma once

#include <cstddef>

// The instantiated (WR, KC) tiles. (256, 256) is left out: its 32-row slot is 50 KiB, a ring of 2 slots.
#define GD_W4_TILES(X) \
  X(64, 256)           \
  X(128, 256)

namespace die {
namespace gd {
namespace w4 {

constexpr int RING_BYTES = 147456;  // LDS for the ring (144 KiB of the CU's 160), as the W8 kernels'
constexpr int MAX_M = 32;           // activation images of 16 and 32 rows
constexpr int MAX_SLOTS = 8;
constexpr int BLOCK = 32;           // weights per scale byte
// the scales of a slot in LDS: 256 bytes per wave, the reach of one 4-byte-per-lane LDS-DMA instruction; a wave's
// 2 WR scale bytes are at its start
constexpr int SCALE_LDS = 4 * 256;

constexpr int chunk_bytes(int wr, int kc) { return wr * kc / 2; }        // the nibble image of a chunk
constexpr int scale_bytes(int wr, int kc) { return wr * kc / BLOCK; }    // its scale bytes
constexpr int record_bytes(int wr, int kc) { return chunk_bytes(wr, kc) + scale_bytes(wr, kc); }
constexpr int row_bytes(int k) { return k / 2 + k / BLOCK; }             // packed bytes per weight row
// a ring slot: the nibble image, the scale area, the bf16 X image
constexpr int slot_bytes(int wr, int xr, int kc) { return chunk_bytes(wr, kc) + SCALE_LDS + xr * kc * 2; }
// vector-memory instructions a wave issues per chunk: its share of the 1-KiB pieces and its own scale piece
constexpr int per_wave(int wr, int xr, int kc) { return (chunk_bytes(wr, kc) + xr * kc * 2) / 1024 / 4 + 1; }

// ring depth: the deepest that fits RING_BYTES, MAX_SLOTS and the 6-bit vmcnt
constexpr int ring_slots(int wr, int xr, int kc) {
  int s = RING_BYTES / slot_bytes(wr, xr, kc);
  if (s > MAX_SLOTS) s = MAX_SLOTS;
  while (s > 2 && (s - 1) * per_wave(wr, xr, kc) > 63) --s;
  return s;
}

// LDS bytes of a launch: the ring; after the loop the partials red[4][32][WR] fp32 reuse it
constexpr size_t lds_bytes(int wr, int xr, int kc) {
  const size_t ring = (size_t)ring_slots(wr, xr, kc) * slot_bytes(wr, xr, kc);
  const size_t red = (size_t)4 * 32 * wr * 4;
  return ring > red ? ring : red;
}

// a (WR, XR, KC) form exists: whole 16-byte groups of four tiles, two k-steps per wave, a wave's scales within one
// 4-byte-per-lane piece, the 1-KiB pieces split over 4 waves with no piece mixing weights and activations, a ring of
// >= 3 slots
constexpr bool valid(int wr, int xr, int kc) {
  return wr % 64 == 0 && kc == 256 && (xr == 16 || xr == 32) && 2 * wr <= SCALE_LDS / 4 &&
         (chunk_bytes(wr, kc) / 1024) % 4 == 0 && (xr * kc * 2 / 1024) % 4 == 0 && ring_slots(wr, xr, kc) >= 3 &&
         lds_bytes(wr, xr, kc) <= RING_BYTES;
}

// byte offset in its chunk's record of the nibble pair that holds the weight at image row r, chunk column k
constexpr int byte_off(int wr, int kc, int r, int k) {
  const int w = k / (kc / 4), step = (k % (kc / 4)) / 32, kg = (k % 32) / 8, nt = r / 16;
  const int group = (w * (kc / 128) + step) * (wr / 64) + nt / 4;
  return (group * 64 + kg * 16 + r % 16) * 16 + (nt & 3) * 4 + (k % 8) / 2;
}

// which nibble of that byte: 0 the low one (even columns), 1 the high one
constexpr int nibble_of(int k) { return k & 1; }

// byte offset in its chunk's record of the scale of image row r, block blk = (chunk column) / 32
constexpr int scale_off(int wr, int kc, int r, int blk) {
  const int w = blk / (kc / 128), step = blk % (kc / 128);
  return chunk_bytes(wr, kc) + w * (scale_bytes(wr, kc) / 4) + ((r % 16) * (wr / 16) + r / 16) * (kc / 128) + step;
}

// where lane `lane` of wave w reads its 16 bytes of k-step `step`, tile group p, in a slot
constexpr int read_off(int wr, int kc, int w, int step, int p, int lane) {
  return (((w * (kc / 128) + step) * (wr / 64) + p) * 64 + lane) * 16;
}

}  // namespace w4
}  // namespace gd
}  // namespace die
