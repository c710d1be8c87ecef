// "W8": the layout of FP8 (OCP e4m3fn) weights for the W8A16 decode GEMM (gemm_decode_w8.hip; packed by
// src/ops/w8.py, which mirrors this file and is compared with it through csrc/kernels/tests/gd_w8_dump.cpp).
// A quantised projection is W[n, k] = q[n, k] * s[n]: q one e4m3 byte, s one fp32 per output row (a separate
// [N] tensor, not part of this layout).
//
// The bytes are stored per column tile (WR image rows), then per K-chunk (KC columns): a chunk is WR x KC
// contiguous bytes in the order the consumer loop reads them. Wave w takes the chunk's columns
// [w KC / 4, (w + 1) KC / 4) in KC / 128 k-steps of 32; in a k-step its lane (fr = lane & 15, kg = lane >> 4)
// needs, for each 16-row MFMA column tile nt, the 8 weights of image row 16 nt + fr at columns 8 kg + 0..7 of the
// step (the B fragment of v_mfma_f32_16x16x32_bf16). One 16-byte read carries that for the tiles (2 p, 2 p + 1):
//   [w][step][p = nt / 2][lane] 16 B = 8 bytes of tile 2 p, then 8 bytes of tile 2 p + 1
// Each [w][step][p] group is 64 lanes x 16 B = 1 KiB: one LDS-DMA piece, one linear global read, lane-linear in
// LDS, and read back lane-linear by ds_read_b128 - no bank conflict and no swizzle.
// The SiLU form pairs gate and up rows inside a tile: image rows [0, WR / 2) are gate rows, [WR / 2, WR) the
// matching up rows (as gd_pack_weights(..., silu=True)).
// Plain C++17, no HIP constructs: the host compiler reads it too.
#pragma once

#include <cstddef>

// The instantiated (WR, KC) tiles. KC = 256: a slot carries WR x 256 weight bytes, what the bf16 kernel's
// (WR, 128) slot carries.
#define GD_W8_TILES(X) \
  X(32, 256)           \
  X(64, 256)           \
  X(128, 256)

namespace die {
namespace gd {
namespace w8 {

constexpr int RING_BYTES = 147456;  // LDS for the ring (144 KiB of the CU's 160), as the bf16 kernel's
constexpr int MAX_M = 32;           // activation images of 16 and 32 rows
constexpr int MAX_SLOTS = 8;

constexpr int chunk_bytes(int wr, int kc) { return wr * kc; }            // the weight image of a slot
constexpr int slot_bytes(int wr, int xr, int kc) { return wr * kc + xr * kc * 2; }  // + the bf16 X image
constexpr int pieces(int wr, int xr, int kc) { return slot_bytes(wr, xr, kc) / 1024; }  // 1-KiB LDS-DMA pieces

// ring depth: the deepest that fits RING_BYTES, MAX_SLOTS and the 6-bit vmcnt
constexpr int ring_slots(int wr, int xr, int kc) {
  int s = RING_BYTES / slot_bytes(wr, xr, kc);
  if (s > MAX_SLOTS) s = MAX_SLOTS;
  while (s > 2 && (s - 1) * (pieces(wr, xr, kc) / 4) > 63) --s;
  return s;
}

// LDS bytes of a launch: the ring; after the loop the partials red[4][32][WR] fp32 reuse it
constexpr size_t lds_bytes(int wr, int xr, int kc) {
  const size_t ring = (size_t)ring_slots(wr, xr, kc) * slot_bytes(wr, xr, kc);
  const size_t red = (size_t)4 * 32 * wr * 4;
  return ring > red ? ring : red;
}

// a (WR, XR, KC) form exists: whole 16-byte tile pairs, whole k-steps per wave, the pieces split over 4 waves
// with no piece mixing weights and activations, a ring of >= 2 slots
constexpr bool valid(int wr, int xr, int kc) {
  return wr % 32 == 0 && kc % 128 == 0 && (xr == 16 || xr == 32) && (wr * kc / 1024) % 4 == 0 &&
         (xr * kc * 2 / 1024) % 4 == 0 && ring_slots(wr, xr, kc) >= 2 && lds_bytes(wr, xr, kc) <= RING_BYTES;
}

// byte offset in its chunk of the weight at image row r, chunk column k
constexpr int byte_off(int wr, int kc, int r, int k) {
  const int w = k / (kc / 4), step = (k % (kc / 4)) / 32, kg = (k % 32) / 8, nt = r / 16;
  const int group = (w * (kc / 128) + step) * (wr / 32) + nt / 2;
  return (group * 64 + kg * 16 + r % 16) * 16 + (nt & 1) * 8 + k % 8;
}

// where lane `lane` of wave w reads its 16 bytes of k-step `step`, tile pair p
constexpr int read_off(int wr, int kc, int w, int step, int p, int lane) {
  return (((w * (kc / 128) + step) * (wr / 32) + p) * 64 + lane) * 16;
}

// the slice rule of split-K (the bf16 kernel's): slice by of sk takes chunks [by tch / sk, (by + 1) tch / sk)
constexpr int slice_lo(int by, int tch, int sk) { return by * tch / sk; }

}  // namespace w8
}  // namespace gd
}  // namespace die
