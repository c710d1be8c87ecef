// Geometry of the wide W8A16 decode GEMM (gemm_decode_w8_wide.hip): 33 to 128 activation rows on the FP8 weights of
// gd_w8.h, in gd_w8.h's layout and for its tiles (GD_W8_TILES, KC = 256). Nothing here changes that layout: a packed
// chunk is [w][step][p][lane], eight consecutive k-step blocks of WR x 32 bytes in ascending K, so any multiple of 32
// columns is a contiguous sub-image, and this kernel streams the same bytes at a grain of GRAIN = 128 columns (half
// a chunk: four k-step blocks, WR x 128 bytes). src/ops/w8.py mirrors the ring depth (ring_slots_w8_wide).
// Plain C++17, no HIP constructs: the host compiler reads it too.
#pragma once

#include <cstddef>

#include "gd_w8.h"

namespace die {
namespace gd {
namespace w8 {
namespace wide {

constexpr int MIN_M = w8::MAX_M + 1;  // 33: up to w8::MAX_M rows are the 32-row kernel's
constexpr int MAX_M = 128;        // activation images of 64 and 128 rows
constexpr int KC = 256;           // the layout's chunk (split-K slices are whole chunks, slice_lo's rule)
constexpr int GRAIN = 128;        // columns of a ring slot
constexpr int STEPS = GRAIN / 32; // k-steps of 32 per slot; every wave runs all of them

constexpr int wimg_bytes(int wr) { return wr * GRAIN; }                     // a slot's weight sub-image
constexpr int slot_bytes(int wr, int xr) { return wr * GRAIN + xr * GRAIN * 2; }  // + the bf16 X image (256 B rows)
constexpr int pieces(int wr, int xr) { return slot_bytes(wr, xr) / 1024; }  // 1-KiB LDS-DMA pieces

// ring depth in slots: the deepest that fits RING_BYTES, MAX_SLOTS and the 6-bit vmcnt
constexpr int ring_slots(int wr, int xr) {
  int s = RING_BYTES / slot_bytes(wr, xr);
  if (s > MAX_SLOTS) s = MAX_SLOTS;
  while (s > 2 && (s - 1) * (pieces(wr, xr) / 4) > 63) --s;
  return s;
}

// The output split over the 4 waves: col_groups(wr) column groups of wr / 32 / col_groups tile pairs each, times
// 4 / col_groups row groups of xr / 16 / row_groups 16-row tiles each.
constexpr int col_groups(int wr) { return wr >= 64 ? 2 : 1; }

// LDS bytes of a launch: the ring; after the loop the fp32 tile stage[xr][stage_ld] reuses it (rows padded by 4
// floats: the accumulator rows 4 kg + r of a wave's store then spread over the banks, and stay 16-byte aligned)
constexpr int stage_ld(int wr) { return wr + 4; }
constexpr size_t lds_bytes(int wr, int xr) {
  const size_t ring = (size_t)ring_slots(wr, xr) * slot_bytes(wr, xr), stage = (size_t)xr * stage_ld(wr) * 4;
  return ring > stage ? ring : stage;
}

// a (WR, XR) form exists: whole tile pairs per column group, whole row tiles per row group, the pieces split over 4
// waves with no piece mixing weights and activations, a ring of >= 2 slots
constexpr bool valid(int wr, int xr) {
  return wr % (32 * col_groups(wr)) == 0 && (xr == 64 || xr == 128) && (xr / 16) % (4 / col_groups(wr)) == 0 &&
         (wimg_bytes(wr) / 1024) % 4 == 0 && (xr * GRAIN * 2 / 1024) % 4 == 0 && ring_slots(wr, xr) >= 2 &&
         (ring_slots(wr, xr) - 1) * (pieces(wr, xr) / 4) <= 63 && lds_bytes(wr, xr) <= RING_BYTES;
}

// where a lane reads its 16 bytes of k-step `step` (0 .. STEPS - 1 of the slot), tile pair p: gd_w8.h's read_off
// with the k-step counted from the slot's first
constexpr int read_off(int wr, int step, int p, int lane) { return ((step * (wr / 32) + p) * 64 + lane) * 16; }
static_assert(read_off(128, 1, 0, 0) == w8::read_off(128, KC, 0, 1, 0, 0) &&
                  read_off(64, 2, 1, 5) + wimg_bytes(64) == w8::read_off(64, KC, 3, 0, 1, 5),
              "a slot is the first or the second half of gd_w8.h's chunk image");

// the table of gemm_decode_w8_wide.hip's comment
static_assert(slot_bytes(128, 128) == 48 * 1024 && ring_slots(128, 128) == 3, "(128, 128 rows)");
static_assert(slot_bytes(128, 64) == 32 * 1024 && ring_slots(128, 64) == 4, "(128, 64 rows)");
static_assert(slot_bytes(64, 128) == 40 * 1024 && ring_slots(64, 128) == 3, "(64, 128 rows)");
static_assert(slot_bytes(64, 64) == 24 * 1024 && ring_slots(64, 64) == 6, "(64, 64 rows)");
static_assert(slot_bytes(32, 128) == 36 * 1024 && ring_slots(32, 128) == 4, "(32, 128 rows)");
static_assert(slot_bytes(32, 64) == 20 * 1024 && ring_slots(32, 64) == 7, "(32, 64 rows)");
#define GD_W8_WIDE_TILE(WR, KC_) static_assert(KC_ == KC && valid(WR, 64) && valid(WR, 128), "every GD_W8_TILES tile");
GD_W8_TILES(GD_W8_WIDE_TILE)
#undef GD_W8_WIDE_TILE

}  // namespace wide
}  // namespace w8
}  // namespace gd
}  // namespace die
