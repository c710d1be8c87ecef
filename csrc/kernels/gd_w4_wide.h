// Geometry of the wide grouped W4A16 decode GEMM (gemm_decode_w4_grouped_wide.hip): groups of 33 to 128 activation
// rows on the MXFP4 records of gd_w4.h, in gd_w4.h's layout and for its tiles (GD_W4_TILES, KC = 256). Nothing here
// changes that layout. A record is [w][step][p][lane] x 16 B nibbles, then [w][fr][nt][step] scale bytes, both in
// ascending wave w = 64 columns of K, so the waves {2 h, 2 h + 1} of half h are one contiguous run of either part:
// WR * 64 nibble bytes at h * WR * 64 and 4 WR scale bytes at chunk_bytes + h * 4 WR. This kernel streams the same
// bytes at a grain of GRAIN = 128 columns (half a chunk). src/ops/w4.py mirrors the ring depth (ring_slots_w4_wide).
// Plain C++17, no HIP constructs: the host compiler reads it too.
#pragma once

#include <cstddef>

#include "gd_w4.h"

namespace die {
namespace gd {
namespace w4 {
namespace wide {

constexpr int MIN_M = w4::MAX_M + 1;  // 33: up to w4::MAX_M rows are the 32-row body's
constexpr int MAX_M = 128;        // activation images of 64 and 128 rows
constexpr int KC = 256;           // the layout's chunk
constexpr int GRAIN = 128;        // columns of a ring slot
constexpr int STEPS = GRAIN / 32; // k-steps of 32 per slot, ks = 2 w' + step; every wave runs all of them

constexpr int wimg_bytes(int wr) { return wr * GRAIN / 2; }         // a slot's nibble sub-image
constexpr int scale_bytes(int wr) { return wr * GRAIN / BLOCK; }    // its scale bytes in the record: 4 WR
constexpr int scale_quarter(int wr) { return scale_bytes(wr) / 4; } // what one wave's 4-byte-per-lane piece brings
// a ring slot: the nibble sub-image, the scale area (256 bytes per wave, as gd_w4.h), the bf16 X image (256 B rows)
constexpr int slot_bytes(int wr, int xr) { return wimg_bytes(wr) + SCALE_LDS + xr * GRAIN * 2; }
constexpr int pieces(int wr, int xr) { return (wimg_bytes(wr) + xr * GRAIN * 2) / 1024; }  // 1-KiB LDS-DMA pieces
// vector-memory instructions a wave issues per slot: its share of the 1-KiB pieces and its quarter of the scales
constexpr int per_wave(int wr, int xr) { return pieces(wr, xr) / 4 + 1; }

// ring depth in slots: the deepest that fits RING_BYTES, MAX_SLOTS and the 6-bit vmcnt
constexpr int ring_slots(int wr, int xr) {
  int s = RING_BYTES / slot_bytes(wr, xr);
  if (s > MAX_SLOTS) s = MAX_SLOTS;
  while (s > 2 && (s - 1) * per_wave(wr, xr) > 63) --s;
  return s;
}

// The output split over the 4 waves: 2 column groups of wr / 32 16-column tiles each (WR = 128: one 16-byte group of
// four tiles; WR = 64: half of the only group) times 2 row groups of xr / 32 16-row tiles each.
constexpr int COL_GROUPS = 2;
constexpr int tiles_per_wave(int wr) { return wr / 16 / COL_GROUPS; }

// LDS bytes of a launch: the ring; after the loop the fp32 tile stage[xr][stage_ld] reuses it (rows padded by 4
// floats: the accumulator rows 4 kg + r of a wave's store then spread over the banks, and stay 16-byte aligned)
constexpr int stage_ld(int wr) { return wr + 4; }
constexpr size_t lds_bytes(int wr, int xr) {
  const size_t ring = (size_t)ring_slots(wr, xr) * slot_bytes(wr, xr), stage = (size_t)xr * stage_ld(wr) * 4;
  return ring > stage ? ring : stage;
}

// a (WR, XR) form exists: 2 or 4 tiles per wave out of whole 16-byte groups, whole row tiles per row group, a quarter
// of the scales within one 4-byte-per-lane piece, the 1-KiB pieces split over 4 waves with no piece mixing weights
// and activations, a ring of >= 3 slots under the vmcnt bound
constexpr bool valid(int wr, int xr) {
  return wr % 64 == 0 && (tiles_per_wave(wr) == 2 || tiles_per_wave(wr) == 4) && (xr == 64 || xr == 128) &&
         scale_quarter(wr) % 4 == 0 && scale_quarter(wr) <= 256 && (wimg_bytes(wr) / 1024) % 4 == 0 &&
         (xr * GRAIN * 2 / 1024) % 4 == 0 && ring_slots(wr, xr) >= 3 && (ring_slots(wr, xr) - 1) * per_wave(wr, xr) <= 63 &&
         lds_bytes(wr, xr) <= RING_BYTES;
}

// where a lane reads the 16 bytes of k-step ks (0 .. STEPS - 1 of the slot), tile group p: gd_w4.h's read_off with
// the k-step counted from the slot's first
constexpr int read_off(int wr, int ks, int p, int lane) { return ((ks * (wr / 64) + p) * 64 + lane) * 16; }
// where half h's scale bytes begin in the chunk's record
constexpr int scale_src(int wr, int h) { return chunk_bytes(wr, KC) + h * scale_bytes(wr); }
// where byte b of a half's scale bytes lies in the slot's scale area: wave b / quarter brought it to its 256 bytes
constexpr int scale_lds(int wr, int b) { return b / scale_quarter(wr) * 256 + b % scale_quarter(wr); }
// where lane fr reads the scale bytes [2 (nt - nt0) + step] of its tiles nt0 .. of the slot's wave w' (0 or 1)
constexpr int scale_read(int wr, int wp, int fr, int nt0) {
  return (2 * wp + fr / 8) * 256 + (fr % 8) * (wr / 8) + 2 * nt0;
}

static_assert(read_off(128, 1, 1, 0) == w4::read_off(128, KC, 0, 1, 1, 0) &&
                  read_off(64, 2, 0, 5) + wimg_bytes(64) == w4::read_off(64, KC, 3, 0, 0, 5) &&
                  read_off(128, 3, 1, 63) + wimg_bytes(128) == w4::read_off(128, KC, 3, 1, 1, 63),
              "a slot's nibbles are the first or the second half of gd_w4.h's nibble image");
static_assert(scale_src(128, 0) == w4::scale_off(128, KC, 0, 0) && scale_src(128, 1) == w4::scale_off(128, KC, 0, 4) &&
                  scale_src(64, 1) == w4::scale_off(64, KC, 0, 4),
              "a slot's scales are the first or the second half of gd_w4.h's scale part");
// image row 16 nt + fr, block 4 h + 2 w' + step of the chunk -> the byte the lane reads at scale_read + 2 i + step
static_assert(scale_lds(128, w4::scale_off(128, KC, 16 * 5 + 9, 4 + 2 + 1) - scale_src(128, 1)) ==
                      scale_read(128, 1, 9, 4) + 2 * 1 + 1 &&
                  scale_lds(128, w4::scale_off(128, KC, 16 * 2 + 7, 1) - scale_src(128, 0)) ==
                      scale_read(128, 0, 7, 0) + 2 * 2 + 1 &&
                  scale_lds(64, w4::scale_off(64, KC, 16 * 3 + 15, 4 + 2) - scale_src(64, 1)) ==
                      scale_read(64, 1, 15, 2) + 2 * 1 + 0 &&
                  scale_lds(64, w4::scale_off(64, KC, 16 * 0 + 8, 3) - scale_src(64, 0)) ==
                      scale_read(64, 1, 8, 0) + 2 * 0 + 1,
              "a lane's scale read finds gd_w4.h's [w][fr][nt][step] bytes where the four quarter pieces put them");

// the table of gemm_decode_w4_grouped_wide.hip's comment
static_assert(slot_bytes(128, 128) == 41 * 1024 && ring_slots(128, 128) == 3 && per_wave(128, 128) == 11,
              "(128, 128 rows)");
static_assert(slot_bytes(128, 64) == 25 * 1024 && ring_slots(128, 64) == 5 && per_wave(128, 64) == 7, "(128, 64 rows)");
static_assert(slot_bytes(64, 128) == 37 * 1024 && ring_slots(64, 128) == 3 && per_wave(64, 128) == 10, "(64, 128 rows)");
static_assert(slot_bytes(64, 64) == 21 * 1024 && ring_slots(64, 64) == 6 && per_wave(64, 64) == 6, "(64, 64 rows)");
#define GD_W4_WIDE_TILE(WR, KC_) static_assert(KC_ == KC && valid(WR, 64) && valid(WR, 128), "every GD_W4_TILES tile");
GD_W4_TILES(GD_W4_WIDE_TILE)
#undef GD_W4_WIDE_TILE

}  // namespace wide
}  // namespace w4
}  // namespace gd
}  // namespace die
