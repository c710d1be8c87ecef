// Decode-GEMM (gemm_decode.hip) tiles and their LDS geometry, once: the launcher builds its dispatch chain
// from GD_TILES, the bindings their tile check, and src/ops/decode_tiles.py mirrors this file (GD_TILES and
// gd_tile_valid; tests/test_decode_tiles_cpu.py compares the two through csrc/kernels/tests/gd_tiles_dump.cpp).
// Plain C++17, no HIP constructs: the host compiler reads it too.
#pragma once

#include <cstddef>

// The instantiated (WR, KC) tiles: weight rows per workgroup and K elements per LDS ring slot.
#define GD_TILES(X) \
  X(32, 256)        \
  X(48, 256)        \
  X(64, 256)        \
  X(32, 128)        \
  X(48, 128)        \
  X(64, 128)        \
  X(96, 128)        \
  X(112, 128)       \
  X(128, 128)       \
  X(64, 64)         \
  X(128, 64)        \
  X(64, 32)         \
  X(128, 32)

namespace die {
namespace gd {

constexpr int LDS_BYTES = 160 * 1024;  // LDS of a CU
constexpr int RING_BYTES = 147456;     // LDS for the ring (144 KiB; the epilogue scratch reuses it)

// LDS ring depth for a (WR, XR, KC) tile: the deepest that fits RING_BYTES and the 6-bit vmcnt
constexpr int ring_slots(int wr, int xr, int kc) {
  const int slot = (wr + xr) * kc * 2;
  const int per_wave = (wr + xr) / (64 / (kc / 8)) / 4;
  int s = RING_BYTES / slot;
  if (s > 8) s = 8;
  while (s > 2 && (s - 1) * per_wave > 63) --s;
  return s;
}

// LDS bytes of one launch: the ring, and after the loop the partials red[NRED][RR][WR] fp32 + scratch
constexpr size_t gd_lds(int wr, int xr, int kc, int s) {
  const size_t ring = (size_t)s * (wr + xr) * kc * 2;
  const size_t red = (size_t)(xr < 64 && kc >= 128 ? 4 : 1) * (xr < 32 ? 32 : xr) * wr * 4 + 2048;
  return ring > red ? ring : red;
}

// a (WR, XR, KC) tile exists: a ring of >= 2 slots fits, the DMA pieces split evenly over the 4 waves and
// the wave split has work for every wave
constexpr bool gd_valid(int wr, int xr, int kc) {
  const int rpp = 64 / (kc / 8);
  const int s = ring_slots(wr, xr, kc);
  return s >= 2 && (wr + xr) % (4 * rpp) == 0 && xr % rpp == 0 && wr % rpp == 0 &&
         !(xr < 64 && kc < 128 && wr % 64 != 0) && gd_lds(wr, xr, kc, s) <= LDS_BYTES;
}

// ring depth of the half-LDS form (mode 3, fz.half_ring): at most HALF_RING_BYTES so that two workgroups fit on a
// CU (160 KiB of LDS). The TP row-parallel projections use it where the grid is about one workgroup per CU: with
// two resident per CU the whole grid of every GPU is co-resident with room to spare, which the exchange's
// waiting last arrivers need (CustomAllReduce.fused_ok); 0 = no such form
constexpr int HALF_RING_BYTES = 76 * 1024;
constexpr int half_ring_slots(int wr, int xr, int kc) {
  const int s = ring_slots(wr, xr, kc);
  const int h = HALF_RING_BYTES / ((wr + xr) * kc * 2);
  const int r = h < s ? h : s;
  return r >= 2 ? r : 0;
}

}  // namespace gd
}  // namespace die
