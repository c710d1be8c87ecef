// Host launchers of the grouped W4A16 decode GEMM (gemm_decode_w4_grouped.hip, gemm_decode_w4_grouped_wide.hip). As launchers.h: raw pointers and an
// explicit stream, no allocation, no synchronisation.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.h"

namespace die {

// Y[off[e] : off[e + 1]] = Xrows · dequant(q[e])^T for the E groups of offsets [E + 1] (int32, ascending, at most
// max_rows <= 32 rows each; an empty group reads nothing). Wq: [E, N, K / 2 + K / 32] bytes, every expert's MXFP4 codes
// and scale bytes packed for the (wr, kc) tile of gd_w4.h (src/ops/w4.py gd_pack_experts_w4; mode 1: with silu=True).
// Y: bf16 [R, N] (mode 0) or [R, N / 2] = silu(gate) * up (mode 1; ldy % 4 == 0, 8-byte aligned). rows null: X is
// [R, K], image row j of group e is X[off[e] + j]; rows [R] int32: X is [T, K] in token order and the row is
// X[rows[off[e] + j] / k]. The kernel chooses the 16- or 32-row image per group; indices read from offsets / rows are
// clamped to [0, R] / [0, T).
// hipErrorInvalidValue (nothing launched) for max_rows outside [1, 32], a (wr, kc) that is no GD_W4_TILES tile, K % kc,
// or N (mode 1: N / 2) no multiple of the tile's columns.
hipError_t launch_gemm_decode_w4_grouped(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                         const int* offsets, const int* rows, int k, int E, int T, int R, int N, int K,
                                         int mode, int wr, int kc, int max_rows, hipStream_t s);

// The same product on the same packed bytes for groups of at most max_rows <= 128 rows each
// (gemm_decode_w4_grouped_wide.hip): the kernel chooses the 16-, 32-, 64- or 128-row image per group. Same arguments,
// same clamping, same refusals with max_rows outside [1, 128].
hipError_t launch_gemm_decode_w4_grouped_wide(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                              const int* offsets, const int* rows, int k, int E, int T, int R, int N,
                                              int K, int mode, int wr, int kc, int max_rows, hipStream_t s);

}  // namespace die
