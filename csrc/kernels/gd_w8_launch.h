// Host launchers of the W8A16 decode GEMMs (gemm_decode_w8.hip, its wide, its grouped and its wide grouped form). As launchers.h: raw pointers and an explicit stream,
// no allocation, no synchronisation.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.h"

namespace die {

// Y = (X · q^T) ⊙ s for M <= 32 rows. Wq: the e4m3 bytes of q [N, K] packed for the (wr, kc) tile of gd_w8.h
// (src/ops/w8.py gd_pack_weights_w8; mode 1: with silu=True); scales: [N] fp32 in q's row order, 16-byte aligned.
// mode 0: bf16 Y [M, N] (ldy % 4 == 0, 8-byte aligned); mode 1: bf16 Y [M, N / 2] = silu(gate) * up, q = [gate; up];
// mode 2: fp32 slabs Y [sk, M, N] (ldy = N, 16-byte aligned), slice by of sk over the K-chunks
// [by tch / sk, (by + 1) tch / sk). sk = 1 unless mode 2; sk <= K / kc.
// hipErrorInvalidValue (nothing launched) for M > 32, a (wr, kc) that is no GD_W8_TILES tile, K % kc, or N (mode 1:
// N / 2) no multiple of the tile's columns.
hipError_t launch_gemm_decode_w8(void* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                 const float* scales, int M, int N, int K, int mode, int wr, int kc, int sk,
                                 hipStream_t s);

// The wide form (gemm_decode_w8_wide.hip): the same product, operands, packed bytes, modes and split-K rule for
// 33 <= M <= 128 rows (activation images of 64 and 128 rows; geometry in gd_w8_wide.h).
// hipErrorInvalidValue (nothing launched) for M outside [33, 128] and for everything launch_gemm_decode_w8 refuses.
hipError_t launch_gemm_decode_w8_wide(void* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                      const float* scales, int M, int N, int K, int mode, int wr, int kc, int sk,
                                      hipStream_t s);

// The grouped (MoE) form (gemm_decode_w8_grouped.hip): Y[off[e] : off[e + 1]] = (Xrows · q[e]^T) ⊙ s[e] for the E
// groups of offsets [E + 1] (int32, ascending, at most max_rows <= 32 rows each; an empty group reads nothing).
// Wq: [E, N, K] e4m3 bytes, every expert's [N, K] packed for (wr, kc) as above; scales: [E, N] fp32. Y: bf16 [R, N]
// (mode 0) or [R, N / 2] = silu(gate) * up (mode 1). rows null: X is [R, K], image row j of group e is
// X[off[e] + j]; rows [R] int32: X is [T, K] in token order and the row is X[rows[off[e] + j] / k]. The kernel chooses
// the 16- or 32-row image per group; indices read from offsets / rows are clamped to [0, R] / [0, T).
// hipErrorInvalidValue (nothing launched) for max_rows outside [1, 32], a (wr, kc) that is no GD_W8_TILES tile, K % kc,
// or N (mode 1: N / 2) no multiple of the tile's columns.
hipError_t launch_gemm_decode_w8_grouped(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                         const float* scales, const int* offsets, const int* rows, int k, int E, int T,
                                         int R, int N, int K, int mode, int wr, int kc, int max_rows, hipStream_t s);

// The wide grouped form (gemm_decode_w8_grouped_wide.hip): the same product, operands, packed bytes, gather and modes
// for groups of at most max_rows <= 128 rows each. The kernel chooses the 16-, 32-, 64- or 128-row image per group
// (up to 32 rows: the grouped kernel's own body; above: half-chunk slots on gd_w8_wide.h's geometry).
// hipErrorInvalidValue (nothing launched) for max_rows outside [1, 128] and for everything else
// launch_gemm_decode_w8_grouped refuses.
hipError_t launch_gemm_decode_w8_grouped_wide(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                              const float* scales, const int* offsets, const int* rows, int k, int E,
                                              int T, int R, int N, int K, int mode, int wr, int kc, int max_rows,
                                              hipStream_t s);

}  // namespace die
