// Grouped (MoE) W8A16 decode GEMM: for every expert e with rows in this step
//   Y[off[e] : off[e + 1], :] = (Xrows · q[e]^T) ⊙ s[e]
// X bf16, q[e] the e4m3 bytes of expert e in gd_w8.h's fragment order (one packed [rows, K] image per expert, stacked
// [E, rows, K]), s [E, rows] fp32, fp32 accumulation on v_mfma_f32_16x16x32_bf16, the scale multiplied in once at the
// end. The experts' weights are the step's HBM stream (Mixtral-8x7B: ~90 GB in bf16); this kernel streams one byte per
// weight. Conversion, ring, K split over the four waves and the LDS reduction are gemm_decode_w8.hip's (shared
// helpers: gd_w8_dev.h); what is this kernel's own:
//
// Grid. (N_out / NO, 1, E), 256 threads, one workgroup per CU (the ring takes the LDS). Workgroup (bx, e) owns WR
// image rows of expert e (NO = WR output columns, or WR / 2 (gate, up) pairs in the SiLU form) over all of K: the
// group dimension already multiplies the grid, so there is no split-K and no slab epilogue. A workgroup whose group
// is empty returns before it issues any DMA: idle experts read nothing.
//
// Row image per group, at run time. A workgroup reads its own M = off[e + 1] - off[e] and takes the 16-row body
// (MT = 1: half the activation DMA and MFMAs, the deeper ring of ring_slots(WR, 16, KC)) when M <= 16, the 32-row
// body otherwise: a wave-uniform branch between two instantiations of one templated __device__ body. The launch
// asks for the larger of the two LDS sizes. (At 32 tokens, top-2 of 8 experts, a group holds 8 rows on average.)
//
// Gather in the DMA addresses. Image row j of group e is X[rows[off[e] + j] / k] (rows: moe_align's sorted order; the
// gate/up GEMM reads token-order activations) or X[off[e] + j] (no rows: the down GEMM reads the sorted rows the
// gate/up GEMM wrote). The per-lane source pointers of the activation pieces are computed once, before the ring is
// primed, so the index loads are complete before the first counted wait; rows past M are clamped to row M - 1 and
// never written. Output rows are Y[off[e] + j]. Every index read from device memory is clamped to its tensor (a
// group to [0, R] and 32 rows, a gathered token to [0, T)), so a malformed offsets / rows array cannot take an
// access outside X or Y.
//
// Epilogues (EPI): 0 bf16 Y; 1 bf16 silu(g) * u with q[e] = [gate rows; up rows] per tile, as the dense SiLU form.
//
// Group and the templated body are in gd_w8_grouped_dev.h: gemm_decode_w8_grouped_wide.hip (groups of up to 128 rows)
// runs the same body for its groups of up to 32.
#include "common.h"
#include "gd_w8.h"
#include "gd_w8_dev.h"
#include "gd_w8_grouped_dev.h"
#include "gd_w8_launch.h"

namespace die {
namespace gd {
namespace w8 {

// off [E + 1]: group e's rows; rows [R] or null; T rows of X, R rows of Y
template <int WR, int KC, int EPI>
__global__ void __launch_bounds__(NTH) gemm_decode_w8_grouped_kernel(const uint8_t* __restrict__ Wq,
                                                                     const bf16_t* __restrict__ X, int64_t ldx,
                                                                     const float* __restrict__ scales,
                                                                     bf16_t* __restrict__ Y, int64_t ldy,
                                                                     const int* __restrict__ off,
                                                                     const int* __restrict__ rows, int k, int T, int R,
                                                                     int N_out, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int e = blockIdx.z;
  const int r0 = min(max(off[e], 0), R);
  const int M = min(min(off[e + 1], R) - r0, MAX_M);
  if (M <= 0) return;  // an idle expert: no DMA was issued
  const int64_t img_rows = EPI == 1 ? 2 * (int64_t)N_out : N_out;
  Group g;
  g.Wq = Wq + (int64_t)e * img_rows * K;
  g.scales = scales + (int64_t)e * img_rows;
  g.X = X;
  g.Y = Y + (int64_t)r0 * ldy;
  g.rows = rows != nullptr ? rows + r0 : nullptr;
  g.ldx = ldx;
  g.ldy = ldy;
  g.r0 = r0;
  g.M = M;
  g.k = k;
  g.T = T;
  g.N_out = N_out;
  g.K = K;
  if (M <= 16)
    grouped_body<WR, KC, 16, EPI>(g, smem);
  else
    grouped_body<WR, KC, 32, EPI>(g, smem);
}

template <int WR, int KC, int EPI>
static hipError_t launch_grouped(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                 const float* scales, const int* off, const int* rows, int k, int E, int T, int R,
                                 int N_out, int K, hipStream_t s) {
  if constexpr (!(valid(WR, 16, KC) && valid(WR, 32, KC))) {
    return hipErrorInvalidValue;
  } else {
    constexpr int NO = EPI == 1 ? WR / 2 : WR;
    if (N_out % NO || K % KC || K < KC) return hipErrorInvalidValue;
    // both bodies live in the kernel: the launch asks for the larger ring
    constexpr size_t l16 = lds_bytes(WR, 16, KC), l32 = lds_bytes(WR, 32, KC);
    constexpr size_t lds = l16 > l32 ? l16 : l32;
    const dim3 grid(N_out / NO, 1, E);
    hipLaunchKernelGGL((gemm_decode_w8_grouped_kernel<WR, KC, EPI>), grid, dim3(NTH), lds, s, Wq, X, ldx, scales, Y, ldy,
                       off, rows, k, T, R, N_out, K);
    return hipGetLastError();
  }
}

}  // namespace w8
}  // namespace gd

hipError_t launch_gemm_decode_w8_grouped(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                         const float* scales, const int* offsets, const int* rows, int k, int E, int T,
                                         int R, int N, int K, int mode, int wr, int kc, int max_rows, hipStream_t s) {
  using namespace gd::w8;
  if (max_rows < 1 || max_rows > MAX_M || E < 1 || E > 65535 || T < 1 || R < 1 || N <= 0 || K <= 0 ||
      (mode != 0 && mode != 1) || (mode == 1 && N % 2) || (rows != nullptr && k < 1))
    return hipErrorInvalidValue;
  const int n_out = mode == 1 ? N / 2 : N;
#define GD_W8_TILE(WR, KC)                                                                                          \
  if (wr == WR && kc == KC) {                                                                                       \
    if (mode == 0) return launch_grouped<WR, KC, 0>(Y, ldy, X, ldx, Wq, scales, offsets, rows, k, E, T, R, n_out, K, s); \
    return launch_grouped<WR, KC, 1>(Y, ldy, X, ldx, Wq, scales, offsets, rows, k, E, T, R, n_out, K, s);           \
  }
  GD_W8_TILES(GD_W8_TILE)
#undef GD_W8_TILE
  return hipErrorInvalidValue;
}

}  // namespace die
