// Grouped (MoE) W4A16 decode GEMM on OCP MXFP4 weights: for every expert e with rows in this step
//   Y[off[e] : off[e + 1], :] = Xrows · dequant(q[e])^T
// X bf16, q[e] the e2m1 codes and e8m0 block scales (one per 32 k of a row) of expert e in gd_w4.h's record order (one
// packed [rows, K / 2 + K / 32] image per expert, stacked [E, ...]), fp32 accumulation on v_mfma_f32_16x16x32_bf16. The
// experts' weights are the step's HBM stream; this kernel streams 17 / 32 of a byte per weight, where the grouped W8
// kernel streams one. The skeleton is that kernel's (gemm_decode_w8_grouped.hip's comment has it; the shared device
// helpers are included from gd_w8_dev.h, not copied): grid (N_out / NO, 1, E) of 256 threads, one workgroup per CU, a
// whole-chunk LDS ring fed by global_load_lds under counted waits, the chunk's K split over the four waves and reduced
// through LDS at the end, a 16- or 32-row body chosen per group on the device, the token gather in the DMA source
// addresses, idle experts returning before any DMA, every index read from device memory clamped to its tensor,
// epilogues EPI 0 (bf16) and 1 (SiLU · up, gate and up rows paired inside a tile). What is this kernel's own:
//
// Fragment build. A lane's B fragment of a (tile, k-step) is one dword of eight codes: four
// v_cvt_scalef32_pk_bf16_fp4 (byte_sel 0..3) turn it into the eight bf16 with the block's scale as the instruction's
// operand, 2^e made from the e8m0 byte as uint(byte) << 23 (the quantiser emits neither byte 0 nor 255). A k-step of 32
// is one MX block, so the scale is one value per (tile, k-step) and lane. e2m1 times a power of two is exact in bf16:
// there is no multiply anywhere, and the epilogue has no scale pass.
//
// Scales: a fifth kind of LDS-DMA piece, one per wave. The scale bytes of a chunk are 8 WR bytes, 1 KiB at WR = 128:
// as one more 1-KiB piece the (128, 256) slot would be 16 + 1 + 16 pieces at 32 rows, which does not divide over
// four waves, and the counted wait needs every wave to issue the same number of vector-memory instructions per chunk.
// But the record keeps them as [w][fr][nt][step], so a wave's OWN scales are 2 WR contiguous bytes: each wave brings
// exactly those with one 4-byte-per-lane global_load_lds (256 bytes a wave; at WR = 64 the upper 32 lanes repeat the
// lower ones' dwords into the slack of the wave's 256-byte area). That is per_wave() = pieces / 4 + 1 instructions per
// wave and chunk for every tile and image, it retires in order with the chunk's other pieces under the same vmcnt, and
// it needs no register ring, which a loop that is not unrolled could rotate only by moving registers that still have
// loads in flight. A lane then reads its 2 WR / 16 scale bytes of the chunk with one ds_read (lanes of equal fr
// read the same address: a broadcast).
//
// Slot geometry and the known weak spot. A slot is [nibble image WR * 128][scale area 1 KiB][X image XR * 512]. At
// XR = 32 the activation image is 16 KiB, as large as the weight image at WR = 128 and twice it at WR = 64: half or
// more of the LDS-DMA traffic and of the ring is activations. They come from L2, not HBM, but they halve the depth of
// the weight stream in flight. Measure before changing it (docs/performance.md has what was measured).
#include "common.h"
#include "gd_w4.h"
#include "gd_w4_launch.h"
#include "gd_w4_grouped_dev.h"

namespace die {
namespace gd {
namespace w4 {

// off [E + 1]: group e's rows; rows [R] or null; T rows of X, R rows of Y
template <int WR, int KC, int EPI>
__global__ void __launch_bounds__(NTH) gemm_decode_w4_grouped_kernel(const uint8_t* __restrict__ Wq,
                                                                     const bf16_t* __restrict__ X, int64_t ldx,
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
  g.Wq = Wq + (int64_t)e * img_rows * row_bytes(K);
  g.X = X;
  g.Y = Y + (int64_t)r0 * ldy;
  g.rows = rows != nullptr ? rows + r0 : nullptr;
  g.ldx = ldx;
  g.ldy = ldy;
  g.r0 = r0;
  g.M = M;
  g.k = k;
  g.T = T;
  g.K = K;
  if (M <= 16)
    grouped_body<WR, KC, 16, EPI>(g, smem);
  else
    grouped_body<WR, KC, 32, EPI>(g, smem);
}

template <int WR, int KC, int EPI>
static hipError_t launch_grouped(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                 const int* off, const int* rows, int k, int E, int T, int R, int N_out, int K,
                                 hipStream_t s) {
  static_assert(valid(WR, 16, KC) && valid(WR, 32, KC), "GD_W4_TILES lists tiles with both images");
  constexpr int NO = EPI == 1 ? WR / 2 : WR;
  if (N_out % NO || K % KC || K < KC) return hipErrorInvalidValue;
  // both bodies live in the kernel: the launch asks for the larger ring
  constexpr size_t l16 = lds_bytes(WR, 16, KC), l32 = lds_bytes(WR, 32, KC);
  constexpr size_t lds = l16 > l32 ? l16 : l32;
  const dim3 grid(N_out / NO, 1, E);
  hipLaunchKernelGGL((gemm_decode_w4_grouped_kernel<WR, KC, EPI>), grid, dim3(NTH), lds, s, Wq, X, ldx, Y, ldy, off,
                     rows, k, T, R, N_out, K);
  return hipGetLastError();
}

}  // namespace w4
}  // namespace gd

hipError_t launch_gemm_decode_w4_grouped(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                         const int* offsets, const int* rows, int k, int E, int T, int R, int N, int K,
                                         int mode, int wr, int kc, int max_rows, hipStream_t s) {
  using namespace gd::w4;
  if (max_rows < 1 || max_rows > MAX_M || E < 1 || E > 65535 || T < 1 || R < 1 || N <= 0 || K <= 0 ||
      (mode != 0 && mode != 1) || (mode == 1 && N % 2) || (rows != nullptr && k < 1))
    return hipErrorInvalidValue;
  const int n_out = mode == 1 ? N / 2 : N;
#define GD_W4_TILE(WR, KC)                                                                                   \
  if (wr == WR && kc == KC) {                                                                                \
    if (mode == 0) return launch_grouped<WR, KC, 0>(Y, ldy, X, ldx, Wq, offsets, rows, k, E, T, R, n_out, K, s); \
    return launch_grouped<WR, KC, 1>(Y, ldy, X, ldx, Wq, offsets, rows, k, E, T, R, n_out, K, s);            \
  }
  GD_W4_TILES(GD_W4_TILE)
#undef GD_W4_TILE
  return hipErrorInvalidValue;
}

}  // namespace die
