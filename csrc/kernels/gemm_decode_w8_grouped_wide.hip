// Grouped (MoE) W8A16 decode GEMM for steps of up to 128 tokens: for every expert e with rows in this step
//   Y[off[e] : off[e + 1], :] = (Xrows · q[e]^T) ⊙ s[e]
// Operands, packed expert images (gd_pack_experts_w8, GD_W8_TILES), scales, gather through rows / k, index clamping
// and the two epilogues are gemm_decode_w8_grouped.hip's: the very bytes that serve steps of up to 32 tokens serve
// these. That kernel holds a group in a 16- or 32-row image; a step of 33 to 128 tokens can route up to 128 rows to
// one expert. What is this kernel's own is the row image chosen per group at run time, out of four.
//
// Grid. (N_out / NO, 1, E), 256 threads, one workgroup per CU. Workgroup (bx, e) owns WR image rows of expert e over
// all of K and reads its own M = off[e + 1] - off[e], clamped to [0, 128] and to R. M == 0: it returns before it
// issues any DMA. Then a wave-uniform branch between four instantiations:
//   M <= 16, M <= 32   gd_w8_grouped_dev.h's K-split body, unchanged: a slot is a whole chunk (256 columns), the four
//                      waves split its K, every wave holds every accumulator, the partials meet in LDS.
//   M <= 64, M <= 128  the wide grouped body below, on gd_w8_wide.h's geometry: a slot is HALF a chunk (128 columns:
//                      WR x 128 weight bytes, then XR rows x 256 bytes of bf16 activations), the four waves split the
//                      OUTPUT tile (2 x 2 column x row groups at WR = 128 and 64, 1 x 4 at WR = 32), every wave runs
//                      all of K, and there is no cross-wave reduction: accumulators go through the padded fp32 stage
//                      stage[XR][WR + 4]. ring_slots, slot_bytes, read_off and their static_asserts are the dense wide
//                      kernel's (3 to 7 slots); an activation row's sixteen 16-byte chunks are XOR-ed with the row on
//                      the source address and on the read.
// Why all four: at 64 tokens, top-2 of 8, a group holds 16 rows on average and groups fall on both sides of 16 and 32
// in almost every step; a 64-row image for each would pay four times the activation DMA for most of them. At 128
// tokens the mean is 32. The launch asks for the largest of the four LDS sizes (all within RING_BYTES).
//
// Gather in the DMA addresses, as in the 32-row kernel: the per-lane source pointers of the activation pieces are
// computed once, before the ring is primed (image row j <- token rows[off[e] + j] / k, or sorted row off[e] + j);
// rows past M are clamped to row M - 1 and never written.
#include "common.h"
#include "gd_w8.h"
#include "gd_w8_dev.h"
#include "gd_w8_grouped_dev.h"
#include "gd_w8_launch.h"
#include "gd_w8_wide.h"

namespace die {
namespace gd {
namespace w8 {
namespace wide {

template <int WR, int XR, int EPI>
__device__ __forceinline__ void grouped_body_wide(const Group& g, char* smem) {
  static_assert(valid(WR, XR) && EPI != 2, "a gd_w8_wide.h form; a group has no split-K slab");
  constexpr int S = ring_slots(WR, XR);
  constexpr int WIMG = wimg_bytes(WR);        // bytes of the weight sub-image in a slot
  constexpr int SLOT = slot_bytes(WR, XR);
  constexpr int XROWB = GRAIN * 2;            // bytes per activation row of a slot: sixteen 16-byte chunks
  constexpr int WPIECES = WIMG / 1024;
  constexpr int PER_WAVE = pieces(WR, XR) / 4;  // pieces a wave issues per slot
  constexpr int CG = col_groups(WR), RG = 4 / CG;
  constexpr int NPW = WR / 32 / CG, NTW = 2 * NPW;  // a wave's tile pairs and 16-column MFMA tiles
  constexpr int MTW = XR / 16 / RG;                 // a wave's 16-row MFMA tiles
  constexpr bool SILU = EPI == 1;
  constexpr int NO = SILU ? WR / 2 : WR;      // output columns per workgroup
  static_assert((S - 1) * PER_WAVE <= 63 && S >= 2 && S <= MAX_SLOTS, "vmcnt field is 6 bits");
  static_assert(WPIECES % 4 == 0, "a wave's piece p is a weight piece or an activation piece for all 4 waves");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cg = wave % CG, rg = wave / CG;
  const int bx = blockIdx.x, M = g.M;
  const int n0 = bx * NO;
  const int tch = g.K / KC;
  const int nsl = 2 * tch;  // slots of the group: two per chunk

  // per-lane source of this wave's pieces q = wave + 4 p of slot 0, as byte pointers; the step to the next slot is a
  // constant per piece kind (p < WPIECES / 4: weights, WIMG bytes; else activations, GRAIN elements). An activation
  // piece holds four image rows, gathered here, once: image row j <- token rows[r0 + j] / k, or sorted row r0 + j
  const char* src[PER_WAVE];
#pragma unroll
  for (int p = 0; p < PER_WAVE; ++p) {
    const int q = wave + 4 * p;
    if (4 * p < WPIECES) {
      src[p] = reinterpret_cast<const char*>(g.Wq) + (int64_t)bx * tch * (WR * KC) + q * 1024 + lane * 16;
    } else {
      const int row = 4 * (q - WPIECES) + lane / 16;
      const int lch = (lane % 16) ^ (row & 15);
      const int j = min(row, M - 1);
      const int xrow = g.rows != nullptr ? min(max(g.rows[j] / g.k, 0), g.T - 1) : g.r0 + j;
      src[p] = reinterpret_cast<const char*>(g.X + (int64_t)xrow * g.ldx + lch * 8);
    }
  }
  auto issue = [&](int h) {
    char* slot = smem + (h % S) * SLOT;
#pragma unroll
    for (int p = 0; p < PER_WAVE; ++p) {
      if (4 * p < WPIECES)
        glds16<2>(src[p] + (int64_t)h * WIMG, slot + (wave + 4 * p) * 1024);  // non-temporal
      else
        glds16<0>(src[p] + (int64_t)h * XROWB, slot + (wave + 4 * p) * 1024);
    }
  };

  f4 acc[MTW][NTW];
#pragma unroll
  for (int a = 0; a < MTW; ++a)
#pragma unroll
    for (int b = 0; b < NTW; ++b) acc[a][b] = f4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int h = 0; h < S - 1; ++h)
    if (h < nsl) issue(h);

  const int fr = lane & 15, kg = lane >> 4;
#pragma unroll 1
  for (int h = 0; h < nsl; ++h) {
    if (h + S - 1 < nsl) issue(h + S - 1);
    wait_chunk<S, PER_WAVE>(min(S - 1, nsl - 1 - h));  // the slots issued after h stay in flight
    __builtin_amdgcn_s_barrier();  // every wave's pieces of slot h have landed
    const char* slot = smem + (h % S) * SLOT;
    const char* ximg = slot + WIMG;
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int lch = 4 * st + kg;  // the lane's 16-byte chunk of an activation row
      bf16x8 a[MTW], b[NTW];
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) {
        const int r = 16 * (rg * MTW + mt) + fr;
        a[mt] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(ximg + r * XROWB + 16 * (lch ^ (r & 15))));
      }
#pragma unroll
      for (int p = 0; p < NPW; ++p) {
        const uint4 v = *reinterpret_cast<const uint4*>(slot + read_off(WR, st, cg * NPW + p, lane));
        b[2 * p] = cvt8(v.x, v.y);
        b[2 * p + 1] = cvt8(v.z, v.w);
      }
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // slot h % S is refilled by the next iteration's issue
  }

  // the waves' tiles into stage[XR][LD] fp32 (every DMA has landed and every read is done)
  constexpr int LD = stage_ld(WR);
  float* stage = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)  // C: column lane & 15, row 4 (lane >> 4) + r
        stage[(16 * (rg * MTW + mt) + 4 * kg + r) * LD + 16 * (cg * NTW + nt) + fr] = acc[mt][nt][r];
  __syncthreads();

  // four output columns per thread: one multiply by the row's scale, the epilogue
  constexpr int Q = NO / 4;
  for (int e = tid; e < XR * Q; e += NTH) {
    const int m = e / Q, j = 4 * (e % Q);
    if (m >= M) continue;
    f4 v = *reinterpret_cast<const f4*>(stage + m * LD + j);
    v *= *reinterpret_cast<const f4*>(g.scales + n0 + j);
    if constexpr (SILU) {
      f4 u = *reinterpret_cast<const f4*>(stage + m * LD + NO + j);
      u *= *reinterpret_cast<const f4*>(g.scales + g.N_out + n0 + j);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = silu_mul(v[i], u[i]);
    }
    uint2 o;
    o.x = pack2(v[0], v[1]);
    o.y = pack2(v[2], v[3]);
    *reinterpret_cast<uint2*>(g.Y + (int64_t)m * g.ldy + n0 + j) = o;
  }
}

// off [E + 1]: group e's rows; rows [R] or null; T rows of X, R rows of Y
template <int WR, int KC_, int EPI>
__global__ void __launch_bounds__(NTH) gemm_decode_w8_grouped_wide_kernel(const uint8_t* __restrict__ Wq,
                                                                          const bf16_t* __restrict__ X, int64_t ldx,
                                                                          const float* __restrict__ scales,
                                                                          bf16_t* __restrict__ Y, int64_t ldy,
                                                                          const int* __restrict__ off,
                                                                          const int* __restrict__ rows, int k, int T,
                                                                          int R, int N_out, int K) {
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
    w8::grouped_body<WR, KC_, 16, EPI>(g, smem);
  else if (M <= w8::MAX_M)
    w8::grouped_body<WR, KC_, 32, EPI>(g, smem);
  else if (M <= 64)
    grouped_body_wide<WR, 64, EPI>(g, smem);
  else
    grouped_body_wide<WR, 128, EPI>(g, smem);
}

constexpr size_t max2(size_t a, size_t b) { return a > b ? a : b; }

template <int WR, int KC_, int EPI>
static hipError_t launch_grouped(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                 const float* scales, const int* off, const int* rows, int k, int E, int T, int R,
                                 int N_out, int K, hipStream_t s) {
  if constexpr (!(KC_ == KC && w8::valid(WR, 16, KC_) && w8::valid(WR, 32, KC_) && valid(WR, 64) && valid(WR, 128))) {
    return hipErrorInvalidValue;
  } else {
    constexpr int NO = EPI == 1 ? WR / 2 : WR;
    if (N_out % NO || K % KC || K < KC) return hipErrorInvalidValue;
    // all four bodies live in the kernel: the launch asks for the largest ring
    constexpr size_t lds = max2(max2(w8::lds_bytes(WR, 16, KC_), w8::lds_bytes(WR, 32, KC_)),
                                max2(lds_bytes(WR, 64), lds_bytes(WR, 128)));
    static_assert(lds <= RING_BYTES, "one workgroup per CU");
    const dim3 grid(N_out / NO, 1, E);
    hipLaunchKernelGGL((gemm_decode_w8_grouped_wide_kernel<WR, KC_, EPI>), grid, dim3(NTH), lds, s, Wq, X, ldx, scales,
                       Y, ldy, off, rows, k, T, R, N_out, K);
    return hipGetLastError();
  }
}

}  // namespace wide
}  // namespace w8
}  // namespace gd

hipError_t launch_gemm_decode_w8_grouped_wide(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                              const float* scales, const int* offsets, const int* rows, int k, int E,
                                              int T, int R, int N, int K, int mode, int wr, int kc, int max_rows,
                                              hipStream_t s) {
  using namespace gd::w8::wide;
  if (max_rows < 1 || max_rows > MAX_M || E < 1 || E > 65535 || T < 1 || R < 1 || N <= 0 || K <= 0 ||
      (mode != 0 && mode != 1) || (mode == 1 && N % 2) || (rows != nullptr && k < 1))
    return hipErrorInvalidValue;
  const int n_out = mode == 1 ? N / 2 : N;
#define GD_W8_TILE(WR, KC_)                                                                                         \
  if (wr == WR && kc == KC_) {                                                                                      \
    if (mode == 0) return launch_grouped<WR, KC_, 0>(Y, ldy, X, ldx, Wq, scales, offsets, rows, k, E, T, R, n_out, K, s); \
    return launch_grouped<WR, KC_, 1>(Y, ldy, X, ldx, Wq, scales, offsets, rows, k, E, T, R, n_out, K, s);          \
  }
  GD_W8_TILES(GD_W8_TILE)
#undef GD_W8_TILE
  return hipErrorInvalidValue;
}

}  // namespace die
