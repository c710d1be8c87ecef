// The wide W8A16 weight-streaming GEMM for decode steps: Y[M, N] = (X[M, K] · q[N, K]^T) ⊙ s[N], 33 <= M <= 128.
// Operands, layout and epilogues are gemm_decode_w8.hip's (X bf16, q e4m3 bytes packed by gd_w8.h for one of
// GD_W8_TILES, s fp32 per output row, fp32 accumulation on v_mfma_f32_16x16x32_bf16, the scale applied once at the
// end): this kernel reads the very same packed bytes. What differs is how the work is split and how the bytes move,
// because the 32-row design does not stretch: there the 4 waves split a chunk's K and each holds every accumulator
// (at 128 rows x 128 columns 256 registers per wave), and a slot holds a whole 256-column chunk (at WR = 128 and 128
// rows 96 KiB: a ring of one).
//
// Work split. A workgroup (256 threads, 4 waves) owns WR image rows of q and a 1 / sk slice of K, as there (by * tch
// / sk over the chunks of 256 columns). The 4 waves split the OUTPUT tile, not K: CG column groups x RG row groups
// (gd_w8_wide.h col_groups), every wave over all of the slice's K:
//   WR   column groups x row groups   a wave's tile at 64 / 128 rows          accumulator registers   conversion
//   128  2 x 2                        64 columns x 32 / 64 rows               32 / 64                 2 x
//   64   2 x 2                        32 columns x 32 / 64 rows               16 / 32                 2 x
//   32   1 x 4                        32 columns x 16 / 32 rows               8 / 16                  4 x
// There is no cross-wave K reduction: a wave's accumulators are final and every output element is one in-order sum
// over its K slice. The price is that waves of different row groups convert the same weight bytes ("conversion":
// how many waves convert each byte). At WR = 128 the split is 2 x 2 and not one tile pair per wave over all rows
// (4 x 1): per k-step of 32 a wave then reads 2 weight and 2 / 4 activation fragments from LDS for its 8 / 16 MFMAs
// where 4 x 1 reads 1 and 4 / 8, and the four waves together read the activation image twice instead of four times
// (16 instead of 32 KiB of LDS reads per 4 KiB of weight bytes at 128 rows), for a conversion done twice, which is
// 16 VALU instructions beside 8 / 16 MFMAs. That is arithmetic; the two splits were not timed against each other.
//
// Data movement. A ring of S LDS slots, filled by LDS-DMA in 1-KiB pieces, piece q of a slot by wave q % 4, exactly
// as in the 32-row kernel (weight pieces linear, non-temporal and lane-linear in LDS; counted s_waitcnt vmcnt(n) and
// a raw s_barrier per slot, never drained before the last one). A slot is HALF a chunk, GRAIN = 128 columns: the
// chunk image's first or last four k-step blocks (WR x 128 contiguous bytes) followed by the bf16 activation image
// (XR rows x 256 bytes, XR = 64 or 128 by decode_bucket(M); a row is sixteen 16-byte chunks, XOR-ed with the row on
// the source address and on the read, so the 16 rows of an A fragment fall into 16 different bank groups).
//   tile, image       slot            S   LDS ring   pieces per wave and slot
//   (128, 128 rows)   16 + 32 KiB     3   144 KiB    12
//   (128, 64)         16 + 16 KiB     4   128 KiB    8
//   (64, 128)         8 + 32 KiB      3   120 KiB    10
//   (64, 64)          8 + 16 KiB      6   144 KiB    6
//   (32, 128)         4 + 32 KiB      4   144 KiB    9
//   (32, 64)          4 + 16 KiB      7   140 KiB    5
// One workgroup per CU. The depths are arithmetic (gd_w8_wide.h asserts them), not measurements. Every workgroup
// streams its own copy of the activation slice through L2: 2 M / WR times its weight bytes, at 128 rows and WR = 128
// twice the weight stream, at WR = 32 eight times. That, and not the weight stream, may be what limits this kernel;
// docs/performance.md has what was measured.
//
// Epilogue. After the loop every DMA has landed and every read is done: the waves put their accumulators into an
// fp32 tile stage[XR][WR + 4] in the ring's memory, and all 256 threads finish four columns each: one multiply by the
// row's scale, then EPI 0 bf16 Y, 1 bf16 silu(g) * u on the paired (gate, up) tile order (image rows [0, WR / 2)
// gate, the rest up; gd_w8_dev.h's silu_mul with its overflow branch), 2 an fp32 split-K slab Y[by][m][n]. Rows >= M
// and columns outside the tile are never written.
#include "common.h"
#include "gd_w8.h"
#include "gd_w8_dev.h"
#include "gd_w8_launch.h"
#include "gd_w8_wide.h"

namespace die {
namespace gd {
namespace w8 {
namespace wide {

template <int WR, int XR, int EPI>
__global__ void __launch_bounds__(NTH) gemm_decode_w8_wide_kernel(const uint8_t* __restrict__ Wq,
                                                                  const bf16_t* __restrict__ X, int64_t ldx,
                                                                  const float* __restrict__ scales,
                                                                  void* __restrict__ Yv, int64_t ldy, int M, int N_out,
                                                                  int K) {
  static_assert(valid(WR, XR), "a gd_w8_wide.h form");
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
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cg = wave % CG, rg = wave / CG;
  const int bx = blockIdx.x, by = blockIdx.y, sk = gridDim.y;
  const int n0 = bx * NO;
  const int tch = K / KC;
  const int c_lo = slice_lo(by, tch, sk);
  const int nsl = 2 * (slice_lo(by + 1, tch, sk) - c_lo);  // slots of the slice: two per chunk

  // per-lane source of this wave's pieces q = wave + 4 p of the slice's first slot, as byte pointers; the step to the
  // next slot is a constant per piece kind (p < WPIECES / 4: weights, WIMG bytes; else activations, GRAIN elements)
  const char* src[PER_WAVE];
#pragma unroll
  for (int p = 0; p < PER_WAVE; ++p) {
    const int q = wave + 4 * p;
    if (4 * p < WPIECES) {
      src[p] = reinterpret_cast<const char*>(Wq) + ((int64_t)bx * tch + c_lo) * (WR * KC) + q * 1024 + lane * 16;
    } else {
      const int row = 4 * (q - WPIECES) + lane / 16;
      const int lch = (lane % 16) ^ (row & 15);
      src[p] = reinterpret_cast<const char*>(X + (int64_t)min(row, M - 1) * ldx + (int64_t)c_lo * KC + lch * 8);
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
    const int after = min(S - 1, nsl - 1 - h);  // slots issued after h: they stay in flight
    wait_chunk<S, PER_WAVE>(after);
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
    v *= *reinterpret_cast<const f4*>(scales + n0 + j);
    if constexpr (SILU) {
      f4 u = *reinterpret_cast<const f4*>(stage + m * LD + NO + j);
      u *= *reinterpret_cast<const f4*>(scales + N_out + n0 + j);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = silu_mul(v[i], u[i]);
    }
    if constexpr (EPI == 2) {
      *reinterpret_cast<f4*>(reinterpret_cast<float*>(Yv) + ((int64_t)by * M + m) * ldy + n0 + j) = v;
    } else {
      uint2 o;
      o.x = pack2(v[0], v[1]);
      o.y = pack2(v[2], v[3]);
      *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(Yv) + (int64_t)m * ldy + n0 + j) = o;
    }
  }
}

template <int WR, int XR, int EPI>
static hipError_t launch_one(void* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq, const float* scales,
                             int M, int N_out, int K, int sk, hipStream_t s) {
  constexpr size_t lds = lds_bytes(WR, XR);
  const dim3 grid(N_out / (EPI == 1 ? WR / 2 : WR), sk, 1);
  hipLaunchKernelGGL((gemm_decode_w8_wide_kernel<WR, XR, EPI>), grid, dim3(NTH), lds, s, Wq, X, ldx, scales, Y, ldy, M,
                     N_out, K);
  return hipGetLastError();
}

template <int WR, int EPI>
static hipError_t launch_image(void* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                               const float* scales, int M, int N_out, int K, int sk, hipStream_t s) {
  constexpr int NO = EPI == 1 ? WR / 2 : WR;
  if (N_out % NO || K % KC || K / KC < sk) return hipErrorInvalidValue;
  // the activation image: the smaller of 64 / 128 rows that holds M (decode_bucket)
  if (M <= 64) return launch_one<WR, 64, EPI>(Y, ldy, X, ldx, Wq, scales, M, N_out, K, sk, s);
  return launch_one<WR, 128, EPI>(Y, ldy, X, ldx, Wq, scales, M, N_out, K, sk, s);
}

}  // namespace wide
}  // namespace w8
}  // namespace gd

hipError_t launch_gemm_decode_w8_wide(void* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                      const float* scales, int M, int N, int K, int mode, int wr, int kc, int sk,
                                      hipStream_t s) {
  using namespace gd::w8::wide;
  if (M < MIN_M || M > MAX_M || N <= 0 || K <= 0 || sk < 1 || sk > 65535 || (mode != 2 && sk != 1) ||
      (mode == 1 && N % 2))
    return hipErrorInvalidValue;
  const int n_out = mode == 1 ? N / 2 : N;
#define GD_W8_TILE(WR, KC_)                                                                       \
  if (wr == WR && kc == KC_) {                                                                    \
    switch (mode) {                                                                               \
      case 0: return launch_image<WR, 0>(Y, ldy, X, ldx, Wq, scales, M, n_out, K, sk, s);         \
      case 1: return launch_image<WR, 1>(Y, ldy, X, ldx, Wq, scales, M, n_out, K, sk, s);         \
      case 2: return launch_image<WR, 2>(Y, ldy, X, ldx, Wq, scales, M, n_out, K, sk, s);         \
      default: return hipErrorInvalidValue;                                                       \
    }                                                                                             \
  }
  GD_W8_TILES(GD_W8_TILE)
#undef GD_W8_TILE
  return hipErrorInvalidValue;
}

}  // namespace die
