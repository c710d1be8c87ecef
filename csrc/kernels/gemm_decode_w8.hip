// W8A16 weight-streaming GEMM for decode steps: Y[M, N] = (X[M, K] · q[N, K]^T) ⊙ s[N], M <= 32.
// X is bf16, q is OCP e4m3fn (one byte per weight, gd_w8.h's layout), s one fp32 scale per output row;
// accumulation is fp32 on v_mfma_f32_16x16x32_bf16. A decode projection is an HBM stream of its weights: this kernel
// streams one byte per weight where gemm_decode.hip streams two, and turns the bytes into bf16 B fragments in
// registers, so the MFMA operands are exactly the e4m3 values and the scale is applied once, in fp32, at the end.
//
// Work split. A workgroup (256 threads, 4 waves) owns WR image rows of q (WR output columns, or WR / 2 (gate, up)
// pairs in the SiLU form) and a 1 / sk slice of K (the bf16 kernel's slice rule, by * tch / sk). K is streamed in
// chunks of KC = 256 columns. The 4 waves split a chunk's K: wave w multiplies columns [64 w, 64 w + 64) (two k-steps
// of 32) for every column tile and every row tile, and the four partial accumulators are summed once through LDS
// after the loop, in the ring's memory.
//
// Data movement. A ring of S LDS slots; a slot holds the chunk's weight image (WR x 256 bytes, already in fragment
// order: gd_w8.h) followed by the bf16 activation image (XR rows x 512 bytes, XR = 16 or 32; 16-byte chunks XOR-ed
// with the row on the source address and on the read). Slots are filled by LDS-DMA (global_load_lds_dwordx4) in
// 1-KiB pieces, piece q of a chunk by wave q % 4: every weight piece is one linear 1-KiB global read, loaded
// non-temporal (each weight byte is read once per step by one CU), and lands lane-linear; the consumer's
// ds_read_b128 reads it back lane-linear, 8 bytes for each of two MFMA column tiles: conflict-free by construction.
// S - 1 chunks are in flight while the landed one is multiplied: the loop waits with a counted s_waitcnt vmcnt(n)
// and a raw s_barrier and never drains to zero before the last chunk.
//
//   tile (WR, KC)   image   slot            S   LDS ring   weight bytes in flight per CU ((S - 1) WR KC)
//   (32, 256)       16      8 + 8 KiB       8   128 KiB    56 KiB
//   (32, 256)       32      8 + 16 KiB      6   144 KiB    40 KiB
//   (64, 256)       16      16 + 8 KiB      6   144 KiB    80 KiB
//   (64, 256)       32      16 + 16 KiB     4   128 KiB    48 KiB
//   (128, 256)      16      32 + 8 KiB      3   120 KiB    64 KiB
//   (128, 256)      32      32 + 16 KiB     3   144 KiB    64 KiB
// One workgroup per CU (the ring takes most of the 160 KiB). The partials red[4][32][WR] fp32 (16 - 64 KiB) fit the
// ring. The geometry above is arithmetic (gd_w8.h). Measured are whole launches only (docs/performance.md: 2.1 - 3.3
// TB/s of weight bytes at 32 rows, where the bf16 kernel moves 4.5 - 5.3: 40 - 80 KiB in flight per CU do not
// saturate HBM). UNMEASURED: the ring depths one by one, the share of the conversion, and the share of the
// activation image (the same size as the bf16 kernel's beside a weight image of half the bytes).
//
// Conversion. Eight e4m3 bytes (two dwords) become eight bf16 (four dwords) with four v_cvt_pk_f32_fp8 and four
// v_perm_b32 that keep the high halves: an e4m3 value has 4 significant bits and an exponent in [-9, 8], so its fp32
// form has zero low mantissa bits and the high half is the exact bf16, for both zeros, every subnormal and every
// normal. No bias is folded into the scale: accumulators hold the true products.
//
// Epilogues (EPI): 0 bf16 Y; 1 bf16 silu(g) * u with q = [gate rows; up rows] (same formula and overflow branch as
// gemm_decode.hip's silu_mul); 2 an fp32 split-K slab Y[by][m][n] for the slab consumers (rope_and_cache_slab,
// fused_add_rms_norm_slab and their kv8 forms). The reduced accumulator is multiplied once by s[n] in fp32 first.
// Rows >= M and columns outside the tile are never written.
#include "common.h"
#include "gd_w8.h"
#include "gd_w8_dev.h"
#include "gd_w8_launch.h"

namespace die {
namespace gd {
namespace w8 {

template <int WR, int KC, int XR, int EPI>
__global__ void __launch_bounds__(NTH) gemm_decode_w8_kernel(const uint8_t* __restrict__ Wq,
                                                             const bf16_t* __restrict__ X, int64_t ldx,
                                                             const float* __restrict__ scales, void* __restrict__ Yv,
                                                             int64_t ldy, int M, int N_out, int K) {
  static_assert(valid(WR, XR, KC) && KC == 256, "a gd_w8.h tile; the X image's swizzle is written for 512-byte rows");
  constexpr int S = ring_slots(WR, XR, KC);
  constexpr int WIMG = chunk_bytes(WR, KC);   // bytes of the weight image in a slot
  constexpr int SLOT = slot_bytes(WR, XR, KC);
  constexpr int XROWB = KC * 2;               // bytes per activation row
  constexpr int XCPR = KC / 8;                // its 16-byte chunks
  constexpr int XRPP = 64 / XCPR;             // activation rows per piece
  constexpr int WPIECES = WIMG / 1024;
  constexpr int PER_WAVE = pieces(WR, XR, KC) / 4;  // pieces a wave issues per chunk
  constexpr int STEPS = KC / 128;             // k-steps of 32 per wave per chunk
  constexpr int NP = WR / 32, NT = WR / 16;   // tile pairs, 16-column MFMA tiles
  constexpr int MT = XR / 16;                 // 16-row MFMA tiles
  constexpr bool SILU = EPI == 1;
  constexpr int NO = SILU ? WR / 2 : WR;      // output columns per workgroup
  static_assert((S - 1) * PER_WAVE <= 63 && S >= 2 && S <= MAX_SLOTS, "vmcnt field is 6 bits");
  static_assert(WPIECES % 4 == 0, "a wave's piece p is a weight piece or an activation piece for all 4 waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bx = blockIdx.x, by = blockIdx.y, sk = gridDim.y;
  const int n0 = bx * NO;
  const int tch = K / KC;
  const int c_lo = slice_lo(by, tch, sk);
  const int nch = slice_lo(by + 1, tch, sk) - c_lo;

  // per-lane source of this wave's pieces q = wave + 4 p of chunk c_lo, as byte pointers; the step to the next chunk
  // is a constant per piece kind (p < WPIECES / 4: weights, WIMG bytes; else activations, KC elements)
  const char* src[PER_WAVE];
#pragma unroll
  for (int p = 0; p < PER_WAVE; ++p) {
    const int q = wave + 4 * p;
    if (4 * p < WPIECES) {
      src[p] = reinterpret_cast<const char*>(Wq) + ((int64_t)bx * tch + c_lo) * WIMG + q * 1024 + lane * 16;
    } else {
      const int row = XRPP * (q - WPIECES) + lane / XCPR;
      const int lch = (lane % XCPR) ^ (row & 15);
      src[p] = reinterpret_cast<const char*>(X + (int64_t)min(row, M - 1) * ldx + (int64_t)c_lo * KC + lch * 8);
    }
  }
  auto issue = [&](int c) {
    char* slot = smem + (c % S) * SLOT;
#pragma unroll
    for (int p = 0; p < PER_WAVE; ++p) {
      if (4 * p < WPIECES)
        glds16<2>(src[p] + (int64_t)c * WIMG, slot + (wave + 4 * p) * 1024);  // non-temporal
      else
        glds16<0>(src[p] + (int64_t)c * XROWB, slot + (wave + 4 * p) * 1024);
    }
  };

  f4 acc[MT][NT];
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = f4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int c = 0; c < S - 1; ++c)
    if (c < nch) issue(c);

  const int fr = lane & 15, kg = lane >> 4;
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    if (c + S - 1 < nch) issue(c + S - 1);
    const int after = min(S - 1, nch - 1 - c);  // chunks issued after c: they stay in flight
    wait_chunk<S, PER_WAVE>(after);
    __builtin_amdgcn_s_barrier();  // every wave's pieces of chunk c have landed
    const char* slot = smem + (c % S) * SLOT;
    const char* ximg = slot + WIMG;
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int lch = 4 * (wave * STEPS + st) + kg;  // the lane's 16-byte chunk of an activation row
      bf16x8 a[MT], b[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int r = 16 * mt + fr;
        a[mt] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(ximg + r * XROWB + 16 * (lch ^ (r & 15))));
      }
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const uint4 v = *reinterpret_cast<const uint4*>(slot + read_off(WR, KC, wave, st, p, lane));
        b[2 * p] = cvt8(v.x, v.y);
        b[2 * p + 1] = cvt8(v.z, v.w);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // slot c % S is refilled by the next iteration's issue
  }

  // the four waves' partials through LDS (every DMA has landed and every read is done): red[4][32][WR] fp32
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)  // C: column lane & 15, row 4 (lane >> 4) + r
        red[(wave * 32 + 16 * mt + 4 * kg + r) * WR + 16 * nt + fr] = acc[mt][nt][r];
  __syncthreads();

  // four output columns per thread: the partials in wave order, one multiply by the row's scale, the epilogue
  constexpr int Q = NO / 4;
  for (int e = tid; e < XR * Q; e += NTH) {
    const int m = e / Q, j = 4 * (e % Q);
    if (m >= M) continue;
    f4 v = *reinterpret_cast<const f4*>(red + m * WR + j);
#pragma unroll
    for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const f4*>(red + (w * 32 + m) * WR + j);
    v *= *reinterpret_cast<const f4*>(scales + n0 + j);
    if constexpr (SILU) {
      f4 u = *reinterpret_cast<const f4*>(red + m * WR + NO + j);
#pragma unroll
      for (int w = 1; w < 4; ++w) u += *reinterpret_cast<const f4*>(red + (w * 32 + m) * WR + NO + j);
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

template <int WR, int KC, int XR, int EPI>
static hipError_t launch_one(void* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq, const float* scales,
                             int M, int N_out, int K, int sk, hipStream_t s) {
  if constexpr (!valid(WR, XR, KC)) {
    return hipErrorInvalidValue;
  } else {
    constexpr size_t lds = lds_bytes(WR, XR, KC);
    const dim3 grid(N_out / (EPI == 1 ? WR / 2 : WR), sk, 1);
    hipLaunchKernelGGL((gemm_decode_w8_kernel<WR, KC, XR, EPI>), grid, dim3(NTH), lds, s, Wq, X, ldx, scales, Y, ldy, M,
                       N_out, K);
    return hipGetLastError();
  }
}

template <int WR, int KC, int EPI>
static hipError_t launch_image(void* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                               const float* scales, int M, int N_out, int K, int sk, hipStream_t s) {
  constexpr int NO = EPI == 1 ? WR / 2 : WR;
  if (N_out % NO || K % KC || K / KC < sk) return hipErrorInvalidValue;
  // the activation image: the smaller of 16 / 32 rows that holds M
  if (M <= 16) return launch_one<WR, KC, 16, EPI>(Y, ldy, X, ldx, Wq, scales, M, N_out, K, sk, s);
  return launch_one<WR, KC, 32, EPI>(Y, ldy, X, ldx, Wq, scales, M, N_out, K, sk, s);
}

}  // namespace w8
}  // namespace gd

hipError_t launch_gemm_decode_w8(void* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                 const float* scales, int M, int N, int K, int mode, int wr, int kc, int sk,
                                 hipStream_t s) {
  using namespace gd::w8;
  if (M <= 0) return hipSuccess;
  if (M > MAX_M || N <= 0 || K <= 0 || sk < 1 || sk > 65535 || (mode != 2 && sk != 1) || (mode == 1 && N % 2))
    return hipErrorInvalidValue;
  const int n_out = mode == 1 ? N / 2 : N;
#define GD_W8_TILE(WR, KC)                                                                             \
  if (wr == WR && kc == KC) {                                                                          \
    switch (mode) {                                                                                    \
      case 0: return launch_image<WR, KC, 0>(Y, ldy, X, ldx, Wq, scales, M, n_out, K, sk, s);          \
      case 1: return launch_image<WR, KC, 1>(Y, ldy, X, ldx, Wq, scales, M, n_out, K, sk, s);          \
      case 2: return launch_image<WR, KC, 2>(Y, ldy, X, ldx, Wq, scales, M, n_out, K, sk, s);          \
      default: return hipErrorInvalidValue;                                                            \
    }                                                                                                  \
  }
  GD_W8_TILES(GD_W8_TILE)
#undef GD_W8_TILE
  return hipErrorInvalidValue;
}

}  // namespace die
