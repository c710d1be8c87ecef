// The K-split body of the grouped (MoE) W4A16 decode GEMM, shared by gemm_decode_w4_grouped.hip (groups of up to 32
// rows) and gemm_decode_w4_grouped_wide.hip (groups of up to 128 rows, which runs this body for its groups of up to 32):
// the fragment build from MXFP4 codes, what a workgroup knows about its group, and the 16- / 32-row body (a whole-chunk
// ring slot, the four waves splitting a chunk's K, the LDS reduction; gemm_decode_w4_grouped.hip's comment has the
// design). One definition, so the two kernels cannot drift apart. HIP device code only.
#pragma once

#include "common.h"
#include "gd_w4.h"
#include "gd_w8_dev.h"

namespace die {
namespace gd {
namespace w4 {

using w8::bf16x8;
using w8::f4;
using w8::glds16;
using w8::NTH;
using w8::silu_mul;
using w8::wait_chunk;

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// the 4-byte-per-lane LDS-DMA piece: lane l's dword lands at lds_wave_base + 4 l
__device__ __forceinline__ void glds4(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((w8::global_cvoid*)src, (w8::lds_void*)lds_wave_base, 4, 0, 0);
}

// eight e2m1 codes (element 2 j: low nibble of byte j, element 2 j + 1: its high nibble) times `scale` -> the 8 bf16
// of a B fragment
__device__ __forceinline__ bf16x8 cvt8(uint32_t codes, float scale) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 2);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 3);
  return __builtin_bit_cast(bf16x8, uint4{__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b),
                                          __builtin_bit_cast(uint32_t, c), __builtin_bit_cast(uint32_t, d)});
}

// 2^(byte - 127) of byte `i` of a dword of e8m0 scale bytes
__device__ __forceinline__ float e8m0(uint32_t dw, int i) { return __uint_as_float(((dw >> (8 * i)) & 0xffu) << 23); }

// what a workgroup knows once it has read its group: rows [r0, r0 + M) of Y (and of X without a gather)
struct Group {
  const uint8_t* Wq;  // expert e's packed image
  const bf16_t* X;
  bf16_t* Y;          // row r0 of the output
  const int* rows;    // rows + r0, or null: no gather
  int64_t ldx, ldy;
  int r0, M, k, T, K;
};

template <int WR, int KC, int XR, int EPI>
__device__ __forceinline__ void grouped_body(const Group& g, char* smem) {
  static_assert(valid(WR, XR, KC), "a gd_w4.h tile; the X image's swizzle is written for 512-byte rows");
  constexpr int S = ring_slots(WR, XR, KC);
  constexpr int WIMG = chunk_bytes(WR, KC);    // bytes of the nibble image in a slot
  constexpr int REC = record_bytes(WR, KC);    // bytes of a chunk in memory: nibble image, then scales
  constexpr int XOFF = WIMG + SCALE_LDS;       // the X image in a slot
  constexpr int SLOT = slot_bytes(WR, XR, KC);
  constexpr int XROWB = KC * 2;                // bytes per activation row
  constexpr int XCPR = KC / 8;                 // its 16-byte chunks
  constexpr int XRPP = 64 / XCPR;              // activation rows per piece
  constexpr int WPIECES = WIMG / 1024;
  constexpr int PER_WAVE = per_wave(WR, XR, KC);  // vector-memory instructions a wave issues per chunk
  constexpr int PW = PER_WAVE - 1;             // of them 1-KiB pieces
  constexpr int STEPS = KC / 128;              // k-steps of 32 per wave per chunk
  constexpr int NG = WR / 64, NT = WR / 16;    // 16-byte groups of four tiles, 16-column MFMA tiles
  constexpr int MT = XR / 16;                  // 16-row MFMA tiles
  constexpr int SCW = 2 * WR;                  // scale bytes of a wave per chunk
  constexpr int SCL = SCW / 16;                // of a lane: [nt][step]
  constexpr bool SILU = EPI == 1;
  constexpr int NO = SILU ? WR / 2 : WR;       // output columns per workgroup
  static_assert((S - 1) * PER_WAVE <= 63 && S >= 3 && S <= MAX_SLOTS, "vmcnt field is 6 bits");
  static_assert(WPIECES % 4 == 0, "a wave's piece p is a weight piece or an activation piece for all 4 waves");
  static_assert(STEPS == 2 && SCW <= 256 && SCL % 4 == 0, "a lane's scales are whole dwords of [nt][2 steps]");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bx = blockIdx.x, M = g.M;
  const int n0 = bx * NO;
  const int nch = g.K / KC;

  // per-lane source of this wave's pieces q = wave + 4 p of chunk 0, as byte pointers; the step to the next chunk is
  // a constant per piece kind (weights and scales: REC bytes; activations: KC elements). An activation piece's row is
  // gathered here, once: image row j <- token rows[r0 + j] / k, or sorted row r0 + j
  const char* tile0 = reinterpret_cast<const char*>(g.Wq) + (int64_t)bx * nch * REC;
  const char* src[PW];
#pragma unroll
  for (int p = 0; p < PW; ++p) {
    const int q = wave + 4 * p;
    if (4 * p < WPIECES) {
      src[p] = tile0 + q * 1024 + lane * 16;
    } else {
      const int row = XRPP * (q - WPIECES) + lane / XCPR;
      const int lch = (lane % XCPR) ^ (row & 15);
      const int j = min(row, M - 1);
      const int xrow = g.rows != nullptr ? min(max(g.rows[j] / g.k, 0), g.T - 1) : g.r0 + j;
      src[p] = reinterpret_cast<const char*>(g.X + (int64_t)xrow * g.ldx + lch * 8);
    }
  }
  // the wave's own scales: SCW bytes, 4 per lane (lanes past SCW / 4 repeat earlier dwords into the area's slack)
  const char* ssrc = tile0 + WIMG + wave * SCW + (lane % (SCW / 4)) * 4;
  auto issue = [&](int c) {
    char* slot = smem + (c % S) * SLOT;
#pragma unroll
    for (int p = 0; p < PW; ++p) {
      if (4 * p < WPIECES)
        glds16<2>(src[p] + (int64_t)c * REC, slot + (wave + 4 * p) * 1024);  // non-temporal
      else
        glds16<0>(src[p] + (int64_t)c * XROWB, slot + XOFF + (wave + 4 * p - WPIECES) * 1024);
    }
    glds4(ssrc + (int64_t)c * REC, slot + WIMG + wave * 256);
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
    wait_chunk<S, PER_WAVE>(min(S - 1, nch - 1 - c));  // the chunks issued after c stay in flight
    __builtin_amdgcn_s_barrier();  // every wave's pieces of chunk c have landed
    const char* slot = smem + (c % S) * SLOT;
    const char* ximg = slot + XOFF;
    uint32_t sc[SCL / 4];  // the lane's scale bytes of the chunk: byte 2 nt + step
    if constexpr (SCL == 16) {
      const uint4 v = *reinterpret_cast<const uint4*>(slot + WIMG + wave * 256 + fr * SCL);
      sc[0] = v.x, sc[1] = v.y, sc[2] = v.z, sc[3] = v.w;
    } else {
      const uint2 v = *reinterpret_cast<const uint2*>(slot + WIMG + wave * 256 + fr * SCL);
      sc[0] = v.x, sc[1] = v.y;
    }
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
      for (int p = 0; p < NG; ++p) {
        const uint4 v = *reinterpret_cast<const uint4*>(slot + read_off(WR, KC, wave, st, p, lane));
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int nt = 4 * p + i;
          b[nt] = cvt8(d[i], e8m0(sc[nt / 2], 2 * (nt & 1) + st));
        }
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

  // the four waves' partials through LDS (every DMA has landed and every read is done): red[4][XR][WR] fp32
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)  // C: column lane & 15, row 4 (lane >> 4) + r
        red[(wave * XR + 16 * mt + 4 * kg + r) * WR + 16 * nt + fr] = acc[mt][nt][r];
  __syncthreads();

  // four output columns per thread: the partials in wave order, then the epilogue (the scales are in the products)
  constexpr int Q = NO / 4;
  for (int e = tid; e < XR * Q; e += NTH) {
    const int m = e / Q, j = 4 * (e % Q);
    if (m >= M) continue;
    f4 v = *reinterpret_cast<const f4*>(red + m * WR + j);
#pragma unroll
    for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const f4*>(red + (w * XR + m) * WR + j);
    if constexpr (SILU) {
      f4 u = *reinterpret_cast<const f4*>(red + m * WR + NO + j);
#pragma unroll
      for (int w = 1; w < 4; ++w) u += *reinterpret_cast<const f4*>(red + (w * XR + m) * WR + NO + j);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = silu_mul(v[i], u[i]);
    }
    uint2 o;
    o.x = pack2(v[0], v[1]);
    o.y = pack2(v[2], v[3]);
    *reinterpret_cast<uint2*>(g.Y + (int64_t)m * g.ldy + n0 + j) = o;
  }
}

}  // namespace w4
}  // namespace gd
}  // namespace die
