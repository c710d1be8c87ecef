// The FP8 KV cache on gfx950: RoPE + cache writers, split-K decode attention and causal prefill attention over a
// paged cache of OCP e4m3 bytes (torch.float8_e4m3fn; gfx950 converts the format natively).
//
// Format. The bf16 pool's layout at one byte per element: [blocks, hkv, block_size, 128]. A stored byte is
// e4m3(x / scale): nearest-even, saturated to +-448 (the hardware conversion does not saturate, so the value is
// clamped in fp32 first; the NaN bytes 0x7f / 0xff are never written). One fp32 scale per layer for K, one for V.
// The writers convert the fp32 value they hold after the rotation and the row scale: nothing is rounded through bf16.
// The readers dequantise to bf16 (exact: e4m3 has 3 mantissa bits, bf16 7, and its exponent range is inside bf16's)
// and feed the v_mfma_f32_32x32x16_bf16 products of attention.hip; Q, P and the accumulators are as there.
// k_scale is folded into the softmax scale (scores are linear in K), v_scale into the final 1 / l.
//
// Decode (attn_decode_kv8_kernel), designed for 128-byte rows:
//  * Work split as attn_decode_v3: one workgroup per CU walks (sequence, kv head, part) tasks; a part that is not the
//    whole context writes an fp32 partial, draws a ticket, and the last arriver merges (same part_o / part_ml /
//    counters buffers, so an engine holds one set for both cache types).
//  * Chunk, ring, part. A 128-key chunk of K + V is 32 KiB here (64 KiB in bf16). The chunk stays at 128 keys, so
//    that a wave still owns 32 keys of it and the task count (CUs busy at small batches) is that of the bf16 kernel;
//    a part is again cpp = ceil(parts x pairs / grid) chunks from the static bound, at least ONE chunk (128 keys,
//    32 KiB): halving the minimum part's bytes costs a merge per 32 KiB instead of per 64 KiB, but at few pairs the
//    number of CUs streaming is what bounds the step, not the merge. What changes is the ring: THREE 32 KiB buffers,
//    two chunks (64 KiB, the bytes the bf16 kernel keeps in flight per CU) issued ahead of the one being computed.
//    LDS: 3 x 32 KiB ring + 17 KiB merge area + 2 KiB q image = 115 KiB, one workgroup per CU.
//  * Data path. K and V rows move global -> LDS by LDS-DMA (global_load_lds_dwordx4, optionally with the once-read
//    policy): one instruction fills 8 rows of 128 B, a wave's 4 + 4 instructions fill exactly the 32 K and 32 V rows
//    it computes on, so waves run decoupled between task boundaries (counted vmcnt waits: 16 / 8 / 0 for two / one /
//    no chunk in flight behind the current one).
//  * Swizzle (K and V alike): 16-byte chunk c of row r sits at physical chunk c ^ ((r >> 1) & 7), applied to the
//    per-lane SOURCE address since the DMA's LDS side is lane-linear. 256 B of banks hold two rows, so rows of equal
//    parity collide: the XOR spreads 8 such rows over the 8 chunk positions. K: a 16-lane group of ds_read_b128 (16
//    rows, one logical chunk) hits 16 distinct 16-byte slots. V: a ds_read_b64_tr_b8 reads 16 keys x 2 chunks, every
//    slot exactly twice (512 B, two passes: the minimum).
//  * K fragments: lane (key = lane & 31, h = lane >> 5) reads chunk 2j + h (16 dims) and feeds it to TWO MFMA steps;
//    the contraction order over the head dim is free, so step 2j + e contracts dims 32j + 16h + 8e + [0, 8) and the
//    Q fragment of that step is loaded to match (16-byte chunk 4j + 2h + e of the bf16 query row).
//  * V^T fragments: ds_read_b64_tr_b8. In a 16-lane group lane i supplies 8 bytes of row i >> 1 (column half i & 1)
//    and receives column i of the 8 rows: with row j -> key 16 s2 + 4h + (j & 3) + 8 (j >> 2) that is exactly the
//    key order of the P fragment (the S^T accumulator layout), one read per MFMA instead of the bf16 image's two.
//
// Fused prologue (attn_decode_kv8_kernel<G, FUSED = true>): the semantics of attn_decode_v3_kernel<G, true> with an
// e4m3 cache. q and the step's new K / V row are not read from a rotated qkv tensor: they are built here from the qkv
// projection's fp32 split-K slabs (summed in index order from +0, as v3's slab_sum, so the fp32 values are that
// path's), scaled by rn = rsqrt(sum(statistics tiles) * inv_n + eps) and rotated at position ctx - 1. The q rows are
// rounded to bf16 once into the q image; the new K / V are quantised from the fp32 values (sat + quant4, the writers'
// rule: nothing goes through bf16), stored to the paged cache (slot < 0, a padded graph row: not stored) and patched
// into this step's LDS image of the chunk that holds key ctx - 1, so the step attends to the bytes later steps read.
// The RMSNorm and RoPE + KV-write launches and the bf16 q round trip of the slab path disappear. The design:
//  * LDS plan. The staging (slab rows of 512 B: [split][q head], then [split][k, v]; behind them 1 KiB of statistics
//    tiles and the RoPE row) gets an area of ITS OWN behind the q image: 27 KiB, v3's limit, so the qkv split-K plan
//    and the engine's size clause are those of the bf16 pool; 115 + 27 = 142 KiB of 160. v3 has to overlay its
//    staging on the merge area; here nothing else ever lives in it, which buys this at a task boundary: a wave that
//    leaves a task's merge issues the next task's prologue DMA at once, BEFORE the barrier that hands over the ring
//    and the merge area, while slower waves still read (m, l, O) or merge the parts. (Every wave's staging reads lie
//    before the merge's first barrier, so the staging itself needs none.) The gain is unmeasured: at one task per
//    workgroup, the flagship shape, there is no boundary.
//  * DMA order and counted waits. Per wave: its share of the slab rows (two rows per instruction), wave 0 the tiles,
//    wave 1 the RoPE row, then chunk c0 (8 instructions) and chunk c0 + 1 (8). The prologue waits on vmcnt(16) (8
//    where the part has one chunk): the small operands have landed, both chunks stay in flight, and the chunk
//    loop's 16 / 8 / 0 are unchanged. The prologue itself touches memory only through LDS (inline asm reads tied to
//    their own lgkmcnt waits), so no ordinary vector load puts a vmcnt(0) in front of the chunk stream. v3 holds its
//    second 64 KiB chunk back until the prologue is done; here BOTH 32 KiB chunks are issued ahead of the prologue:
//    64 KiB per CU is what v3 has in flight at that point, and the small operands sit in front of them in the queue.
//    That choice is UNMEASURED on the e4m3 kernel.
//  * Who builds what: an item is 4 consecutive dims, a 16-byte LDS read per slab. Lanes [0, 16 G) of waves 0 - 1 each
//    rotate 4 dims and their 4 partners of one q row (two 8-byte q-image stores); in wave 3, which has no q item at
//    any G, 16 lanes do the same for the new key and 16 more take the same two groups of 4 value dims, unrotated
//    (two dwords of e4m3 per lane; no byte-per-thread store anywhere). The dwords stay in
//    registers until the last chunk of the part has landed (vmcnt(0), then a workgroup barrier: the row may be
//    another wave's DMA); there each dword is ONE cache store and ONE LDS patch store, at 16-byte chunk
//    (d >> 4) ^ ((rr >> 1) & 7), byte d & 15 of row rr = (ctx - 1) & 127. The cache stores come after the part's last
//    counted wait, so they never sit in front of one. A part that does not hold key ctx - 1 stages only the q rows.
//
// Prefill (attn_prefill_kv8_kernel): attn_prefill_kernel's pipeline (register-staged double-buffered K/V stages, the
// padded bf16 LDS image, lazy-rescale softmax, XCD remap, LDS-staged epilogue) with a new staging role: a key row
// is 8 chunks of 16 B (8 lanes per row, 8 NW rows per pass), held as bytes in the two register sets (half the
// registers) and widened to 32 B of bf16 when the stage is stored to LDS.
#include <algorithm>

#include "attn_common.h"
#include "common.h"
#include "kv8.h"

namespace die {

using namespace attn;

namespace kv8 {

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;
constexpr float E4M3_MAX = 448.f;

// 4 e4m3 bytes -> 2 packed bf16 pairs; 8 bytes -> one MFMA fragment (exact)
__device__ __forceinline__ uint2 widen4(uint32_t w) {
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  return make_uint2(pack2(lo[0], lo[1]), pack2(hi[0], hi[1]));
}
__device__ __forceinline__ bf16x8_t widen8(uint32_t a, uint32_t b) {
  const uint2 x = widen4(a), y = widen4(b);
  return as_frag(make_uint4(x.x, x.y, y.x, y.y));
}

// fp32 -> e4m3 bytes: clamp (NaN goes to -448: fmaxf / fminf return the other operand), then the packed
// nearest-even conversion
__device__ __forceinline__ float sat(float x) { return fminf(fmaxf(x, -E4M3_MAX), E4M3_MAX); }
__device__ __forceinline__ uint32_t quant4(const float* f, float scale) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(sat(f[0] / scale), sat(f[1] / scale), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(sat(f[2] / scale), sat(f[3] / scale), w, true);
  return (uint32_t)w;
}
__device__ __forceinline__ uint4 quant16(const float* f, float scale) {
  return make_uint4(quant4(f, scale), quant4(f + 4, scale), quant4(f + 8, scale), quant4(f + 12, scale));
}

__device__ __forceinline__ void ld16f(const float* p, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(f + 4 * i) = *reinterpret_cast<const float4*>(p + 4 * i);
}
__device__ __forceinline__ void ld16bf(const bf16_t* p, float* f) {
  unpack8(*reinterpret_cast<const uint4*>(p), f);
  unpack8(*reinterpret_cast<const uint4*>(p + 8), f + 8);
}
__device__ __forceinline__ void st16bf(bf16_t* p, const float* f) {
  *reinterpret_cast<uint4*>(p) = pack8(f);
  *reinterpret_cast<uint4*>(p + 8) = pack8(f + 8);
}

constexpr int HALF = D / 2;
constexpr int RC = HALF / 16;  // rotation items per head: 16 dims and their 16 partners, two 16-byte cache stores
constexpr int VC = D / 16;     // value items per head: one 16-byte cache store

// the rotation of rope_cache_kernel on a 16-wide item
__device__ __forceinline__ void rotate16(const float* a, const float* b, const float* cs, int c, float sc, float* ya,
                                         float* yb) {
  float co[16], si[16];
  ld16f(cs + c * 16, co);
  ld16f(cs + HALF + c * 16, si);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    ya[j] = (a[j] * co[j] - b[j] * si[j]) * sc;
    yb[j] = (b[j] * co[j] + a[j] * si[j]) * sc;
  }
}

}  // namespace kv8

using namespace kv8;

// ----------------------------------------------------------------------------------------------------- writers
// grid = tokens, block = 256; an item is 16 dims of one head (a 16-byte store per lane into the cache).
__global__ void __launch_bounds__(256) rope_cache_kv8_kernel(bf16_t* __restrict__ qkv, int64_t qkv_stride,
                                                             const int64_t* __restrict__ positions,
                                                             const float* __restrict__ cos_sin,
                                                             const int64_t* __restrict__ slot_mapping,
                                                             uint8_t* __restrict__ k_cache,
                                                             uint8_t* __restrict__ v_cache, int hq, int hkv,
                                                             int block_size, float k_scale, float v_scale, int rot_q,
                                                             const float* __restrict__ row_scale) {
  const int64_t tok = blockIdx.x;
  bf16_t* row = qkv + tok * qkv_stride;
  const int64_t pos = positions[tok];
  const int64_t slot = slot_mapping ? slot_mapping[tok] : -1;
  const float* cs = cos_sin + pos * D;
  const float rsc = row_scale != nullptr ? row_scale[tok] : 1.f;
  const int h0 = rot_q ? 0 : hq;
  const int n_rot = (hq + hkv - h0) * RC;
  const int n_items = n_rot + hkv * VC;
  const int64_t blk = slot / block_size, off = slot % block_size;
  for (int it = threadIdx.x; it < n_items; it += blockDim.x) {
    if (it < n_rot) {
      const int head = h0 + it / RC, c = it % RC;
      if (head >= hq && slot < 0) continue;
      bf16_t* x = row + head * D + c * 16;
      float a[16], b[16], ya[16], yb[16];
      ld16bf(x, a);
      ld16bf(x + HALF, b);
      rotate16(a, b, cs, c, head < hq ? 1.f : rsc, ya, yb);
      if (head < hq) {
        st16bf(x, ya);
        st16bf(x + HALF, yb);
      } else {
        uint8_t* dst = k_cache + ((blk * hkv + (head - hq)) * block_size + off) * D + c * 16;
        *reinterpret_cast<uint4*>(dst) = quant16(ya, k_scale);
        *reinterpret_cast<uint4*>(dst + HALF) = quant16(yb, k_scale);
      }
    } else if (slot >= 0) {
      const int v = it - n_rot;
      const int kh = v / VC, c = v % VC;
      float f[16];
      ld16bf(row + (hq + hkv + kh) * D + c * 16, f);
#pragma unroll
      for (int j = 0; j < 16; ++j) f[j] *= rsc;
      *reinterpret_cast<uint4*>(v_cache + ((blk * hkv + kh) * block_size + off) * D + c * 16) = quant16(f, v_scale);
    }
  }
}

__global__ void __launch_bounds__(256) rope_cache_slab_kv8_kernel(bf16_t* __restrict__ q_out,
                                                                  const float* __restrict__ slab, int sk,
                                                                  const int64_t* __restrict__ positions,
                                                                  const float* __restrict__ cos_sin,
                                                                  const int64_t* __restrict__ slot_mapping,
                                                                  uint8_t* __restrict__ k_cache,
                                                                  uint8_t* __restrict__ v_cache, int T, int hq, int hkv,
                                                                  int block_size, float k_scale, float v_scale) {
  const int64_t tok = blockIdx.x;
  const int width = (hq + 2 * hkv) * D;
  const int64_t sstride = (int64_t)T * width;
  const float* row = slab + tok * width;
  const int64_t pos = positions[tok];
  const int64_t slot = slot_mapping ? slot_mapping[tok] : -1;
  const float* cs = cos_sin + pos * D;
  const int n_rot = (hq + hkv) * RC;
  const int n_items = n_rot + hkv * VC;
  const int64_t blk = slot / block_size, off = slot % block_size;
  auto sum16 = [&](int o, float* v) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = 0.f;
    for (int s = 0; s < sk; ++s) {
      float t[16];
      ld16f(row + s * sstride + o, t);
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] += t[j];
    }
  };
  for (int it = threadIdx.x; it < n_items; it += blockDim.x) {
    if (it < n_rot) {
      const int head = it / RC, c = it % RC;
      if (head >= hq && slot < 0) continue;
      float a[16], b[16], ya[16], yb[16];
      sum16(head * D + c * 16, a);
      sum16(head * D + c * 16 + HALF, b);
      rotate16(a, b, cs, c, 1.f, ya, yb);
      if (head < hq) {
        bf16_t* x = q_out + tok * hq * D + head * D + c * 16;
        st16bf(x, ya);
        st16bf(x + HALF, yb);
      } else {
        uint8_t* dst = k_cache + ((blk * hkv + (head - hq)) * block_size + off) * D + c * 16;
        *reinterpret_cast<uint4*>(dst) = quant16(ya, k_scale);
        *reinterpret_cast<uint4*>(dst + HALF) = quant16(yb, k_scale);
      }
    } else if (slot >= 0) {
      const int v = it - n_rot;
      const int kh = v / VC, c = v % VC;
      float f[16];
      sum16((hq + hkv + kh) * D + c * 16, f);
      *reinterpret_cast<uint4*>(v_cache + ((blk * hkv + kh) * block_size + off) * D + c * 16) = quant16(f, v_scale);
    }
  }
}

hipError_t launch_rope_and_cache_kv8(bf16_t* qkv, int64_t qkv_stride, const int64_t* positions, const float* cos_sin,
                                     const int64_t* slot_mapping, uint8_t* k_cache, uint8_t* v_cache, int num_tokens,
                                     int hq, int hkv, int head_dim, int block_size, float k_scale, float v_scale,
                                     bool rot_q, const float* row_scale, hipStream_t s) {
  if (num_tokens == 0) return hipSuccess;
  if (head_dim != D || block_size < 1 || !(k_scale > 0.f) || !(v_scale > 0.f)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rope_cache_kv8_kernel, dim3(num_tokens), dim3(256), 0, s, qkv, qkv_stride, positions, cos_sin,
                     slot_mapping, k_cache, v_cache, hq, hkv, block_size, k_scale, v_scale, (int)rot_q, row_scale);
  return hipGetLastError();
}

hipError_t launch_rope_and_cache_slab_kv8(bf16_t* q_out, const float* slab, int sk, const int64_t* positions,
                                          const float* cos_sin, const int64_t* slot_mapping, uint8_t* k_cache,
                                          uint8_t* v_cache, int num_tokens, int hq, int hkv, int head_dim,
                                          int block_size, float k_scale, float v_scale, hipStream_t s) {
  if (num_tokens == 0) return hipSuccess;
  if (head_dim != D || block_size < 1 || sk < 1 || !(k_scale > 0.f) || !(v_scale > 0.f)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rope_cache_slab_kv8_kernel, dim3(num_tokens), dim3(256), 0, s, q_out, slab, sk, positions,
                     cos_sin, slot_mapping, k_cache, v_cache, num_tokens, hq, hkv, block_size, k_scale, v_scale);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------ decode
constexpr int K8_ROW = 128;                       // bytes per e4m3 K / V row
constexpr int K8_IMG = DEC_KEYS * K8_ROW;         // one image of a 128-key chunk: 16 KiB
constexpr int K8_CHUNK = 2 * K8_IMG;              // K + V: 32 KiB
constexpr int K8_RING = 3;                        // buffers: the chunk being computed and two in flight
constexpr int K8_ML = 4 * 32 * 2 * 4;             // per-wave (m, l): 1 KiB
constexpr int K8_MERGE = K8_ML + 4 * 8 * D * 4;   // + per-wave O of G <= 8: 17 KiB
constexpr int K8_QOFF = K8_RING * K8_CHUNK + K8_MERGE;  // q image: G <= 8 rows x 256 B
constexpr int K8_LDS = K8_QOFF + 2048 + 16;
static_assert(K8_LDS <= 160 * 1024, "one workgroup per CU");
// FUSED: the prologue's staging, an area of its own behind the control words (v3's 27 KiB limit)
constexpr int K8_STAGE = 27 * 1024;
constexpr int K8_LDS_FUSED = K8_LDS + K8_STAGE;
static_assert(K8_LDS % 16 == 0 && K8_LDS_FUSED <= 160 * 1024, "one fused workgroup per CU");

// LDS traffic of the fused prologue, in inline asm as attn_common.h's merge-area helpers (and for their reason)
__device__ __forceinline__ void lds_ld128x2(uint32_t a, uint32_t b, f32x4_t& x, f32x4_t& y) {
  asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(x), "=&v"(y)
               : "v"(a), "v"(b)
               : "memory");
}
__device__ __forceinline__ void lds_st64(uint32_t a, uint32_t lo, uint32_t hi) {
  const u32x2_t v = {lo, hi};
  asm volatile("ds_write_b64 %0, %1" ::"v"(a), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_st32u(uint32_t a, uint32_t v) {
  asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(v) : "memory");
}

// S^T tile of this wave's 32 keys from the swizzled e4m3 K image; qf[2j + e] holds dims 32j + 16h + 8e + [0, 8).
// The reads are inline asm retired by one wait tied to their results (as pv_lds_swz_v3: the compiler cannot tell
// them from the LDS-DMA in flight into the other buffers and would drain it first).
__device__ __forceinline__ f32x16_t qk_kv8(const char* kimg, const bf16x8_t qf[8], int lane) {
  f32x16_t s;
#pragma unroll
  for (int r = 0; r < 16; ++r) s[r] = 0.f;
  const int row = lane & 31, h = lane >> 5, sw = (row >> 1) & 7;
  const uint32_t base = lds_addr(kimg) + row * K8_ROW;
  u32x4_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) asm volatile("ds_read_b128 %0, %1" : "=v"(w[j]) : "v"(base + 16 * ((2 * j + h) ^ sw)));
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(widen8(w[j][0], w[j][1]), qf[2 * j], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(widen8(w[j][2], w[j][3]), qf[2 * j + 1], s, 0, 0, 0);
  }
  return s;
}

// O^T += V^T P^T from the swizzled e4m3 V image of this wave's 32 keys.
__device__ __forceinline__ void pv_kv8(const char* vimg, const f32x16_t& p, State& st, int lane) {
  bf16x8_t pf[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    uint4 w;
    w.x = pack2(p[8 * s2 + 0], p[8 * s2 + 1]);
    w.y = pack2(p[8 * s2 + 2], p[8 * s2 + 3]);
    w.z = pack2(p[8 * s2 + 4], p[8 * s2 + 5]);
    w.w = pack2(p[8 * s2 + 6], p[8 * s2 + 7]);
    pf[s2] = as_frag(w);
  }
  const int g = lane >> 4, i = lane & 15, h = lane >> 5, j = i >> 1;
  const int key = 4 * h + (j & 3) + 8 * (j >> 2);  // of 16-key half s2 (+ 16 s2: the swizzle term is unchanged)
  const uint32_t rb = lds_addr(vimg) + key * K8_ROW + 8 * (i & 1);
  const int sw = (key >> 1) & 7;
  u32x2_t t[4][2];
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    const uint32_t a0 = rb + 16 * ((2 * db + (g & 1)) ^ sw);
    asm volatile("ds_read_b64_tr_b8 %0, %1" : "=v"(t[db][0]) : "v"(a0));
    asm volatile("ds_read_b64_tr_b8 %0, %1 offset:2048" : "=v"(t[db][1]) : "v"(a0));
  }
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(t[0][0]), "+v"(t[0][1]), "+v"(t[1][0]), "+v"(t[1][1]), "+v"(t[2][0]), "+v"(t[2][1]),
                 "+v"(t[3][0]), "+v"(t[3][1]));
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
      st.o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(widen8(t[db][s2][0], t[db][s2][1]), pf[s2], st.o[db], 0, 0, 0);
}

// grid = min(tasks, CUs); block = 256; dynamic LDS = K8_LDS (FUSED: K8_LDS_FUSED). scale_log2 carries k_scale.
// FUSED (the file header): q / q_stride are unused; fz, slot_mapping, k_scale and the caches' writable aliases
// kw / vw feed the prologue. Without it they are unused and the kernel is what it was.
template <int G, bool FUSED, int KV_AUX>
__global__ void __launch_bounds__(256, 1) attn_decode_kv8_kernel(
    const int* __restrict__ block_tables, const int* __restrict__ ctx_lens, int bt_stride, int num_seqs, int hkv,
    int maxp, int cpp, const uint8_t* __restrict__ k_cache, const uint8_t* __restrict__ v_cache, int hq,
    float scale_log2, float v_scale, const bf16_t* __restrict__ q, int64_t q_stride, bf16_t* __restrict__ out,
    float* __restrict__ part_o, float* __restrict__ part_ml, int* __restrict__ counters, AttnDecodeFuse fz,
    const int64_t* __restrict__ slot_mapping, float k_scale, uint8_t* kw, uint8_t* vw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ml = reinterpret_cast<float*>(smem + K8_RING * K8_CHUNK);
  float* ob = reinterpret_cast<float*>(smem + K8_RING * K8_CHUNK + K8_ML);
  int* ctl = reinterpret_cast<int*>(smem + K8_QOFF + 2048);
  constexpr int QI = (G * 256 + 1023) / 1024;  // LDS-DMA instructions for the query rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, row = lane & 31;
  const int pairs = num_seqs * hkv;
  const int C = cpp;  // chunks per part (host: launch_attn_decode_kv8)
  const int np = (maxp + C - 1) / C;
  const int n_tasks = pairs * np;
  // FUSED staging: slab rows x 128 fp32, [split][q heads] then [split][k, v]; behind them the statistics tiles
  // (1 KiB) and the RoPE row. A part without the step's new token stages only the q rows.
  char* fa = smem + K8_LDS;
  const int fsk = FUSED ? fz.sk : 0;
  const int frows = fsk * (G + 2), qrows = fsk * G;
  const int fs_off = ((frows + 1) / 2) * 1024;
  bool ran = false;  // FUSED: a task of this workgroup has used the ring and the merge area

#pragma unroll 1
  for (int t = blockIdx.x; t < n_tasks; t += gridDim.x) {
    const int pair = t % pairs, part = t / pairs;
    const int seq = pair / hkv, kvh = pair - seq * hkv;
    const int c0 = part * C;
    const int* bt = block_tables + (int64_t)seq * bt_stride;
    const int ctx = __builtin_amdgcn_readfirstlane(ctx_lens[seq]);
    const int nch = (ctx + DEC_KEYS - 1) / DEC_KEYS;
    if (c0 >= nch) continue;  // uniform
    const int c1 = min(c0 + C, nch);
    const int last_blk = (ctx - 1) >> 4;
    const bool has_new = FUSED && c1 == nch;  // this part holds the step's new token (key ctx - 1)

    if constexpr (FUSED) {
      // the prologue's operands, ahead of the first chunk in the same queue
      const float* srow = fz.slab + (int64_t)seq * fz.width;
      const int nrows = has_new ? frows : qrows;
      for (int i = wave; i < (nrows + 1) / 2; i += 4) {  // two rows per instruction (an odd count: the last twice)
        const int ri = min(2 * i + (lane >> 5), nrows - 1);
        int sl, j;
        if (ri < qrows) {
          sl = ri / G;
          j = ri - sl * G;
        } else {
          sl = (ri - qrows) >> 1;
          j = G + ((ri - qrows) & 1);
        }
        const int col = j < G ? (kvh * G + j) * D : (j == G ? (hq + kvh) * D : (hq + hkv + kvh) * D);
        glds16(srow + sl * fz.slab_stride + col + (lane & 31) * 4, fa + i * 1024);
      }
      if (wave == 0) {  // the statistics tiles (<= 256: 4 x 64 lanes; the upper two only when present)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < 2 || 64 * i < fz.ssp_tiles)
            glds4(fz.ssp + min(lane + 64 * i, fz.ssp_tiles - 1) * DECODE_SSP_LD + seq, fa + fs_off + i * 256);
      }
      if (wave == 1)  // decode: the new token sits at position ctx - 1
        glds16(fz.cos_sin + (int64_t)(ctx - 1) * D + (lane & 31) * 4, fa + fs_off + 1024);
      // the staging is nobody else's, so only now the hand-over of the ring and the merge area by the previous task
      if (ran) lds_barrier();
      ran = true;
    } else if (wave == 0) {
      // the G query rows (256 B each) go to the q image by LDS-DMA, ahead of the first chunk in the same queue, so
      // no ordinary load sits in front of the counted chunk waits
      const bf16_t* qb = q + (int64_t)seq * q_stride + (int64_t)kvh * G * D;
#pragma unroll
      for (int i = 0; i < QI; ++i) {
        const int qr = min(4 * i + (lane >> 4), G - 1);
        glds16(qb + qr * D + (lane & 15) * 8, smem + K8_QOFF + i * 1024);
      }
    }

    // LDS-DMA this wave's 32 K rows and 32 V rows of chunk c into buffer b: 8 instructions per lane. The table row
    // is read speculatively (clamped to the row, not to the context); keys past the context re-read key ctx - 1.
    auto issue = [&](int c, int b) {
      char* base = smem + b * K8_CHUNK;
      const int j0 = c * 8 + 2 * wave;
      const int e0 = bt[__builtin_amdgcn_readfirstlane(min(j0, bt_stride - 1))];
      const int e1 = bt[__builtin_amdgcn_readfirstlane(min(j0 + 1, bt_stride - 1))];
      const int el = j0 + 1 > last_blk ? bt[last_blk] : 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 8 * i + (lane >> 3);  // row of the wave's 32: one instruction fills 8 rows
        const int j = j0 + (i >> 1);
        const int64_t blk = j <= last_blk ? (i < 2 ? e0 : e1) : el;
        const int key = min(c * DEC_KEYS + 32 * wave + r, ctx - 1);
        const int64_t roff = ((blk * hkv + kvh) * 16 + (key & 15)) * K8_ROW + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
        glds16<KV_AUX>(k_cache + roff, base + (wave * 4 + i) * 1024);
        glds16<KV_AUX>(v_cache + roff, base + K8_IMG + (wave * 4 + i) * 1024);
      }
    };

    State st;
    init_state(st);
    bf16x8_t qf[8];
    issue(c0, 0);
    if (c0 + 1 < c1) issue(c0 + 1, 1);
    uint32_t nk0 = 0, nk1 = 0;  // FUSED: this lane's two dwords of the new token's e4m3 K or V row
    if constexpr (FUSED) {
      // the prologue's operands have landed; the chunks issued behind them stay in flight
      if (c0 + 1 < c1)
        wait_vm<16>();
      else
        wait_vm<8>();
      __builtin_amdgcn_s_barrier();
      const uint32_t fb = lds_addr(fa), cs = fb + fs_off + 1024;
      // rn = rsqrt(mean(h^2) + eps) of this sequence's row (v3's order of the sum)
      float ssum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        ssum += lane + 64 * i < fz.ssp_tiles ? lds_ld32(fb + fs_off + 4 * (lane + 64 * i)) : 0.f;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ssum += __shfl_xor(ssum, o, 64);
      const float rn = rsqrtf(ssum * fz.inv_n + fz.eps);
      // 4 dims d .. d + 3 and their rotation partners of staged row j (q head j < G, G: k, G + 1: v) of every
      // split, summed in index order from +0 and scaled
      auto sum4x2 = [&](int j, int d, float* a, float* bq) {
        f32x4_t va = {0.f, 0.f, 0.f, 0.f}, vb = va;
        for (int sl = 0; sl < fsk; ++sl) {
          const uint32_t r = fb + (((j < G ? sl * G : qrows + 2 * sl - G) + j) * D + d) * 4;
          f32x4_t x, y;
          lds_ld128x2(r, r + 4 * HALF, x, y);
          va += x;
          vb += y;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = va[e] * rn;
          bq[e] = vb[e] * rn;
        }
      };
      auto rot4 = [&](int j, int d, float* ya, float* yb) {
        float a[4], bq[4];
        sum4x2(j, d, a, bq);
        f32x4_t co, si;
        lds_ld128x2(cs + 4 * d, cs + 4 * (d + HALF), co, si);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ya[e] = a[e] * co[e] - bq[e] * si[e];
          yb[e] = bq[e] * co[e] + a[e] * si[e];
        }
      };
      if (tid < 16 * G) {  // the rotated query rows, rounded to bf16 once -> q image
        const int j = tid >> 4, d = 4 * (tid & 15);
        float ya[4], yb[4];
        rot4(j, d, ya, yb);
        const uint32_t qa = lds_addr(smem + K8_QOFF + j * 256);
        lds_st64(qa + 2 * d, pack2(ya[0], ya[1]), pack2(ya[2], ya[3]));
        lds_st64(qa + 2 * (d + HALF), pack2(yb[0], yb[1]), pack2(yb[2], yb[3]));
      } else if (has_new && tid >= 192 && tid < 208) {  // the new key: e4m3 from the fp32 values
        float ya[4], yb[4];
        rot4(G, 4 * (tid - 192), ya, yb);
        nk0 = quant4(ya, k_scale);
        nk1 = quant4(yb, k_scale);
      } else if (has_new && tid >= 208 && tid < 224) {  // the new value: the same two groups of 4 dims, unrotated
        float f0[4], f1[4];
        sum4x2(G + 1, 4 * (tid - 208), f0, f1);
        nk0 = quant4(f0, v_scale);
        nk1 = quant4(f1, v_scale);
      }
      // the q image is read after the first chunk's barrier below: retire this wave's LDS writes first
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    int b = 0;
#pragma unroll 1
    for (int c = c0; c < c1; ++c) {
      // the buffer two ahead held chunk c - 1: this wave's own rows, whose reads it retired last iteration
      if (c + 2 < c1) {
        issue(c + 2, b >= 1 ? b - 1 : 2);
        wait_vm<16>();
      } else if (c + 1 < c1) {
        wait_vm<8>();
      } else {
        wait_vm<0>();
      }
      // a wave needs another wave's data at the first chunk (the q image: wave 0's DMA, or FUSED every thread's
      // stores) and, FUSED, at the chunk that gets the new token's row patched in (the row may be another wave's DMA)
      if (c == c0 || (FUSED && has_new && c + 1 == c1)) __builtin_amdgcn_s_barrier();
      if constexpr (FUSED) {
        if (has_new && c + 1 == c1) {
          // the part's last chunk: vmcnt(0) above, so the cache stores sit in front of no counted wait. Each dword
          // goes to the paged cache (for later steps; slot < 0: a padded graph row, not stored) and to the same
          // row of this step's LDS image, at its swizzled place
          const int rr = (ctx - 1) - c * DEC_KEYS, sw = (rr >> 1) & 7;
          const int64_t slot = slot_mapping[seq];
          const int64_t roff = (((slot >> 4) * hkv + kvh) * 16 + (slot & 15)) * K8_ROW;
          if (tid >= 192 && tid < 224) {
            const bool isv = tid >= 208;
            const int d = 4 * (tid - (isv ? 208 : 192));
            const uint32_t img = lds_addr(smem + b * K8_CHUNK) + (isv ? K8_IMG : 0) + rr * K8_ROW + (d & 15);
            lds_st32u(img + 16 * ((d >> 4) ^ sw), nk0);
            lds_st32u(img + 16 * (((d + HALF) >> 4) ^ sw), nk1);
            if (slot >= 0) {
              uint8_t* dst = (isv ? vw : kw) + roff + d;
              *reinterpret_cast<uint32_t*>(dst) = nk0;
              *reinterpret_cast<uint32_t*>(dst + HALF) = nk1;
            }
          }
          lds_barrier();
        }
      }
      if (c == c0) {
        // the fragments follow qk_kv8's contraction order: step 2j + e is 16-byte chunk 4j + 2h + e of the row
#pragma unroll
        for (int j = 0; j < 8; ++j)
          qf[j] = row < G ? __builtin_bit_cast(bf16x8_t, lds_ld128(lds_addr(smem + K8_QOFF + row * 256 +
                                                                              (4 * (j >> 1) + 2 * h + (j & 1)) * 16)))
                          : zero_frag();
      }
      const char* kimg = smem + b * K8_CHUNK + 32 * wave * K8_ROW;
      f32x16_t s = qk_kv8(kimg, qf, lane);
      softmax_tile_lazy(s, st, c * DEC_KEYS + 32 * wave, ctx, scale_log2, h);  // keys >= ctx: masked
      pv_kv8(kimg + K8_IMG, s, st, lane);
      b = b == K8_RING - 1 ? 0 : b + 1;
    }

    // merge the 4 waves' (m, l, O) through LDS (attn_decode_v3's epilogue; v_scale joins the normalisation)
    if (row < G) {
      if (h == 0) {
        lds_st32(lds_addr(ml + (wave * 32 + row) * 2 + 0), st.m);
        lds_st32(lds_addr(ml + (wave * 32 + row) * 2 + 1), st.l);
      }
      const uint32_t o = lds_addr(ob + (wave * G + row) * D);
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
          lds_st128(o + 4 * (32 * db + 8 * g4 + 4 * h),
                    f32x4_t{st.o[db][4 * g4], st.o[db][4 * g4 + 1], st.o[db][4 * g4 + 2], st.o[db][4 * g4 + 3]});
    }
    lds_barrier();
    const int nparts = (nch + C - 1) / C;  // parts of THIS pair
    for (int e = tid; e < G * (D / 4); e += 256) {
      const int r = e / (D / 4), d = 4 * (e % (D / 4));
      float mw[4], lw[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        mw[w] = lds_ld32(lds_addr(ml + (w * 32 + r) * 2));
        lw[w] = lds_ld32(lds_addr(ml + (w * 32 + r) * 2 + 1));
      }
      float M = NEG_BIG;
#pragma unroll
      for (int w = 0; w < 4; ++w) M = fmaxf(M, mw[w]);
      float L = 0.f;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float f = exp2f(mw[w] - M);
        L += f * lw[w];
        const f32x4_t v = lds_ld128(lds_addr(ob + (w * G + r) * D + d));
        acc.x += f * v.x;
        acc.y += f * v.y;
        acc.z += f * v.z;
        acc.w += f * v.w;
      }
      const int head = kvh * G + r;
      if (nparts == 1) {
        const float inv = L > 0.f ? v_scale / L : 0.f;
        uint2 pk;
        pk.x = pack2(acc.x * inv, acc.y * inv);
        pk.y = pack2(acc.z * inv, acc.w * inv);
        *reinterpret_cast<uint2*>(out + ((int64_t)seq * hq + head) * D + d) = pk;
      } else {
        const int64_t slot = ((int64_t)seq * hq + head) * maxp + part;
        __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(part_o, 0, 0x7fffffff, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, acc),
                                               ro, (int)(slot * D + d) * 4, 0, 16);
        if (d == 0) {
          __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(part_ml, 0, 0x7fffffff, 0x00020000);
          const float2 mlv = make_float2(M, L);
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, mlv),
                                                rm, (int)(slot * 2) * 4, 0, 16);
        }
      }
    }
    if (nparts > 1) {
      wait_vm<0>();  // this wave's write-through partial stores are done
      lds_barrier();
      if (tid == 0) {
        const int old = __hip_atomic_fetch_add(counters + pair, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ctl[1] = old == nparts - 1;
      }
      lds_barrier();
      if (ctl[1]) {  // last arriver: merge every part of this pair
        __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(part_o, 0, 0x7fffffff, 0x00020000);
        __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(part_ml, 0, 0x7fffffff, 0x00020000);
        for (int e = tid; e < G * (D / 4); e += 256) {
          const int r = e / (D / 4), d = 4 * (e % (D / 4));
          const int head = kvh * G + r;
          const int64_t s0 = ((int64_t)seq * hq + head) * maxp;
          float M = NEG_BIG, L = 0.f;
          float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
          constexpr int PB = 8;  // parts per round of loads (indices clamped, the surplus masked)
          for (int p0 = 0; p0 < nparts; p0 += PB) {
            float2 mv[PB];
            float4 ov[PB];
#pragma unroll
            for (int j = 0; j < PB; ++j) {
              const int p = min(p0 + j, nparts - 1);
              mv[j] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rm, (int)((s0 + p) * 2) * 4, 0, 16));
              ov[j] = __builtin_bit_cast(float4,
                                         __builtin_amdgcn_raw_buffer_load_b128(ro, (int)((s0 + p) * D + d) * 4, 0, 16));
            }
#pragma unroll
            for (int j = 0; j < PB; ++j) {
              const bool ok = p0 + j < nparts;
              const float mx = ok ? mv[j].x : NEG_BIG;
              const float Mn = fmaxf(M, mx);
              const float a = exp2f(M - Mn), bb = ok ? exp2f(mx - Mn) : 0.f;
              L = L * a + mv[j].y * bb;
              acc.x = acc.x * a + ov[j].x * bb;
              acc.y = acc.y * a + ov[j].y * bb;
              acc.z = acc.z * a + ov[j].z * bb;
              acc.w = acc.w * a + ov[j].w * bb;
              M = Mn;
            }
          }
          const float inv = L > 0.f ? v_scale / L : 0.f;
          uint2 pk;
          pk.x = pack2(acc.x * inv, acc.y * inv);
          pk.y = pack2(acc.z * inv, acc.w * inv);
          *reinterpret_cast<uint2*>(out + ((int64_t)seq * hq + head) * D + d) = pk;
        }
        if (tid == 0) __hip_atomic_store(counters + pair, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // merge area and ring are reused by the next task (FUSED: the barrier follows that task's staging DMA, above)
    if constexpr (!FUSED) lds_barrier();
  }
}

// chunks per part from the static bound: pairs x parts ~ the grid, as launch_attn_decode's v3 split
static int kv8_chunks_per_part(int pairs, int maxp, int* grid_out) {
  const int tasks = pairs * maxp, ncu = num_cus();
  const int grid = tasks < ncu ? tasks : ncu;
  if (grid_out) *grid_out = grid;
  return std::max(1, std::min(maxp, (maxp * pairs + grid - 1) / grid));
}

int attn_decode_kv8_part_keys(int num_seqs, int hkv, int max_ctx) {
  const int maxp = (max_ctx + DEC_KEYS - 1) / DEC_KEYS;
  if (num_seqs < 1 || hkv < 1 || maxp < 1) return DEC_KEYS;
  return DEC_KEYS * kv8_chunks_per_part(num_seqs * hkv, maxp, nullptr);
}

// both decode launchers; fz != nullptr: the fused prologue, kw / vw the caches' writable aliases
static hipError_t decode_kv8(bf16_t* out, float* part_o, float* part_ml, int* counters, const bf16_t* q,
                             int64_t q_stride, const uint8_t* k_cache, const uint8_t* v_cache, uint8_t* kw, uint8_t* vw,
                             const int* block_tables, int bt_stride, const int* ctx_lens, int num_seqs, int max_ctx,
                             int hq, int hkv, int head_dim, int block_size, float scale, float k_scale, float v_scale,
                             const AttnDecodeFuse* fz, bool kv_once, hipStream_t s) {
  if (num_seqs == 0) return hipSuccess;
  if (head_dim != D || hkv < 1 || hq % hkv || block_size != 16 || counters == nullptr || max_ctx < 1 || bt_stride < 1)
    return hipErrorInvalidValue;
  const int G = hq / hkv;
  const int maxp = (max_ctx + DEC_KEYS - 1) / DEC_KEYS;
  if ((int64_t)num_seqs * hq * maxp * D * 4 >= ((int64_t)1 << 31)) return hipErrorInvalidValue;  // 32-bit buffer offsets
  AttnDecodeFuse fzc{};
  if (fz != nullptr) {
    if (!(k_scale > 0.f) || !(v_scale > 0.f) || fz->slab == nullptr || fz->ssp == nullptr || fz->cos_sin == nullptr ||
        fz->slot_mapping == nullptr || fz->sk < 1 || fz->ssp_tiles < 1 || fz->ssp_tiles > DECODE_SSP_MAX_TILES ||
        num_seqs > DECODE_SSP_LD || fz->width != (hq + 2 * hkv) * D ||
        ((fz->sk * (G + 2) + 1) / 2) * 1024 + 2048 > K8_STAGE)
      return hipErrorInvalidValue;
    fzc = *fz;
    fzc.ts = nullptr;
  }
  const int64_t* slots = fzc.slot_mapping;
  const float sl2 = scale * 1.4426950408889634f * k_scale;
  int gridx = 1;
  const int cpp = kv8_chunks_per_part(num_seqs * hkv, maxp, &gridx);
  dim3 grid(gridx), block(256);
#define K8_LAUNCH(GG, FU, AUX)                                                                                     \
  hipLaunchKernelGGL((attn_decode_kv8_kernel<GG, FU, AUX>), grid, block, FU ? K8_LDS_FUSED : K8_LDS, s, block_tables, \
                     ctx_lens, bt_stride, num_seqs, hkv, maxp, cpp, k_cache, v_cache, hq, sl2, v_scale, q, q_stride, \
                     out, part_o, part_ml, counters, fzc, slots, k_scale, kw, vw)
#define K8_CASE(GG)                              \
  case GG:                                       \
    if (fz && kv_once)                           \
      K8_LAUNCH(GG, true, KV_AUX_ONCE);          \
    else if (fz)                                 \
      K8_LAUNCH(GG, true, KV_AUX_DEFAULT);       \
    else if (kv_once)                            \
      K8_LAUNCH(GG, false, KV_AUX_ONCE);         \
    else                                         \
      K8_LAUNCH(GG, false, KV_AUX_DEFAULT);      \
    break;
  switch (G) {
    K8_CASE(1)
    K8_CASE(2)
    K8_CASE(4)
    K8_CASE(8)
    default:
      return hipErrorInvalidValue;
  }
#undef K8_CASE
#undef K8_LAUNCH
  return hipGetLastError();
}

hipError_t launch_attn_decode_kv8(bf16_t* out, float* part_o, float* part_ml, int* counters, const bf16_t* q,
                                  int64_t q_stride, const uint8_t* k_cache, const uint8_t* v_cache,
                                  const int* block_tables, int bt_stride, const int* ctx_lens, int num_seqs, int max_ctx,
                                  int hq, int hkv, int head_dim, int block_size, float scale, float k_scale,
                                  float v_scale, bool kv_once, hipStream_t s) {
  return decode_kv8(out, part_o, part_ml, counters, q, q_stride, k_cache, v_cache, nullptr, nullptr, block_tables,
                    bt_stride, ctx_lens, num_seqs, max_ctx, hq, hkv, head_dim, block_size, scale, k_scale, v_scale,
                    nullptr, kv_once, s);
}

hipError_t launch_attn_decode_fused_kv8(bf16_t* out, float* part_o, float* part_ml, int* counters, uint8_t* k_cache,
                                        uint8_t* v_cache, const int* block_tables, int bt_stride, const int* ctx_lens,
                                        int num_seqs, int max_ctx, int hq, int hkv, int head_dim, int block_size,
                                        float scale, float k_scale, float v_scale, const AttnDecodeFuse* fz,
                                        bool kv_once, hipStream_t s) {
  if (fz == nullptr) return hipErrorInvalidValue;
  return decode_kv8(out, part_o, part_ml, counters, nullptr, 0, k_cache, v_cache, k_cache, v_cache, block_tables,
                    bt_stride, ctx_lens, num_seqs, max_ctx, hq, hkv, head_dim, block_size, scale, k_scale, v_scale, fz,
                    kv_once, s);
}

// ----------------------------------------------------------------------------------------------------- prefill
// attn_prefill_kernel (attention.hip) with the e4m3 staging role; everything after the LDS image is that kernel's.
template <int G, int NS, int NW>
__global__ void __launch_bounds__(64 * NW, 8 / NW) attn_prefill_kv8_kernel(
    bf16_t* __restrict__ out, const bf16_t* __restrict__ q, int64_t q_stride, const uint8_t* __restrict__ k_cache,
    const uint8_t* __restrict__ v_cache, const int* __restrict__ block_tables, int bt_stride,
    const int* __restrict__ cu_q, const int* __restrict__ ctx_lens, int hq, int hkv, int block_size, float scale_log2,
    float v_scale, const float* __restrict__ cos_sin, int n_pos, const float* __restrict__ q_scale) {
  constexpr int TPW = 32 / G;   // tokens per wave
  constexpr int TPB = NW * TPW;  // tokens per workgroup
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // XCD-aware order (attn_prefill_kernel): a (sequence, kv head) group's q tiles share one L2
  const int gx = gridDim.x, gy = gridDim.y;
  const int hw = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
  const int nwg = gx * gy * gridDim.z, xq = nwg >> 3, xr = nwg & 7, xcd = hw & 7;
  const int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (hw >> 3);
  const int bx = lid % gx, seq = (lid / gx) % gy, kvh = lid / (gx * gy);
  const int qbeg = cu_q[seq], qlen = cu_q[seq + 1] - qbeg;
  const int t0 = (gx - 1 - bx) * TPB;  // heaviest (latest) tiles of a group launch first
  if (t0 >= qlen) return;
  const int ctx = ctx_lens[seq];
  const int pos0 = ctx - qlen;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  const int row = lane & 31;
  const int tok = t0 + wave * TPW + row / G;
  const int head = kvh * G + row % G;
  const bool row_valid = tok < qlen;
  const int kv_len_row = min(ctx, pos0 + min(tok, qlen - 1) + 1);
  const int kv_end = min(ctx, pos0 + min(t0 + TPB, qlen));
  constexpr int ST = NS * KT;  // keys per stage
  const int ntiles = (kv_end + ST - 1) / ST;
  const int wave_last_tok = min(t0 + wave * TPW + TPW, qlen) - 1;
  const int wave_kv_end = pos0 + wave_last_tok + 1;
  const int wave_kv_min = min(ctx, pos0 + min(t0 + wave * TPW, qlen - 1) + 1);
  const int* bt = block_tables + (int64_t)seq * bt_stride;

  bf16x8_t qf[8];
  load_q(qf, row_valid ? q + (int64_t)(qbeg + tok) * q_stride + (int64_t)head * D : nullptr, h);
  if (cos_sin != nullptr && row_valid) {  // RoPE and the RMSNorm row scale on the Q row as it is loaded
    const float* cs = cos_sin + (int64_t)min(pos0 + tok, n_pos - 1) * D;
    const float qs = q_scale != nullptr ? q_scale[qbeg + tok] : 1.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      float a[8], b[8], ya[8], yb[8];
      unpack8(__builtin_bit_cast(uint4, qf[kk]), a);
      unpack8(__builtin_bit_cast(uint4, qf[kk + 4]), b);
      const int i0 = 16 * kk + 8 * h;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float co = cs[i0 + j] * qs, si = cs[D / 2 + i0 + j] * qs;
        ya[j] = a[j] * co - b[j] * si;
        yb[j] = b[j] * co + a[j] * si;
      }
      qf[kk] = as_frag(pack8(ya));
      qf[kk + 4] = as_frag(pack8(yb));
    }
  }
  State st;
  init_state(st);

  // staging role: key kr + RPP i of the stage, 16-byte chunk c of its 128-byte row (8 lanes per row). The two
  // register sets hold BYTES (one u32x4 per K and V row chunk); store_one widens a chunk to 32 B of the bf16 image.
  constexpr int RPP = 8 * NW, NP = ST / RPP;
  static_assert(ST % RPP == 0, "whole passes per stage");
  const int kr = tid >> 3, c = tid & 7;
  u32x4_t kA[NP], vA[NP], kB[NP], vB[NP];
  auto load_one = [&](int kt, auto I, u32x4_t* kreg, u32x4_t* vreg) __attribute__((always_inline)) {
    constexpr int i = decltype(I)::value;
    const int key = kt * ST + kr + RPP * i;
    // a wave stages 8 consecutive keys (8-aligned, block_size a multiple of 16): one block, a scalar load. Keys past
    // kv_end re-read row kv_end - 1 (finite values the causal mask zeroes; no branch)
    const int kb = __builtin_amdgcn_readfirstlane(min(kt * ST + RPP * i + (kr & ~7), kv_end - 1) / block_size);
    const int64_t blk = bt[kb];
    const int64_t roff = ((blk * hkv + kvh) * block_size + min(key, kv_end - 1) % block_size) * D + c * 16;
    kreg[i] = *reinterpret_cast<const u32x4_t*>(k_cache + roff);
    vreg[i] = *reinterpret_cast<const u32x4_t*>(v_cache + roff);
  };
  auto widen_store = [](char* dst, u32x4_t w) __attribute__((always_inline)) {
    const uint2 a = widen4(w[0]), b = widen4(w[1]), cc = widen4(w[2]), d = widen4(w[3]);
    *reinterpret_cast<u32x4_t*>(dst) = u32x4_t{a.x, a.y, b.x, b.y};
    *reinterpret_cast<u32x4_t*>(dst + 16) = u32x4_t{cc.x, cc.y, d.x, d.y};
  };
  auto store_one = [&](int buf, auto I, const u32x4_t* kreg, const u32x4_t* vreg) __attribute__((always_inline)) {
    constexpr int i = decltype(I)::value;
    const int ks = kr + RPP * i;                        // key in the stage
    char* kl = smem + (buf * NS + ks / KT) * KV_TILE;  // its 32-key sub-tile
    char* vl = kl + K_TILE;
    widen_store(kl + (ks % KT) * K_PITCH + c * 32, kreg[i]);
    widen_store(vl + (ks % KT) * V_PITCH + c * 32, vreg[i]);
  };
#define LOAD_STAGE(kt, K, V) static_for<NP>([&](auto I) { load_one(kt, I, K, V); })
#define STORE_STAGE(buf, K, V) static_for<NP>([&](auto I) { store_one(buf, I, K, V); })
  auto compute = [&](int kt, int cur) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int kb0 = kt * ST + j * KT;
      if (kb0 < wave_kv_end) {  // wave-uniform: sub-tile not entirely in this wave's causal future
        const char* kl = smem + (cur * NS + j) * KV_TILE;
        f32x16_t s = qk_lds(kl, qf, lane);
        if (kb0 + KT <= wave_kv_min)
          softmax_tile_prefill<false>(s, st, kb0, kv_len_row, scale_log2, h);
        else
          softmax_tile_prefill<true>(s, st, kb0, kv_len_row, scale_log2, h);
        pv_lds(kl + K_TILE, s, st, lane);
      }
    }
  };

  LOAD_STAGE(0, kA, vA);
  LOAD_STAGE(min(1, ntiles - 1), kB, vB);
  STORE_STAGE(0, kA, vA);
  __syncthreads();
  auto stage_barrier = [] {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };
#pragma unroll 1
  for (int kt = 0; kt < ntiles; kt += 2) {
    LOAD_STAGE(min(kt + 2, ntiles - 1), kA, vA);
    compute(kt, 0);
    if (kt + 1 < ntiles) STORE_STAGE(1, kB, vB);
    stage_barrier();
    if (kt + 1 >= ntiles) break;
    LOAD_STAGE(min(kt + 3, ntiles - 1), kB, vB);
    compute(kt + 1, 1);
    if (kt + 2 < ntiles) STORE_STAGE(0, kA, vA);
    stage_barrier();
  }
#undef LOAD_STAGE
#undef STORE_STAGE

  // Epilogue: O staged through LDS and stored as whole rows (attn_prefill_kernel); v_scale joins the 1 / l
  {
    constexpr int OP = 272;
    char* ob = smem + wave * 32 * OP;
    const float inv = v_scale / st.l;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = 32 * db + 8 * g4 + 4 * h;
        uint2 v;
        v.x = pack2(st.o[db][4 * g4 + 0] * inv, st.o[db][4 * g4 + 1] * inv);
        v.y = pack2(st.o[db][4 * g4 + 2] * inv, st.o[db][4 * g4 + 3] * inv);
        *reinterpret_cast<uint2*>(ob + row * OP + d * 2) = v;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const int c16 = lane & 15;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = 4 * i + (lane >> 4);
      const int rtok = t0 + wave * TPW + r / G;
      const uint4 v = *reinterpret_cast<const uint4*>(ob + r * OP + c16 * 16);
      if (rtok < qlen)
        *reinterpret_cast<uint4*>(out + (int64_t)(qbeg + rtok) * hq * D + (int64_t)(kvh * G + r % G) * D + c16 * 8) = v;
    }
  }
}

hipError_t launch_attn_prefill_kv8(bf16_t* out, const bf16_t* q, int64_t q_stride, const uint8_t* k_cache,
                                   const uint8_t* v_cache, const int* block_tables, int bt_stride, const int* cu_q,
                                   const int* ctx_lens, int num_seqs, int max_q_len, int hq, int hkv, int head_dim,
                                   int block_size, float scale, float k_scale, float v_scale, const float* cos_sin,
                                   int n_pos, const float* q_scale, hipStream_t s) {
  if (num_seqs == 0 || max_q_len == 0) return hipSuccess;
  if (cos_sin != nullptr && n_pos < 1) return hipErrorInvalidValue;
  if (q_scale != nullptr && cos_sin == nullptr) return hipErrorInvalidValue;
  if (head_dim != D || hkv < 1 || hq % hkv || block_size < 16 || block_size % 16) return hipErrorInvalidValue;
  const int G = hq / hkv;
  const float sl2 = scale * 1.4426950408889634f * k_scale;
  // the bf16 launcher's two shapes: 8 waves x 64-key stages above 256 query tokens, 4 waves x 32-key stages below
  const bool short_q = max_q_len <= 256;
  const int NWr = short_q ? 4 : 8, NSr = short_q ? 1 : 2;
  const int tpb = NWr * (32 / (G > 32 ? 32 : G));
  dim3 grid((max_q_len + tpb - 1) / tpb, num_seqs, hkv), block(64 * NWr);
  const size_t lds = std::max<size_t>(2 * NSr * KV_TILE, (size_t)NWr * 32 * 272);  // ring / O staging
#define PF8_CASE2(GG, NS_, NW_)                                                                                    \
  if (G == GG && NSr == NS_ && NWr == NW_) {                                                                      \
    hipLaunchKernelGGL((attn_prefill_kv8_kernel<GG, NS_, NW_>), grid, block, lds, s, out, q, q_stride, k_cache,    \
                       v_cache, block_tables, bt_stride, cu_q, ctx_lens, hq, hkv, block_size, sl2, v_scale, cos_sin, \
                       n_pos, q_scale);                                                                            \
    return hipGetLastError();                                                                                      \
  }
#define PF8_CASE(GG) PF8_CASE2(GG, 2, 8) PF8_CASE2(GG, 1, 4)
  PF8_CASE(1)
  PF8_CASE(2)
  PF8_CASE(4)
  PF8_CASE(8)
  PF8_CASE(16)
  PF8_CASE(32)
  return hipErrorInvalidValue;
#undef PF8_CASE
#undef PF8_CASE2
}

}  // namespace die
