// What the guide kernels (token_guide, byte_guide, json_guide, schema_guide) share, and what logit_process.hip shares
// with them: the best-entry reduction and the rewrite of the LM-head candidates, the dense mask pass over a row, two
// pieces of the byte guides' token walks, and the launchers' argument checks. Everything here is inlined into its
// caller; docs/performance.md ("Shared guide passes") compares each kernel's registers, LDS and instruction count with
// what they were when each kernel carried its own copy. The token walks themselves (bg_, jg_, sg_walk_tokens) stay per
// kernel: one shared template was built and measured, and every form of it either slowed byte_guide's loop or cost
// schema_guide a wave per SIMD (same section).
#pragma once
#include "common.h"
#include "launchers.h"

namespace die {

constexpr int GUIDE_T = 1024;                    // threads per workgroup: one workgroup per batch row
constexpr int GUIDE_MAX_MAP_BYTES = 48 * 1024;   // the bitmap's share of LDS: vocab <= 393216 (as logit_process)
constexpr uint32_t GUIDE_NINF2 = 0xFF80FF80u;    // two bf16 -inf
constexpr int GUIDE_TU = 4;                      // tokens (independent chains) per lane in flight in a token walk

struct Best {
  float v;
  int i;
};
// Mirrors sampling.hip's better(), which stays the definition: larger value first, then lower index (sampling.hip is
// built with kernarg preload and keeps its own copy)
__device__ __forceinline__ Best better(Best a, Best b) {
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

// The workgroup's best of every thread's `best` becomes the row's LM-head candidate 0, the others (-inf, 0x7fffffff):
// the unchanged sampling tail then yields that entry. pc: the row's lm_parts (value bits, index) pairs. Every thread of
// the T-thread workgroup calls it.
template <int T>
__device__ __forceinline__ void write_best_candidate(Best best, uint32_t* pc, int lm_parts) {
  __shared__ Best red[T / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Best y;
    y.v = __shfl_xor(best.v, off, 64);
    y.i = __shfl_xor(best.i, off, 64);
    best = better(best, y);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = best;
  __syncthreads();
  Best wn = red[0];
  for (int q = 1; q < T / 64; ++q) wn = better(wn, red[q]);
  for (int q = threadIdx.x; q < lm_parts; q += T) {
    const uint2 cd = q == 0 ? make_uint2(__float_as_uint(wn.v), (uint32_t)wn.i) : make_uint2(0xff800000u, 0x7fffffffu);
    *reinterpret_cast<uint2*>(pc + 2 * q) = cd;
  }
}

// The dense pass of a guide kernel, after its state write-back. s_map: bit t says token t is allowed, read one BYTE per
// 16-B group. A barred entry becomes bf16 -inf (0xFF80), an allowed entry keeps its exact bits; a group with no allowed
// entry is stored without being loaded, a group with all eight allowed is not stored: at most one load and one store
// per group. pc != nullptr: the row's LM-head candidates (lm_parts pairs) are rewritten with the best ALLOWED entry.
template <int T>
__device__ __forceinline__ void guide_mask_row(bf16_t* row, int vocab, const uint32_t* s_map, uint32_t* pc,
                                               int lm_parts) {
  const uint8_t* map8 = reinterpret_cast<const uint8_t*>(s_map);
  constexpr int AU = 4;  // 16-B groups per lane in flight
  Best best{-INFINITY, 0x7fffffff};
  for (int i0 = threadIdx.x * 8; i0 < vocab; i0 += T * 8 * AU) {
    uint4 lv[AU];
    uint32_t mb[AU];
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int i = i0 + u * T * 8;
      mb[u] = 0u;
      if (i < vocab) {
        mb[u] = (uint32_t)map8[i >> 3];
        if (mb[u] != 0u) lv[u] = *reinterpret_cast<const uint4*>(row + i);
      }
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int i = i0 + u * T * 8;
      if (i >= vocab) continue;
      const uint32_t m = mb[u];
      if (m == 0u) {  // nothing allowed here: the group was not loaded
        *reinterpret_cast<uint4*>(row + i) = make_uint4(GUIDE_NINF2, GUIDE_NINF2, GUIDE_NINF2, GUIDE_NINF2);
        continue;
      }
      uint32_t w[4] = {lv[u].x, lv[u].y, lv[u].z, lv[u].w};
      if (m != 0xffu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!(m & (1u << (2 * j)))) w[j] = (w[j] & 0xffff0000u) | 0xFF80u;
          if (!(m & (1u << (2 * j + 1)))) w[j] = (w[j] & 0x0000ffffu) | 0xFF800000u;
        }
        *reinterpret_cast<uint4*>(row + i) = make_uint4(w[0], w[1], w[2], w[3]);
      }
      if (pc != nullptr) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (m & (1u << j)) {
            const uint32_t h = (j & 1) ? (w[j >> 1] & 0xffff0000u) : (w[j >> 1] << 16);
            best = better(best, Best{__uint_as_float(h), i + j});
          }
        }
      }
    }
  }
  if (pc == nullptr) return;  // uniform
  write_best_candidate<T>(best, pc, lm_parts);
}

// A chain's next eight bytes, lowest first, in one load: the walks call it every eighth level (uniform), so that the
// levels between depend on the trans lookup alone. act: the chain reads at p; the window [q, q + 8) is pulled back from
// the table's end (the launchers require bytes_len >= 8), p - q <= 7 because p < e <= bytes_len. A chain with nothing
// to read loads the table's head: the loads stay unconditional, so a lane's chains issue theirs together.
__device__ __forceinline__ unsigned long long guide_next_bytes(const uint8_t* __restrict__ tok_bytes, int bytes_len,
                                                               bool act, int p) {
  const int q = act ? (p < bytes_len - 8 ? p : bytes_len - 8) : 0;
  unsigned long long x;
  __builtin_memcpy(&x, tok_bytes + q, 8);
  return x >> (8 * (act ? p - q : 0));
}

// A wave's 64 verdicts (alive: this lane's token t is allowed) become two bitmap words by ballot: plain LDS stores, no
// atomics. Every lane of the wave calls it; the wave's tokens start at a multiple of 64.
__device__ __forceinline__ void guide_write_verdicts(uint32_t* s_map, int map_words, int t, bool alive) {
  const int lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(alive);
  const int wi = (t - lane) >> 5;
  if (lane == 0) {
    if (wi < map_words) s_map[wi] = (uint32_t)m;
    if (wi + 1 < map_words) s_map[wi + 1] = (uint32_t)(m >> 32);
  }
}

// The arguments every guide launcher checks; *map_words: the bitmap's 32-bit words.
static inline bool guide_row_args_ok(int vocab, int64_t stride, int rows, int num_slots, const uint32_t* lm_part,
                                     int lm_parts, int* map_words) {
  *map_words = (vocab / 8 + 3) / 4;
  return vocab > 0 && vocab % 8 == 0 && rows >= 0 && num_slots >= 1 && stride >= vocab && stride % 8 == 0 &&
         (lm_part == nullptr || lm_parts >= 1) && *map_words * 4 <= GUIDE_MAX_MAP_BYTES;
}

// The vocabulary's byte table. bytes_len >= 8: the walk fetches a token's bytes eight at a time, from a window that
// lies inside the table.
static inline bool guide_tok_table_ok(int64_t n_tok, int64_t bytes_len) {
  return n_tok >= 1 && n_tok <= GUIDE_TOK_TABLE_MAX && bytes_len >= 8 && bytes_len <= GUIDE_TOK_BYTES_MAX;
}

// More than 64 KiB of dynamic LDS has to be asked for, once per device. asked: the calling launcher's own flags.
static inline hipError_t guide_ask_dynamic_lds(const void* kernel, int bytes, bool (&asked)[64]) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidValue;
  if (!asked[dev]) {
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    asked[dev] = true;
  }
  return hipSuccess;
}

}  // namespace die
