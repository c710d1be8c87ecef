// Logit processing for gfx950: repetition / frequency / presence penalties and logit_bias applied to a step's
// bf16 logits rows IN PLACE, before the sampler reads them. One 1024-thread workgroup per batch row; row r maps
// through slot[r] to per-sequence state (slot[r] < 0, or beyond the table: the workgroup exits at once and the
// row's bytes stay as they are):
//   * state[slot][vocab] uint16: bit 15 = "token occurs in the prompt", bits 0-14 = how often the token was
//     generated (saturating at 32767);
//   * params[slot] = (rp, inv_rp, freq, pres): the host passes inv_rp = fp32(1 / rp), the kernel never divides;
//   * a bias list of at most LOGIT_BIAS_MAX (id, value) pairs, ids unique (validated on the host).
// Contract (tests/logit_process_reference.py is the oracle; tests/test_logit_process_kernel_gpu.py compares bit
// for bit). From the bf16 logit z of token t with output count c, each step ONE individually rounded fp32
// operation (add_rn / mul_rn / sub_rn below, compiled with contraction off: no FMA):
//   1. x = float(z) + bias[t]                (0 where the list has no entry for t)
//   2. if t is in the prompt or c > 0:       x = x > 0 ? x * inv_rp : x * rp
//   3. x = x - freq * float(c)
//   4. if c > 0:                             x = x - pres
//   5. one rounding to bf16.
// count_ids != nullptr: count_ids[r] is this step's INPUT token (the previous step's sample, not yet counted):
// it is counted first, by the thread that owns the token's 16-B group — that thread alone reads and writes the
// entry, so no ordering between threads is needed. The bias list becomes a bitmap in LDS (one BYTE per 16-B
// group of 8 entries, vocab / 8 bytes) and a 1024-slot open-addressing table id -> value: the dense pass reads its
// group's byte and probes the table only where a bit is set (a linear search of the list there cost 480 us at
// 32 rows x 300 entries: most wave iterations hold a biased lane), so biased entries are rounded once like
// every other entry.
// lm_part != nullptr: the row's LM-head candidates (sample_kernel's lm_part path) are overwritten so that they
// agree with the rewritten row: candidate 0 = the processed row's (max, lowest index) in better()'s total order
// (sampling.hip), the others (-inf, 0x7fffffff); the unchanged sampling tail then yields the processed argmax.
// Rows stream 16 B per lane (logits load + state load + logits store: 750 KiB per 128256-entry row).
#include "guide_common.h"  // Best, better() and the candidate write, shared with the guide kernels

// The five steps must stay five roundings. The __fadd_rn / __fmul_rn / __fsub_rn of this toolchain's headers are plain
// operators compiled under HIP's default -ffp-contract=fast-honor-pragmas, so step 3 was fused into one v_fma_f32
// (x - freq * c with an exact product): on tests/logit_process_reference.py's `rounding` rows (shape_1016, row 2) 29
// bf16 values differed from the CPU path. The operators below are this file's own, under a pragma that no build flag
// overrides.
#pragma clang fp contract(off)

namespace die {

constexpr int LPT = 1024;
constexpr int LP_MAX_MAP_BYTES = 48 * 1024;  // the bitmap's share of LDS: vocab <= 393216
constexpr int LP_HASH = 1024;                // bias table slots (>= 3 x LOGIT_BIAS_MAX: short probe chains)
constexpr uint32_t LP_EMPTY = 0xffffffffu;
static_assert(LP_HASH >= 2 * LOGIT_BIAS_MAX && (LP_HASH & (LP_HASH - 1)) == 0, "bias table size");

__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }

__device__ __forceinline__ uint32_t lp_hash(uint32_t id) { return (id * 2654435761u) >> 22; }  // 10 bits

__global__ void __launch_bounds__(LPT) logit_process_kernel(bf16_t* __restrict__ logits, int64_t stride, int vocab,
                                                            const int* __restrict__ slot_of_row, int num_slots,
                                                            uint16_t* __restrict__ state,
                                                            const float4* __restrict__ params,
                                                            const int* __restrict__ bias_cnt,
                                                            const int* __restrict__ bias_ids,
                                                            const float* __restrict__ bias_vals, int bias_cap,
                                                            const int64_t* __restrict__ count_ids,
                                                            uint32_t* __restrict__ lm_part, int lm_parts) {
  extern __shared__ uint32_t s_map[];  // bit t: token t has a bias entry
  __shared__ uint32_t s_key[LP_HASH];
  __shared__ float s_val[LP_HASH];
  const int r = blockIdx.x;
  const int slot = slot_of_row[r];
  if (slot < 0 || slot >= num_slots) return;  // uniform
  bf16_t* row = logits + (int64_t)r * stride;
  uint16_t* srow = state + (int64_t)slot * vocab;
  const float4 pr = params[slot];
  const float rp = pr.x, inv_rp = pr.y, freq = pr.z, pres = pr.w;
  int64_t cid = -1;
  if (count_ids != nullptr) {
    cid = count_ids[r];
    if (cid < 0 || cid >= vocab) cid = -1;
  }
  const int nb = bias_cap > 0 ? min(max(bias_cnt[slot], 0), bias_cap) : 0;
  if (nb > 0) {  // uniform
    const int words = (vocab / 8 + 3) / 4;
    for (int w = threadIdx.x; w < words; w += LPT) s_map[w] = 0u;
    for (int w = threadIdx.x; w < LP_HASH; w += LPT) s_key[w] = LP_EMPTY;
    __syncthreads();
    for (int t = threadIdx.x; t < nb; t += LPT) {
      const int id = bias_ids[(int64_t)slot * bias_cap + t];
      if (id < 0 || id >= vocab) continue;
      atomicOr(&s_map[id >> 5], 1u << (id & 31));
      // at most LOGIT_BIAS_MAX of the LP_HASH slots fill, so a free one is always met
      for (uint32_t h = lp_hash((uint32_t)id);; h = (h + 1) & (LP_HASH - 1)) {
        const uint32_t prev = atomicCAS(&s_key[h], LP_EMPTY, (uint32_t)id);
        if (prev == LP_EMPTY || prev == (uint32_t)id) {
          s_val[h] = bias_vals[(int64_t)slot * bias_cap + t];
          break;
        }
      }
    }
    __syncthreads();
  }
  const uint8_t* map8 = reinterpret_cast<const uint8_t*>(s_map);

  constexpr int AU = 4;  // 16-B groups per lane in flight (logits and state: 8 loads)
  Best best{-INFINITY, 0x7fffffff};
  for (int i0 = threadIdx.x * 8; i0 < vocab; i0 += LPT * 8 * AU) {
    uint4 lv[AU], sv[AU];
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int i = i0 + u * LPT * 8;
      if (i < vocab) {
        lv[u] = *reinterpret_cast<const uint4*>(row + i);
        sv[u] = *reinterpret_cast<const uint4*>(srow + i);
      }
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int i = i0 + u * LPT * 8;
      if (i >= vocab) continue;
      float z[8], o[8];
      unpack8(lv[u], z);
      const uint32_t sw[4] = {sv[u].x, sv[u].y, sv[u].z, sv[u].w};
      const uint32_t mb = nb > 0 ? (uint32_t)map8[i >> 3] : 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t st = (j & 1) ? (sw[j >> 1] >> 16) : (sw[j >> 1] & 0xffffu);
        float b = 0.f;
        if (mb & (1u << j)) {  // at most LOGIT_BIAS_MAX entries of the row; the bit says the id is in the table
          uint32_t h = lp_hash((uint32_t)(i + j));
          for (int probe = 0; probe < LP_HASH && s_key[h] != (uint32_t)(i + j); ++probe) h = (h + 1) & (LP_HASH - 1);
          b = s_key[h] == (uint32_t)(i + j) ? s_val[h] : 0.f;
        }
        uint32_t c = st & 0x7fffu;
        if ((int64_t)(i + j) == cid) {
          c = c < 0x7fffu ? c + 1u : c;
          srow[i + j] = (uint16_t)((st & 0x8000u) | c);
        }
        float x = add_rn(z[j], b);
        if ((st & 0x8000u) != 0u || c > 0u) x = x > 0.f ? mul_rn(x, inv_rp) : mul_rn(x, rp);
        x = sub_rn(x, mul_rn(freq, (float)c));
        if (c > 0u) x = sub_rn(x, pres);
        o[j] = x;
      }
      const uint4 ov = pack8(o);
      *reinterpret_cast<uint4*>(row + i) = ov;
      if (lm_part != nullptr) {
        unpack8(ov, o);  // the values as the sampler will read them
#pragma unroll
        for (int j = 0; j < 8; ++j) best = better(best, Best{o[j], i + j});
      }
    }
  }
  if (lm_part == nullptr) return;  // uniform
  write_best_candidate<LPT>(best, lm_part + (int64_t)r * lm_parts * 2, lm_parts);
}

hipError_t launch_logit_process(bf16_t* logits, int64_t stride, int rows, int vocab, const int* slot, int num_slots,
                                uint16_t* state, const float* params, const int* bias_cnt, const int* bias_ids,
                                const float* bias_vals, int bias_cap, const int64_t* count_ids, uint32_t* lm_part,
                                int lm_parts, hipStream_t s) {
  if (state == nullptr || vocab <= 0 || vocab % 8 || bias_cap < 0 || bias_cap > LOGIT_BIAS_MAX)
    return hipErrorInvalidValue;
  if (rows < 0 || num_slots < 1 || logits == nullptr || slot == nullptr || params == nullptr || stride < vocab ||
      stride % 8)
    return hipErrorInvalidValue;
  if (bias_cap > 0 && (bias_cnt == nullptr || bias_ids == nullptr || bias_vals == nullptr)) return hipErrorInvalidValue;
  if (lm_part != nullptr && lm_parts < 1) return hipErrorInvalidValue;
  const int map_bytes = ((vocab / 8 + 3) / 4) * 4;
  if (map_bytes > LP_MAX_MAP_BYTES) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(logit_process_kernel, dim3(rows), dim3(LPT), map_bytes, s, logits, stride, vocab, slot, num_slots,
                     state, reinterpret_cast<const float4*>(params), bias_cnt, bias_ids, bias_vals, bias_cap,
                     count_ids, lm_part, lm_parts);
  return hipGetLastError();
}

}  // namespace die
