// Host launchers of the FP8 (OCP e4m3) KV-cache kernels (attention_kv8.hip). As launchers.h: raw pointers and an
// explicit stream, no allocation, no synchronisation. The cache is the paged layout of the bf16 pool at one byte per
// element, [blocks, hkv, block_size, head_dim]; a stored byte is e4m3(x / scale), nearest-even, saturated to +-448.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.h"

namespace die {

// rope_cache_kernel's op with an e4m3 cache: k rotated (and q, bf16 in place, when rot_q), k / v scaled by row_scale
// (optional), divided by their scales and written as bytes. head_dim 128.
hipError_t launch_rope_and_cache_kv8(bf16_t* qkv, int64_t qkv_stride, const int64_t* positions, const float* cos_sin,
                                     const int64_t* slot_mapping, uint8_t* k_cache, uint8_t* v_cache, int num_tokens,
                                     int hq, int hkv, int head_dim, int block_size, float k_scale, float v_scale,
                                     bool rot_q, const float* row_scale, hipStream_t s);
// rope_cache_slab_kernel's op with an e4m3 cache: fp32 split-K slabs [sk][T][(hq + 2 hkv) * 128] summed, q -> q_out bf16
hipError_t launch_rope_and_cache_slab_kv8(bf16_t* q_out, const float* slab, int sk, const int64_t* positions,
                                          const float* cos_sin, const int64_t* slot_mapping, uint8_t* k_cache,
                                          uint8_t* v_cache, int num_tokens, int hq, int hkv, int head_dim,
                                          int block_size, float k_scale, float v_scale, hipStream_t s);
// decode attention over an e4m3 cache: block_size 16, head_dim 128, hq / hkv in {1, 2, 4, 8}; part_o / part_ml /
// counters are launch_attn_decode's buffers (sized by attn_decode_max_partials(max_ctx), counters zero and re-armed)
hipError_t launch_attn_decode_kv8(bf16_t* out, float* part_o, float* part_ml, int* counters, const bf16_t* q,
                                  int64_t q_stride, const uint8_t* k_cache, const uint8_t* v_cache,
                                  const int* block_tables, int bt_stride, const int* ctx_lens, int num_seqs, int max_ctx,
                                  int hq, int hkv, int head_dim, int block_size, float scale, float k_scale,
                                  float v_scale, bool kv_once, hipStream_t s);
// the same with the fused prologue (attn_decode_kv8_kernel<G, true>): q and the new token's K / V are built from the
// operands of launch_attn_decode's AttnDecodeFuse (fz.ts is ignored), the new row is written to the cache as e4m3
// bytes (slot_mapping < 0: not written) and attended to in this step. hipErrorInvalidValue when the slab staging,
// ((sk (G + 2) + 1) / 2) * 1024 + 2048 bytes, does not fit its 27 KiB of LDS, or num_seqs > DECODE_SSP_LD.
hipError_t launch_attn_decode_fused_kv8(bf16_t* out, float* part_o, float* part_ml, int* counters, uint8_t* k_cache,
                                        uint8_t* v_cache, const int* block_tables, int bt_stride, const int* ctx_lens,
                                        int num_seqs, int max_ctx, int hq, int hkv, int head_dim, int block_size,
                                        float scale, float k_scale, float v_scale, const AttnDecodeFuse* fz,
                                        bool kv_once, hipStream_t s);
// keys per part of the launches above (a context longer than this is cut into parts merged by ticket)
int attn_decode_kv8_part_keys(int num_seqs, int hkv, int max_ctx);
// launch_attn_prefill over an e4m3 cache
hipError_t launch_attn_prefill_kv8(bf16_t* out, const bf16_t* q, int64_t q_stride, const uint8_t* k_cache,
                                   const uint8_t* v_cache, const int* block_tables, int bt_stride, const int* cu_q,
                                   const int* ctx_lens, int num_seqs, int max_q_len, int hq, int hkv, int head_dim,
                                   int block_size, float scale, float k_scale, float v_scale, const float* cos_sin,
                                   int n_pos, const float* q_scale, hipStream_t s);

}  // namespace die
