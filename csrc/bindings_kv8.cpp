// Torch bindings of the FP8 KV-cache kernels (module `src._C_kv8`, csrc/kernels/attention_kv8.hip). A second module
// next to `_C` with the same rules (bindings.cpp): every entry point validates device, dtype, shape and contiguity
// through the vocabulary of arg_check.h before anything is launched on the current stream, and no tensor is asked
// for its address here. What is new: a cache must be one-byte elements (uint8 or float8_e4m3fn) and the two scales
// finite and positive.
#include <cmath>

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "arg_check.h"
#include "kernels/kv8.h"

using torch::Tensor;
using chk::ANY;
using chk::ge;
using chk::Op;
using die::bf16_t;

namespace {

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_only(bool on) { chk::g_check_only = on; }

constexpr int64_t HEAD_DIM = 128;

// [num_blocks, num_kv_heads, block_size, 128] of e4m3 bytes, 16-byte aligned (the kernels move 16-byte groups)
uint8_t* check_cache8(const Op& a, const Tensor& c, int64_t hkv, const char* name) {
  TORCH_CHECK(c.scalar_type() == at::kByte || c.scalar_type() == at::kFloat8_e4m3fn, a.op, ": ", name,
              " must be uint8 or float8_e4m3fn, got ", c.scalar_type());
  return static_cast<uint8_t*>(a.dense<void>(c, name, 0, {ANY, hkv, ANY, HEAD_DIM}, 16));
}

struct Scales {
  float k, v;
};
Scales check_scales(const Op& a, double k_scale, double v_scale) {
  TORCH_CHECK(std::isfinite(k_scale) && std::isfinite(v_scale) && k_scale > 0 && v_scale > 0 &&
                  std::isfinite((float)k_scale) && std::isfinite((float)v_scale) && (float)k_scale > 0.f &&
                  (float)v_scale > 0.f,
              a.op, ": k_scale and v_scale must be finite and > 0, got ", k_scale, ", ", v_scale);
  return {(float)k_scale, (float)v_scale};
}

struct Caches {
  uint8_t *k, *v;
  int bs;
};
Caches check_caches(const Op& a, const Tensor& k_cache, const Tensor& v_cache, int64_t hkv) {
  Caches c{check_cache8(a, k_cache, hkv, "k_cache"), check_cache8(a, v_cache, hkv, "v_cache"), 0};
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), a.op, ": k/v cache shapes differ");
  c.bs = a.i32(k_cache.size(2));
  TORCH_CHECK(c.bs >= 1, a.op, ": empty cache blocks");
  return c;
}

struct RopeIndex {
  const int64_t *pos, *slots;
  const float* cos_sin;
};
RopeIndex check_rope_index(const Op& a, const Tensor& positions, const Tensor& slot_mapping, const Tensor& cos_sin,
                           int64_t tokens) {
  return {a.dense<int64_t>(positions, "positions", tokens), a.dense<int64_t>(slot_mapping, "slot_mapping", tokens),
          a.dense<float>(cos_sin, "cos_sin", 0, {ANY, HEAD_DIM}, 16)};
}

void rope_and_cache_kv8(Tensor qkv, Tensor positions, Tensor cos_sin, Tensor slot_mapping, Tensor k_cache,
                        Tensor v_cache, int64_t hq, int64_t hkv, double k_scale, double v_scale, bool rot_q,
                        Tensor row_scale) {
  const Op a("rope_and_cache_kv8", qkv, "qkv");
  const auto q = a.rows(qkv, "qkv");
  const int T = a.i32(qkv.size(0));
  TORCH_CHECK(hq >= 1 && hkv >= 1 && qkv.size(1) >= (hq + 2 * hkv) * HEAD_DIM,
              "rope_and_cache_kv8: qkv width < (hq + 2*hkv) * 128 (head_dim must be 128)");
  const RopeIndex ix = check_rope_index(a, positions, slot_mapping, cos_sin, T);
  const Caches c = check_caches(a, k_cache, v_cache, hkv);
  const Scales sc = check_scales(a, k_scale, v_scale);
  const float* rs = a.dense_opt<float>(row_scale, "row_scale", T);
  LAUNCH(launch_rope_and_cache_kv8(q.p, q.ld, ix.pos, ix.cos_sin, ix.slots, c.k, c.v, T, a.i32(hq), a.i32(hkv),
                                   (int)HEAD_DIM, c.bs, sc.k, sc.v, rot_q, rs, cur_stream()));
}

void rope_and_cache_slab_kv8(Tensor q_out, Tensor slab, Tensor positions, Tensor cos_sin, Tensor slot_mapping,
                             Tensor k_cache, Tensor v_cache, int64_t hq, int64_t hkv, double k_scale, double v_scale) {
  const Op a("rope_and_cache_slab_kv8", slab, "slab");
  TORCH_CHECK(hq >= 1 && hkv >= 1, "rope_and_cache_slab_kv8: hq, hkv >= 1");
  const float* sp = a.dense<float>(slab, "slab", 0, {ge(1), ANY, (hq + 2 * hkv) * HEAD_DIM}, 16);
  const int T = a.i32(slab.size(1));
  bf16_t* qp = a.dense<bf16_t>(q_out, "q_out", T * hq * HEAD_DIM, {}, 16);
  const RopeIndex ix = check_rope_index(a, positions, slot_mapping, cos_sin, T);
  const Caches c = check_caches(a, k_cache, v_cache, hkv);
  const Scales sc = check_scales(a, k_scale, v_scale);
  LAUNCH(launch_rope_and_cache_slab_kv8(qp, sp, a.i32(slab.size(0)), ix.pos, ix.cos_sin, ix.slots, c.k, c.v, T,
                                        a.i32(hq), a.i32(hkv), (int)HEAD_DIM, c.bs, sc.k, sc.v, cur_stream()));
}

// part_o / part_ml: fp32 [>= num_seqs * hq * decode_partials(max_ctx) * 128 / * 2]; counters: int32 [>= num_seqs *
// hkv], zero before first use (the kernel re-arms them): the bf16 decode attention's buffers.
void attn_decode_kv8(Tensor out, Tensor part_o, Tensor part_ml, Tensor counters, Tensor q, Tensor k_cache,
                     Tensor v_cache, Tensor block_tables, Tensor ctx_lens, int64_t max_ctx, int64_t hq, int64_t hkv,
                     double scale, double k_scale, double v_scale, bool kv_once) {
  const Op a("attn_decode_kv8", q, "q");
  const int64_t D = HEAD_DIM;
  TORCH_CHECK(hkv >= 1 && hq % hkv == 0, "attn_decode_kv8: hq % hkv");
  const int64_t G = hq / hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8, "attn_decode_kv8: hq / hkv in {1, 2, 4, 8}, got ", G);
  const int* ctx = a.dense<int>(ctx_lens, "ctx_lens", 0);
  const int nseq = a.i32(ctx_lens.numel());
  const Caches c = check_caches(a, k_cache, v_cache, hkv);
  TORCH_CHECK(c.bs == 16, "attn_decode_kv8: block_size 16, got ", c.bs);
  const int* bt = a.dense<int>(block_tables, "block_tables", 0, {ge(nseq), ge(1)});
  TORCH_CHECK(max_ctx >= 1 && block_tables.size(1) * c.bs >= max_ctx, "attn_decode_kv8: block table narrower than max_ctx");
  const int64_t maxp = (a.i32(max_ctx) + 127) / 128;  // _C.decode_partials: one partial per 128-key chunk
  float* po = a.dense<float>(part_o, "part_o", nseq * hq * maxp * D, {}, 16);
  float* pm = a.dense<float>(part_ml, "part_ml", nseq * hq * maxp * 2, {}, 8);
  int* cnt = a.dense<int>(counters, "counters", nseq * hkv);
  const auto qr = a.rows(q, "q", ge(nseq), ge(hq * D));
  bf16_t* op = a.dense<bf16_t>(out, "out", nseq * hq * D, {}, 16);
  const Scales sc = check_scales(a, k_scale, v_scale);
  LAUNCH(launch_attn_decode_kv8(op, po, pm, cnt, qr.p, qr.ld, c.k, c.v, bt, a.i32(block_tables.size(1)), ctx, nseq,
                                a.i32(max_ctx), a.i32(hq), a.i32(hkv), (int)D, c.bs, (float)scale, sc.k, sc.v, kv_once,
                                cur_stream()));
}

// _C's attn_decode_fused over an e4m3 cache: q / the new K, V built from the qkv projection's fp32 split-K slabs
// [sk, M, (hq + 2 hkv) * 128] (RMSNorm row scale from ssp [tiles, 128], RoPE from cos_sin [max_pos, 128] at position
// ctx_len - 1); the new row goes to the paged cache at slot_mapping as e4m3(x / scale).
void attn_decode_fused_kv8(Tensor out, Tensor part_o, Tensor part_ml, Tensor counters, Tensor slab, Tensor ssp,
                           Tensor positions, Tensor cos_sin, Tensor slot_mapping, Tensor k_cache, Tensor v_cache,
                           Tensor block_tables, Tensor ctx_lens, int64_t max_ctx, int64_t hq, int64_t hkv, double scale,
                           double eps, int64_t hidden, double k_scale, double v_scale, bool kv_once) {
  const Op a("attn_decode_fused_kv8", slab, "slab");
  const int64_t D = HEAD_DIM;
  TORCH_CHECK(hkv >= 1 && hq % hkv == 0, "attn_decode_fused_kv8: hq % hkv");
  const int64_t G = hq / hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8, "attn_decode_fused_kv8: hq / hkv in {1, 2, 4, 8}, got ", G);
  const int* ctx = a.dense<int>(ctx_lens, "ctx_lens", 0);
  const int nseq = a.i32(ctx_lens.numel());
  const Caches c = check_caches(a, k_cache, v_cache, hkv);
  TORCH_CHECK(c.bs == 16, "attn_decode_fused_kv8: block_size 16, got ", c.bs);
  const int* bt = a.dense<int>(block_tables, "block_tables", 0, {ge(nseq), ge(1)});
  TORCH_CHECK(max_ctx >= 1 && block_tables.size(1) * c.bs >= max_ctx,
              "attn_decode_fused_kv8: block table narrower than max_ctx");
  const int64_t maxp = (a.i32(max_ctx) + 127) / 128;
  float* po = a.dense<float>(part_o, "part_o", nseq * hq * maxp * D, {}, 16);
  float* pm = a.dense<float>(part_ml, "part_ml", nseq * hq * maxp * 2, {}, 8);
  int* cnt = a.dense<int>(counters, "counters", nseq * hkv);
  die::AttnDecodeFuse fz;
  fz.slab = a.dense<float>(slab, "slab", 0, {ge(1), ge(nseq), (hq + 2 * hkv) * D}, 16);
  fz.sk = a.i32(slab.size(0));
  fz.slab_stride = slab.size(1) * slab.size(2);
  fz.width = a.i32(slab.size(2));
  bf16_t* op = a.dense<bf16_t>(out, "out", nseq * hq * D, {}, 16);
  fz.ssp = a.dense<float>(ssp, "ssp", 0, {ANY, die::DECODE_SSP_LD});
  TORCH_CHECK(ssp.size(0) >= 1 && ssp.size(0) <= die::DECODE_SSP_MAX_TILES && nseq <= die::DECODE_SSP_LD,
              "attn_decode_fused_kv8: ssp [tiles <= 256, 128], <= 128 sequences");
  fz.ssp_tiles = a.i32(ssp.size(0));
  TORCH_CHECK(hidden >= 1, "attn_decode_fused_kv8: hidden >= 1");
  fz.inv_n = 1.f / (float)hidden;
  fz.eps = (float)eps;
  // decode: every sequence's new token sits at position ctx_len - 1 <= max_ctx - 1 (the kernel reads that table row)
  const RopeIndex ix = check_rope_index(a, positions, slot_mapping, cos_sin, nseq);
  TORCH_CHECK(cos_sin.size(0) >= max_ctx, "attn_decode_fused_kv8: cos_sin has fewer rows than max_ctx");
  fz.cos_sin = ix.cos_sin;
  fz.slot_mapping = ix.slots;
  const Scales sc = check_scales(a, k_scale, v_scale);
  LAUNCH(launch_attn_decode_fused_kv8(op, po, pm, cnt, c.k, c.v, bt, a.i32(block_tables.size(1)), ctx, nseq,
                                      a.i32(max_ctx), a.i32(hq), a.i32(hkv), (int)D, c.bs, (float)scale, sc.k, sc.v,
                                      &fz, kv_once, cur_stream()));
}

int64_t decode_part_keys(int64_t num_seqs, int64_t hkv, int64_t max_ctx) {
  return die::attn_decode_kv8_part_keys((int)num_seqs, (int)hkv, (int)max_ctx);
}

void attn_prefill_kv8(Tensor out, Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor cu_q,
                      Tensor ctx_lens, int64_t max_q_len, int64_t hq, int64_t hkv, double scale, double k_scale,
                      double v_scale, Tensor cos_sin, Tensor q_scale) {
  const Op a("attn_prefill_kv8", q, "q");
  const int64_t D = HEAD_DIM;
  const auto qr = a.rows(q, "q");
  const int64_t T = q.size(0);
  TORCH_CHECK(q.size(1) >= hq * D, "attn_prefill_kv8: q width < hq*128 (head_dim must be 128)");
  bf16_t* op = a.dense<bf16_t>(out, "out", T * hq * D, {}, 16);
  TORCH_CHECK(hkv >= 1 && hq % hkv == 0 && (hq / hkv) <= 32 && (32 % (hq / hkv)) == 0,
              "attn_prefill_kv8: hq/hkv must divide 32");
  const Caches c = check_caches(a, k_cache, v_cache, hkv);
  TORCH_CHECK(c.bs % 16 == 0, "attn_prefill_kv8: block_size a multiple of 16, got ", c.bs);
  const int* ctx = a.dense<int>(ctx_lens, "ctx_lens", 0);
  const int nseq = a.i32(ctx_lens.numel());
  const int* cu = a.dense<int>(cu_q, "cu_q", nseq + 1);
  const int* bt = a.dense<int>(block_tables, "block_tables", 0, {ge(nseq), ge(1)});
  const float* cs = a.dense_opt<float>(cos_sin, "cos_sin", 0, {ANY, D});
  const int n_pos = cs ? a.i32(cos_sin.size(0)) : 0;
  const float* qs = a.dense_opt<float>(q_scale, "q_scale", T);
  TORCH_CHECK(qs == nullptr || cs != nullptr, "attn_prefill_kv8: q_scale is applied with the rotation (cos_sin)");
  const Scales sc = check_scales(a, k_scale, v_scale);
  LAUNCH(launch_attn_prefill_kv8(op, qr.p, qr.ld, c.k, c.v, bt, a.i32(block_tables.size(1)), cu, ctx, nseq,
                                 a.i32(max_q_len), a.i32(hq), a.i32(hkv), (int)D, c.bs, (float)scale, sc.k, sc.v, cs,
                                 n_pos, qs, cur_stream()));
}

}  // namespace

PYBIND11_MODULE(_C_kv8, m) {
  m.doc() = "gfx950 HIP kernels of the FP8 (e4m3) KV cache";
  m.def("rope_and_cache_kv8", &rope_and_cache_kv8);
  m.def("rope_and_cache_slab_kv8", &rope_and_cache_slab_kv8);
  m.def("attn_decode_kv8", &attn_decode_kv8);
  m.def("attn_decode_fused_kv8", &attn_decode_fused_kv8);
  m.def("attn_prefill_kv8", &attn_prefill_kv8);
  m.def("decode_part_keys", &decode_part_keys);
  m.def("check_only", &check_only);
}
