// Torch bindings of the gfx950 kernels (module `src._C`). Each entry point
// validates device/dtype/shape up front and throws on mismatch — a wrong shape
// never reaches a kernel (a faulting kernel can take down every GPU on the
// host) — then launches on the current HIP stream (graph-capture safe).
#include <cstdlib>

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "kernels/gd_tiles.h"
#include "kernels/launchers.h"

using torch::Tensor;

namespace {

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline die::bf16_t* bf(const Tensor& t) { return reinterpret_cast<die::bf16_t*>(t.data_ptr()); }

#define CHK_CUDA(x) TORCH_CHECK((x).is_cuda(), #x " must be a GPU tensor")
#define CHK_BF16(x) TORCH_CHECK((x).scalar_type() == at::kBFloat16, #x " must be bfloat16")
#define CHK_DTYPE(x, d) TORCH_CHECK((x).scalar_type() == (d), #x " has wrong dtype")
#define CHK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")
#define HIP_OK(call)                                                                 \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    TORCH_CHECK(e_ == hipSuccess, "HIP launch failed: ", hipGetErrorString(e_), " (", \
                #call, ")");                                                          \
  } while (0)

inline void check_rows(const Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() == 2, name, " must be 2-D [rows, hidden]");
  TORCH_CHECK(t.stride(1) == 1, name, " rows must be contiguous");
  TORCH_CHECK(t.stride(0) % 8 == 0, name, " row stride must be a multiple of 8 elements");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

void rms_norm(Tensor out, Tensor x, Tensor w, double eps) {
  CHK_CUDA(x);
  CHK_BF16(x);
  CHK_BF16(out);
  CHK_BF16(w);
  check_rows(x, "x");
  check_rows(out, "out");
  TORCH_CHECK(out.size(0) == x.size(0) && out.size(1) == x.size(1) && w.numel() == x.size(1), "rms_norm shapes");
  TORCH_CHECK(x.size(1) <= 8 * 256 * 8, "hidden too large");
  HIP_OK(die::launch_rms_norm(bf(out), bf(x), bf(w), (float)eps, (int)x.size(0), (int)x.size(1), x.stride(0),
                               out.stride(0), cur_stream()));
}

void fused_add_rms_norm(Tensor out, Tensor x, Tensor residual, Tensor w, double eps) {
  CHK_CUDA(x);
  CHK_BF16(x);
  CHK_BF16(out);
  CHK_BF16(residual);
  CHK_BF16(w);
  check_rows(x, "x");
  check_rows(out, "out");
  CHK_CONTIG(residual);
  TORCH_CHECK(residual.size(0) == x.size(0) && residual.size(1) == x.size(1), "residual shape");
  TORCH_CHECK(out.size(0) == x.size(0) && out.size(1) == x.size(1) && w.numel() == x.size(1), "norm shapes");
  TORCH_CHECK(x.size(1) <= 8 * 256 * 8, "hidden too large");
  HIP_OK(die::launch_fused_add_rms_norm(bf(out), bf(x), bf(residual), bf(w), (float)eps, (int)x.size(0),
                                         (int)x.size(1), x.stride(0), out.stride(0), cur_stream()));
}

// row_scale (optional, numel 0 = absent): fp32 [T] RMSNorm row scale applied to gate and up (prefill with the
// norm weight folded into Wgate_up)
static const float* opt_row_scale(const Tensor& rs, int64_t rows, const Tensor& like, const char* name) {
  if (rs.numel() == 0) return nullptr;
  CHK_DTYPE(rs, at::kFloat);
  CHK_CONTIG(rs);
  TORCH_CHECK(rs.device() == like.device() && rs.numel() >= rows, name, ": row scale [T] fp32 on the same device");
  return rs.data_ptr<float>();
}

void silu_and_mul(Tensor out, Tensor x, Tensor row_scale) {
  CHK_CUDA(x);
  CHK_BF16(x);
  CHK_BF16(out);
  CHK_CONTIG(x);
  CHK_CONTIG(out);
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2 && x.size(1) == 2 * out.size(1) && x.size(0) == out.size(0),
              "silu_and_mul: x [T, 2I], out [T, I]");
  TORCH_CHECK(out.size(1) % 8 == 0, "intermediate size must be a multiple of 8");
  HIP_OK(die::launch_silu_and_mul(bf(out), bf(x), (int)x.size(0), (int)out.size(1), cur_stream(),
                                  opt_row_scale(row_scale, x.size(0), x, "silu_and_mul")));
}

// silu(gate) * up on [T, I] row views (unit column stride, 16-byte aligned rows; gate and up share a row stride).
void silu_and_mul_views(Tensor out, Tensor gate, Tensor up, Tensor row_scale, int64_t per) {
  CHK_CUDA(gate);
  CHK_BF16(gate);
  CHK_BF16(up);
  CHK_BF16(out);
  TORCH_CHECK(gate.dim() == 2 && up.sizes() == gate.sizes() && out.sizes() == gate.sizes(),
              "silu_and_mul_views: gate, up, out [T, I]");
  TORCH_CHECK(gate.stride(1) == 1 && up.stride(1) == 1 && out.stride(1) == 1 && up.stride(0) == gate.stride(0),
              "silu_and_mul_views: unit column strides, one row stride for gate and up");
  TORCH_CHECK(gate.size(1) % 8 == 0 && gate.stride(0) % 8 == 0 && out.stride(0) % 8 == 0 &&
                  (reinterpret_cast<uintptr_t>(gate.data_ptr()) | reinterpret_cast<uintptr_t>(up.data_ptr()) |
                   reinterpret_cast<uintptr_t>(out.data_ptr())) % 16 == 0,
              "silu_and_mul_views: 16-byte aligned rows");
  HIP_OK(die::launch_silu_and_mul_views(bf(out), out.stride(0), bf(gate), bf(up), gate.stride(0),
                                        (int)gate.size(0), (int)gate.size(1), cur_stream(),
                                        opt_row_scale(row_scale, gate.size(0), gate, "silu_and_mul_views"),
                                        (int)per));
}

// Prefill RMSNorm as a row scale: resid += x (x empty: no add) and rs [T] = rsqrt(mean(resid^2) + eps).
void rms_row_scale(Tensor rs, Tensor resid, Tensor x, double eps) {
  CHK_CUDA(resid);
  CHK_BF16(resid);
  check_rows(resid, "resid");
  CHK_DTYPE(rs, at::kFloat);
  CHK_CONTIG(rs);
  TORCH_CHECK(rs.device() == resid.device() && rs.numel() >= resid.size(0), "rs [T] fp32");
  const bool add = x.numel() > 0;
  if (add) {
    CHK_BF16(x);
    check_rows(x, "x");
    TORCH_CHECK(x.sizes() == resid.sizes() && x.device() == resid.device(), "x like resid");
  }
  TORCH_CHECK(resid.size(1) <= 8192, "hidden <= 8192");
  HIP_OK(die::launch_rms_row_scale(rs.data_ptr<float>(), bf(resid), add ? bf(x) : nullptr, (int)resid.size(0),
                                   (int)resid.size(1), resid.stride(0), add ? x.stride(0) : 0, (float)eps,
                                   cur_stream()));
}

void check_cache(const Tensor& c, int64_t hkv, int64_t head_dim, const char* name) {
  CHK_CUDA(c);
  CHK_BF16(c);
  CHK_CONTIG(c);
  TORCH_CHECK(c.dim() == 4 && c.size(1) == hkv && c.size(3) == head_dim, name,
              " must be [num_blocks, num_kv_heads, block_size, head_dim]");
}

// positions, slot_mapping and cos_sin reach the RoPE kernels as raw pointers: dense arrays on the rows' device
void check_rope_index(const Tensor& positions, const Tensor& slot_mapping, const Tensor& cos_sin, const Tensor& like,
                      int64_t tokens, int64_t head_dim) {
  CHK_DTYPE(positions, at::kLong);
  CHK_DTYPE(slot_mapping, at::kLong);
  CHK_DTYPE(cos_sin, at::kFloat);
  CHK_CONTIG(positions);
  CHK_CONTIG(slot_mapping);
  CHK_CONTIG(cos_sin);
  TORCH_CHECK(positions.device() == like.device() && slot_mapping.device() == like.device() &&
                  cos_sin.device() == like.device(),
              "positions, slot_mapping and cos_sin must be on the device of the rows");
  TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == head_dim, "cos_sin must be [max_pos, head_dim]");
  TORCH_CHECK(positions.numel() >= tokens && slot_mapping.numel() >= tokens, "positions/slots too short");
}

void rope_and_cache(Tensor qkv, Tensor positions, Tensor cos_sin, Tensor slot_mapping, Tensor k_cache,
                    Tensor v_cache, int64_t hq, int64_t hkv, int64_t head_dim, bool rot_q, Tensor row_scale) {
  CHK_CUDA(qkv);
  CHK_BF16(qkv);
  check_rows(qkv, "qkv");
  TORCH_CHECK(qkv.size(1) >= (hq + 2 * hkv) * head_dim, "qkv width < (hq + 2*hkv) * head_dim");
  check_rope_index(positions, slot_mapping, cos_sin, qkv, qkv.size(0), head_dim);
  check_cache(k_cache, hkv, head_dim, "k_cache");
  check_cache(v_cache, hkv, head_dim, "v_cache");
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), "k/v cache shapes differ");
  HIP_OK(die::launch_rope_and_cache(bf(qkv), qkv.stride(0), positions.data_ptr<int64_t>(), cos_sin.data_ptr<float>(),
                                     slot_mapping.data_ptr<int64_t>(), bf(k_cache), bf(v_cache), (int)qkv.size(0),
                                     (int)hq, (int)hkv, (int)head_dim, (int)k_cache.size(2), cur_stream(), rot_q,
                                     opt_row_scale(row_scale, qkv.size(0), qkv, "rope_and_cache")));
}

void attn_prefill(Tensor out, Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor cu_q,
                  Tensor ctx_lens, int64_t max_q_len, int64_t hq, int64_t hkv, double scale, Tensor cos_sin,
                  Tensor q_scale) {
  CHK_CUDA(q);
  CHK_BF16(q);
  CHK_BF16(out);
  check_rows(q, "q");
  CHK_CONTIG(out);
  const int64_t D = 128;
  TORCH_CHECK(q.size(1) >= hq * D, "q width < hq*128 (head_dim must be 128)");
  TORCH_CHECK(out.numel() >= q.size(0) * hq * D, "out too small");
  TORCH_CHECK(hq % hkv == 0 && (hq / hkv) <= 32 && (32 % (hq / hkv)) == 0, "hq/hkv must divide 32");
  check_cache(k_cache, hkv, D, "k_cache");
  check_cache(v_cache, hkv, D, "v_cache");
  CHK_DTYPE(block_tables, at::kInt);
  CHK_DTYPE(cu_q, at::kInt);
  CHK_DTYPE(ctx_lens, at::kInt);
  CHK_CONTIG(block_tables);
  const int64_t nseq = ctx_lens.numel();
  TORCH_CHECK(cu_q.numel() >= nseq + 1 && block_tables.dim() == 2 && block_tables.size(0) >= nseq,
              "cu_q / block_tables sizes");
  // cos_sin (optional, numel 0 = absent): [max_pos, 128] fp32; Q rows are rotated on load (unrotated q)
  const bool rot = cos_sin.numel() > 0;
  if (rot) {
    CHK_DTYPE(cos_sin, at::kFloat);
    CHK_CONTIG(cos_sin);
    TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == D && cos_sin.device() == q.device(),
                "cos_sin must be [max_pos, 128] on q's device");
  }
  HIP_OK(die::launch_attn_prefill(bf(out), bf(q), q.stride(0), bf(k_cache), bf(v_cache),
                                   block_tables.data_ptr<int>(), (int)block_tables.size(1), cu_q.data_ptr<int>(),
                                   ctx_lens.data_ptr<int>(), (int)nseq, (int)max_q_len, (int)hq, (int)hkv, (int)D,
                                   (int)k_cache.size(2), (float)scale, cur_stream(),
                                   rot ? cos_sin.data_ptr<float>() : nullptr, rot ? (int)cos_sin.size(0) : 0,
                                   opt_row_scale(q_scale, q.size(0), q, "attn_prefill")));
}

// counters: int32 [>= num_seqs * hkv], zero before first use (the kernel re-arms them); an empty tensor
// selects the two-kernel path (partials + merge launch).
void attn_decode(Tensor out, Tensor part_o, Tensor part_ml, Tensor counters, Tensor q, Tensor k_cache, Tensor v_cache,
                 Tensor block_tables, Tensor ctx_lens, int64_t max_ctx, int64_t hq, int64_t hkv, double scale,
                 bool kv_once) {
  CHK_CUDA(q);
  CHK_BF16(q);
  CHK_BF16(out);
  check_rows(q, "q");
  CHK_CONTIG(out);
  const int64_t D = 128;
  const int64_t nseq = ctx_lens.numel();
  TORCH_CHECK(q.size(0) >= nseq && q.size(1) >= hq * D, "q shape");
  TORCH_CHECK(out.numel() >= nseq * hq * D, "out too small");
  TORCH_CHECK(hq % hkv == 0 && (hq / hkv) <= 32, "hq/hkv <= 32");
  check_cache(k_cache, hkv, D, "k_cache");
  check_cache(v_cache, hkv, D, "v_cache");
  CHK_DTYPE(block_tables, at::kInt);
  CHK_DTYPE(ctx_lens, at::kInt);
  CHK_CONTIG(block_tables);
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) >= nseq, "block_tables shape");
  TORCH_CHECK(block_tables.size(1) * k_cache.size(2) >= max_ctx, "block table narrower than max_ctx");
  const int maxp = die::attn_decode_max_partials((int)max_ctx);
  CHK_DTYPE(part_o, at::kFloat);
  CHK_DTYPE(part_ml, at::kFloat);
  TORCH_CHECK(part_o.numel() >= nseq * hq * maxp * D && part_ml.numel() >= nseq * hq * maxp * 2,
              "partial buffers too small for max_ctx");
  int* cnt = nullptr;
  if (counters.numel() > 0) {
    CHK_DTYPE(counters, at::kInt);
    TORCH_CHECK(counters.is_cuda() && counters.numel() >= nseq * hkv, "attn counters: int32 [>= num_seqs*hkv]");
    cnt = counters.data_ptr<int>();
  }
  HIP_OK(die::launch_attn_decode(bf(out), part_o.data_ptr<float>(), part_ml.data_ptr<float>(), cnt, bf(q), q.stride(0),
                                  bf(k_cache), bf(v_cache), block_tables.data_ptr<int>(), (int)block_tables.size(1),
                                  ctx_lens.data_ptr<int>(), (int)nseq, (int)max_ctx, (int)hq, (int)hkv, (int)D,
                                  (int)k_cache.size(2), (float)scale, nullptr, kv_once, cur_stream()));
}

// Decode attention with the fused prologue: q / new K,V built from the qkv projection's
// fp32 split-K slabs [sk, M, (hq+2hkv)*128] (RMSNorm row scale from ssp [T, 32], RoPE from
// cos_sin [max_pos, 128] at positions [M]); the new K/V go to the paged cache at slot_mapping.
void attn_decode_fused(Tensor out, Tensor part_o, Tensor part_ml, Tensor counters, Tensor slab, Tensor ssp,
                       Tensor positions, Tensor cos_sin, Tensor slot_mapping, Tensor k_cache, Tensor v_cache,
                       Tensor block_tables, Tensor ctx_lens, int64_t max_ctx, int64_t hq, int64_t hkv, double scale,
                       double eps, int64_t hidden, bool kv_once) {
  CHK_CUDA(slab);
  CHK_DTYPE(slab, at::kFloat);
  CHK_CONTIG(slab);
  CHK_BF16(out);
  CHK_CONTIG(out);
  const int64_t D = 128;
  const int64_t nseq = ctx_lens.numel();
  TORCH_CHECK(slab.dim() == 3 && slab.size(1) >= nseq && slab.size(2) == (hq + 2 * hkv) * D, "slab [sk, M, width]");
  TORCH_CHECK(out.numel() >= nseq * hq * D, "out too small");
  TORCH_CHECK(hq % hkv == 0, "hq % hkv");
  const int64_t G = hq / hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8, "fused decode attention: G in {1, 2, 4, 8}");
  check_cache(k_cache, hkv, D, "k_cache");
  check_cache(v_cache, hkv, D, "v_cache");
  TORCH_CHECK(k_cache.size(2) == 16, "fused decode attention: block_size 16");
  CHK_DTYPE(block_tables, at::kInt);
  CHK_DTYPE(ctx_lens, at::kInt);
  CHK_CONTIG(block_tables);
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) >= nseq, "block_tables shape");
  TORCH_CHECK(block_tables.size(1) * 16 >= max_ctx, "block table narrower than max_ctx");
  CHK_DTYPE(ssp, at::kFloat);
  CHK_CONTIG(ssp);
  TORCH_CHECK(ssp.dim() == 2 && ssp.size(1) == die::DECODE_SSP_LD && ssp.size(0) >= 1 &&
                  ssp.size(0) <= die::DECODE_SSP_MAX_TILES,
              "ssp [tiles <= 256, 128]");
  CHK_DTYPE(positions, at::kLong);
  CHK_DTYPE(slot_mapping, at::kLong);
  CHK_DTYPE(cos_sin, at::kFloat);
  CHK_CONTIG(cos_sin);
  TORCH_CHECK(cos_sin.size(1) == D, "cos_sin [max_pos, 128]");
  TORCH_CHECK(positions.numel() >= nseq && slot_mapping.numel() >= nseq, "positions / slot_mapping");
  // decode: every sequence's new token sits at position ctx_len - 1 (the kernel uses that)
  const int maxp = die::attn_decode_max_partials((int)max_ctx);
  CHK_DTYPE(part_o, at::kFloat);
  CHK_DTYPE(part_ml, at::kFloat);
  TORCH_CHECK(part_o.numel() >= nseq * hq * maxp * D && part_ml.numel() >= nseq * hq * maxp * 2,
              "partial buffers too small for max_ctx");
  CHK_DTYPE(counters, at::kInt);
  TORCH_CHECK(counters.is_cuda() && counters.numel() >= nseq * hkv, "attn counters: int32 [>= num_seqs*hkv]");
  die::AttnDecodeFuse fz;
  fz.slab = slab.data_ptr<float>();
  fz.sk = (int)slab.size(0);
  fz.slab_stride = slab.size(1) * slab.size(2);
  fz.width = (int)slab.size(2);
  fz.ssp = ssp.data_ptr<float>();
  fz.ssp_tiles = (int)ssp.size(0);
  fz.inv_n = 1.f / (float)hidden;
  fz.eps = (float)eps;
  fz.cos_sin = cos_sin.data_ptr<float>();
  fz.slot_mapping = slot_mapping.data_ptr<int64_t>();
  HIP_OK(die::launch_attn_decode(bf(out), part_o.data_ptr<float>(), part_ml.data_ptr<float>(),
                                  counters.data_ptr<int>(), nullptr, 0, bf(k_cache), bf(v_cache),
                                  block_tables.data_ptr<int>(), (int)block_tables.size(1), ctx_lens.data_ptr<int>(),
                                  (int)nseq, (int)max_ctx, (int)hq, (int)hkv, (int)D, 16, (float)scale, &fz,
                                  kv_once, cur_stream()));
}

int64_t decode_partials(int64_t max_ctx) { return die::attn_decode_max_partials((int)max_ctx); }

void sample(Tensor out, Tensor logits, c10::optional<Tensor> temperature, c10::optional<Tensor> top_k,
            c10::optional<Tensor> top_p, c10::optional<Tensor> seeds, c10::optional<Tensor> steps,
            c10::optional<Tensor> part, c10::optional<Tensor> cnt, c10::optional<Tensor> lm_part) {
  CHK_CUDA(logits);
  CHK_BF16(logits);
  check_rows(logits, "logits");
  CHK_DTYPE(out, at::kLong);
  const int64_t rows = logits.size(0);
  TORCH_CHECK(out.numel() >= rows, "out too small");
  TORCH_CHECK(logits.size(1) % 8 == 0, "vocab must be a multiple of 8");
  auto opt = [&](const c10::optional<Tensor>& t, at::ScalarType d, const char* n) -> const void* {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->scalar_type() == d && t->is_cuda() && t->numel() >= rows, n, ": wrong dtype/device/size");
    return t->data_ptr();
  };
  // split greedy argmax: a row per `splits` workgroups, so that the grid reaches ~256 workgroups
  int splits = 1;
  uint32_t* pp = nullptr;
  int* cp = nullptr;
  if (part.has_value() && cnt.has_value()) {
    splits = (int)std::max<int64_t>(1, std::min<int64_t>(die::SAMPLE_MAX_SPLITS, 256 / std::max<int64_t>(1, rows)));
    TORCH_CHECK(part->is_cuda() && part->scalar_type() == at::kInt && part->numel() >= rows * splits * 2,
                "sample part scratch [rows * 16 * 2] int32");
    TORCH_CHECK(cnt->is_cuda() && cnt->scalar_type() == at::kInt && cnt->numel() >= rows, "sample cnt [rows] int32");
    pp = reinterpret_cast<uint32_t*>(part->data_ptr<int>());
    cp = cnt->data_ptr<int>();
  }
  // lm_part [>= rows, parts, 2] int32: the LM head's per-column-tile greedy candidates (gemm_decode_argmax)
  const uint32_t* lp = nullptr;
  int lparts = 0;
  if (lm_part.has_value()) {
    TORCH_CHECK(lm_part->is_cuda() && lm_part->scalar_type() == at::kInt && lm_part->dim() == 3 &&
                    lm_part->size(0) >= rows && lm_part->size(2) == 2 && lm_part->is_contiguous(),
                "sample lm_part [rows, parts, 2] int32");
    lp = reinterpret_cast<const uint32_t*>(lm_part->data_ptr<int>());
    lparts = (int)lm_part->size(1);
  }
  HIP_OK(die::launch_sample(out.data_ptr<int64_t>(), bf(logits), logits.stride(0), (int)rows, (int)logits.size(1),
                             (const float*)opt(temperature, at::kFloat, "temperature"),
                             (const int*)opt(top_k, at::kInt, "top_k"), (const float*)opt(top_p, at::kFloat, "top_p"),
                             (const int64_t*)opt(seeds, at::kLong, "seeds"),
                             (const int64_t*)opt(steps, at::kLong, "steps"), cur_stream(), pp, cp, splits,
                             lp, lparts));
}

// Log-probabilities of the raw distribution for targets [rows] int64: lp fp32 / rank int32 [>= rows], and the
// top_n most likely tokens into top_lp fp32 / top_id int32 [>= rows, >= top_n] (same row stride, unit column stride).
void token_logprobs(Tensor lp, Tensor rank, Tensor top_lp, Tensor top_id, Tensor logits, Tensor targets,
                    int64_t top_n) {
  CHK_CUDA(logits);
  CHK_BF16(logits);
  check_rows(logits, "logits");
  const int64_t rows = logits.size(0);
  TORCH_CHECK(targets.is_cuda() && targets.scalar_type() == at::kLong && targets.is_contiguous() &&
                  targets.numel() >= rows, "token_logprobs: targets [rows] int64");
  TORCH_CHECK(lp.is_cuda() && lp.scalar_type() == at::kFloat && lp.is_contiguous() && lp.numel() >= rows &&
                  rank.is_cuda() && rank.scalar_type() == at::kInt && rank.is_contiguous() && rank.numel() >= rows,
              "token_logprobs: lp fp32 [rows], rank int32 [rows]");
  int64_t top_stride = 0;
  if (top_n > 0) {
    TORCH_CHECK(top_lp.is_cuda() && top_lp.scalar_type() == at::kFloat && top_id.is_cuda() &&
                    top_id.scalar_type() == at::kInt && top_lp.dim() == 2 && top_id.dim() == 2 &&
                    top_lp.size(0) >= rows && top_id.size(0) >= rows && top_lp.size(1) >= top_n &&
                    top_id.size(1) >= top_n && top_lp.stride(1) == 1 && top_id.stride(1) == 1 &&
                    top_lp.stride(0) == top_id.stride(0) && top_lp.stride(0) >= top_lp.size(1),
                "token_logprobs: top_lp fp32 / top_id int32 [rows, >= top_n] with the same row stride");
    top_stride = top_lp.stride(0);
  }
  HIP_OK(die::launch_token_logprobs(lp.data_ptr<float>(), rank.data_ptr<int>(),
                                     top_n > 0 ? top_lp.data_ptr<float>() : nullptr,
                                     top_n > 0 ? top_id.data_ptr<int>() : nullptr, top_stride, bf(logits),
                                     logits.stride(0), (int)rows, (int)logits.size(1), targets.data_ptr<int64_t>(),
                                     (int)std::min<int64_t>(std::max<int64_t>(top_n, -1), 1 << 20), cur_stream()));
}

// lm_part int32 [>= rows, parts, 2], optional: the LM-head candidates that logit_process and the guide ops rewrite.
// Returns its pointer (null without one) and the parts; op names the op in the message.
static uint32_t* lm_part_arg(const char* op, int64_t rows, const c10::optional<Tensor>& lm_part, int* lparts) {
  *lparts = 0;
  if (!lm_part.has_value()) return nullptr;
  TORCH_CHECK(lm_part->is_cuda() && lm_part->scalar_type() == at::kInt && lm_part->dim() == 3 &&
                  lm_part->size(0) >= rows && lm_part->size(2) == 2 && lm_part->is_contiguous(),
              op, ": lm_part [rows, parts, 2] int32");
  *lparts = (int)lm_part->size(1);
  return reinterpret_cast<uint32_t*>(lm_part->data_ptr<int>());
}

// Penalties and logit_bias on logits [rows, vocab] in place (logit_process.hip). slot int32 [>= rows]; state int16
// [slots, vocab] (the kernel reads it as uint16); params fp32 [slots, 4]; bias_cnt int32 [slots]; bias_ids int32 /
// bias_vals fp32 [slots, cap]; count_ids int64 [>= rows] and lm_part int32 [>= rows, parts, 2] optional. The
// launcher itself refuses vocab % 8 != 0, cap > 300 and an empty state table.
void logit_process(Tensor logits, Tensor slot, Tensor state, Tensor params, Tensor bias_cnt, Tensor bias_ids,
                   Tensor bias_vals, c10::optional<Tensor> count_ids, c10::optional<Tensor> lm_part) {
  CHK_CUDA(logits);
  CHK_BF16(logits);
  check_rows(logits, "logits");
  const int64_t rows = logits.size(0), vocab = logits.size(1);
  TORCH_CHECK(slot.is_cuda() && slot.scalar_type() == at::kInt && slot.is_contiguous() && slot.numel() >= rows,
              "logit_process: slot int32 [rows]");
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kShort && state.is_contiguous() &&
                  (state.numel() == 0 || (state.dim() == 2 && state.size(1) == vocab)),
              "logit_process: state int16 [slots, vocab]");
  const int64_t slots = state.numel() ? state.size(0) : 0;
  TORCH_CHECK(params.is_cuda() && params.scalar_type() == at::kFloat && params.is_contiguous() &&
                  params.numel() >= 4 * slots && reinterpret_cast<uintptr_t>(params.data_ptr()) % 16 == 0,
              "logit_process: params fp32 [slots, 4]");
  TORCH_CHECK(bias_cnt.is_cuda() && bias_cnt.scalar_type() == at::kInt && bias_cnt.is_contiguous() &&
                  bias_cnt.numel() >= slots, "logit_process: bias_cnt int32 [slots]");
  TORCH_CHECK(bias_ids.is_cuda() && bias_ids.scalar_type() == at::kInt && bias_ids.is_contiguous() &&
                  bias_ids.dim() == 2 && bias_ids.size(0) >= slots && bias_vals.is_cuda() &&
                  bias_vals.scalar_type() == at::kFloat && bias_vals.is_contiguous() && bias_vals.dim() == 2 &&
                  bias_vals.size(0) >= slots && bias_vals.size(1) == bias_ids.size(1),
              "logit_process: bias_ids int32 / bias_vals fp32 [slots, cap]");
  const int64_t* cp = nullptr;
  if (count_ids.has_value()) {
    TORCH_CHECK(count_ids->is_cuda() && count_ids->scalar_type() == at::kLong && count_ids->is_contiguous() &&
                    count_ids->numel() >= rows, "logit_process: count_ids int64 [rows]");
    cp = count_ids->data_ptr<int64_t>();
  }
  int lparts = 0;
  uint32_t* lp = lm_part_arg("logit_process", rows, lm_part, &lparts);
  HIP_OK(die::launch_logit_process(bf(logits), logits.stride(0), (int)rows, (int)vocab, slot.data_ptr<int>(),
                                    (int)slots, slots ? reinterpret_cast<uint16_t*>(state.data_ptr<int16_t>()) : nullptr,
                                    params.data_ptr<float>(), bias_cnt.data_ptr<int>(), bias_ids.data_ptr<int>(),
                                    bias_vals.data_ptr<float>(), (int)bias_ids.size(1), cp, lp, lparts, cur_stream()));
}

// What the four guide ops check alike; op names the op in the messages. The launchers themselves refuse vocab % 8
// != 0, a bad stride, null tables and oversized arenas.
struct GuideArgs {
  int64_t rows, vocab, slots;
  const int64_t* ap;  // advance_ids, or null
  uint32_t* lp;       // lm_part, or null
  int lparts;
};

// logits bf16 [rows, vocab] (16-B aligned); slot int32 [>= rows]; desc int32 [slots, 4]; cur / err int32 [slots];
// advance_ids int64 [>= rows] and lm_part int32 [>= rows, parts, 2] optional
static GuideArgs guide_args(const char* op, const Tensor& logits, const Tensor& slot, const Tensor& desc,
                            const Tensor& cur, const Tensor& err, const c10::optional<Tensor>& advance_ids,
                            const c10::optional<Tensor>& lm_part) {
  CHK_CUDA(logits);
  CHK_BF16(logits);
  check_rows(logits, "logits");
  GuideArgs g{logits.size(0), logits.size(1), 0, nullptr, nullptr, 0};
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0, op, ": logits must be 16-B aligned");
  TORCH_CHECK(slot.is_cuda() && slot.scalar_type() == at::kInt && slot.is_contiguous() && slot.numel() >= g.rows, op,
              ": slot int32 [rows]");
  TORCH_CHECK(desc.is_cuda() && desc.scalar_type() == at::kInt && desc.is_contiguous() && desc.dim() == 2 &&
                  desc.size(1) == 4 && reinterpret_cast<uintptr_t>(desc.data_ptr()) % 16 == 0,
              op, ": desc int32 [slots, 4]");
  g.slots = desc.size(0);
  TORCH_CHECK(cur.is_cuda() && cur.scalar_type() == at::kInt && cur.is_contiguous() && cur.numel() >= g.slots &&
                  err.is_cuda() && err.scalar_type() == at::kInt && err.is_contiguous() && err.numel() >= g.slots,
              op, ": cur / err int32 [slots]");
  if (advance_ids.has_value()) {
    TORCH_CHECK(advance_ids->is_cuda() && advance_ids->scalar_type() == at::kLong && advance_ids->is_contiguous() &&
                    advance_ids->numel() >= g.rows, op, ": advance_ids int64 [rows]");
    g.ap = advance_ids->data_ptr<int64_t>();
  }
  g.lp = lm_part_arg(op, g.rows, lm_part, &g.lparts);
  return g;
}

// the vocabulary's byte table of the byte guides: tok_off int32 [n_tok + 1]; tok_bytes uint8 [B]
static void guide_tok_table(const char* op, const Tensor& tok_off, const Tensor& tok_bytes) {
  TORCH_CHECK(tok_off.is_cuda() && tok_off.scalar_type() == at::kInt && tok_off.is_contiguous() && tok_off.dim() == 1,
              op, ": tok_off int32 [n_tok + 1]");
  TORCH_CHECK(tok_bytes.is_cuda() && tok_bytes.scalar_type() == at::kByte && tok_bytes.is_contiguous() &&
                  tok_bytes.dim() == 1, op, ": tok_bytes uint8 [B]");
}

// Constrained decoding on logits [rows, vocab] in place (token_guide.hip). desc int32 [slots, 4]; rowptr int32 [R];
// edges int32 [E, 2]; the rest as guide_args takes it.
void token_guide(Tensor logits, Tensor slot, Tensor desc, Tensor rowptr, Tensor edges, Tensor cur, Tensor err,
                 c10::optional<Tensor> advance_ids, c10::optional<Tensor> lm_part) {
  const GuideArgs g = guide_args("token_guide", logits, slot, desc, cur, err, advance_ids, lm_part);
  TORCH_CHECK(rowptr.is_cuda() && rowptr.scalar_type() == at::kInt && rowptr.is_contiguous() && rowptr.dim() == 1,
              "token_guide: rowptr int32 [R]");
  TORCH_CHECK(edges.is_cuda() && edges.scalar_type() == at::kInt && edges.is_contiguous() && edges.dim() == 2 &&
                  edges.size(1) == 2 && reinterpret_cast<uintptr_t>(edges.data_ptr()) % 8 == 0,
              "token_guide: edges int32 [E, 2]");
  HIP_OK(die::launch_token_guide(bf(logits), logits.stride(0), (int)g.rows, (int)g.vocab, slot.data_ptr<int>(),
                                  (int)g.slots, desc.data_ptr<int>(), rowptr.data_ptr<int>(), rowptr.numel(),
                                  edges.data_ptr<int>(), edges.size(0), cur.data_ptr<int>(), err.data_ptr<int>(), g.ap,
                                  g.lp, g.lparts, cur_stream()));
}

// Constrained decoding over a multi-byte vocabulary on logits [rows, vocab] in place (byte_guide.hip). desc int32
// [slots, 4] = (state_base, n_states, eos, 0); trans int16 [A, 256]; accept uint8 [A]; tok_off / tok_bytes as
// guide_tok_table takes them; cur / err are token_guide's.
void byte_guide(Tensor logits, Tensor slot, Tensor desc, Tensor trans, Tensor accept, Tensor tok_off, Tensor tok_bytes,
                Tensor cur, Tensor err, c10::optional<Tensor> advance_ids, c10::optional<Tensor> lm_part) {
  const GuideArgs g = guide_args("byte_guide", logits, slot, desc, cur, err, advance_ids, lm_part);
  TORCH_CHECK(trans.is_cuda() && trans.scalar_type() == at::kShort && trans.is_contiguous() && trans.dim() == 2 &&
                  trans.size(1) == 256, "byte_guide: trans int16 [A, 256]");
  TORCH_CHECK(accept.is_cuda() && accept.scalar_type() == at::kByte && accept.is_contiguous() && accept.dim() == 1,
              "byte_guide: accept uint8 [A]");
  guide_tok_table("byte_guide", tok_off, tok_bytes);
  HIP_OK(die::launch_byte_guide(bf(logits), logits.stride(0), (int)g.rows, (int)g.vocab, slot.data_ptr<int>(),
                                 (int)g.slots, desc.data_ptr<int>(), trans.data_ptr<int16_t>(), trans.size(0),
                                 accept.data_ptr<uint8_t>(), accept.numel(), tok_off.data_ptr<int>(),
                                 tok_off.numel() - 1, tok_bytes.data_ptr<uint8_t>(), tok_bytes.numel(),
                                 cur.data_ptr<int>(), err.data_ptr<int>(), g.ap, g.lp, g.lparts, cur_stream()));
}

// JSON mode on logits [rows, vocab] in place (json_guide.hip). desc int32 [slots, 4] = (n_states, done, eos, 0); trans
// int16 [S, 256], the pushdown table; tok_off / tok_bytes: byte_guide's tables; cur / err are token_guide's; jstk
// int32 [slots, 2] = (depth, stack bits).
void json_guide(Tensor logits, Tensor slot, Tensor desc, Tensor trans, Tensor tok_off, Tensor tok_bytes, Tensor cur,
                Tensor jstk, Tensor err, c10::optional<Tensor> advance_ids, c10::optional<Tensor> lm_part) {
  const GuideArgs g = guide_args("json_guide", logits, slot, desc, cur, err, advance_ids, lm_part);
  TORCH_CHECK(trans.is_cuda() && trans.scalar_type() == at::kShort && trans.is_contiguous() && trans.dim() == 2 &&
                  trans.size(1) == 256, "json_guide: trans int16 [S, 256]");
  guide_tok_table("json_guide", tok_off, tok_bytes);
  TORCH_CHECK(jstk.is_cuda() && jstk.scalar_type() == at::kInt && jstk.is_contiguous() && jstk.dim() == 2 &&
                  jstk.size(0) >= g.slots && jstk.size(1) == 2, "json_guide: jstk int32 [slots, 2]");
  HIP_OK(die::launch_json_guide(bf(logits), logits.stride(0), (int)g.rows, (int)g.vocab, slot.data_ptr<int>(),
                                 (int)g.slots, desc.data_ptr<int>(), trans.data_ptr<int16_t>(), trans.size(0),
                                 tok_off.data_ptr<int>(), tok_off.numel() - 1, tok_bytes.data_ptr<uint8_t>(),
                                 tok_bytes.numel(), cur.data_ptr<int>(), jstk.data_ptr<int>(), err.data_ptr<int>(),
                                 g.ap, g.lp, g.lparts, cur_stream()));
}

// Structured outputs on logits [rows, vocab] in place (schema_guide.hip). desc int32 [slots, 4] = (state_base,
// n_states, eos, 0); trans int32 [A, 256] and accept uint8 [A], the pushdown arenas; tok_off / tok_bytes: byte_guide's
// tables; cur / err are token_guide's; sdep int32 [slots] and sstk int16 [slots, 32], the depth and the return states.
void schema_guide(Tensor logits, Tensor slot, Tensor desc, Tensor trans, Tensor accept, Tensor tok_off,
                  Tensor tok_bytes, Tensor cur, Tensor sdep, Tensor sstk, Tensor err,
                  c10::optional<Tensor> advance_ids, c10::optional<Tensor> lm_part) {
  const GuideArgs g = guide_args("schema_guide", logits, slot, desc, cur, err, advance_ids, lm_part);
  TORCH_CHECK(trans.is_cuda() && trans.scalar_type() == at::kInt && trans.is_contiguous() && trans.dim() == 2 &&
                  trans.size(1) == 256, "schema_guide: trans int32 [A, 256]");
  TORCH_CHECK(accept.is_cuda() && accept.scalar_type() == at::kByte && accept.is_contiguous() && accept.dim() == 1,
              "schema_guide: accept uint8 [A]");
  guide_tok_table("schema_guide", tok_off, tok_bytes);
  TORCH_CHECK(sdep.is_cuda() && sdep.scalar_type() == at::kInt && sdep.is_contiguous() && sdep.numel() >= g.slots,
              "schema_guide: sdep int32 [slots]");
  TORCH_CHECK(sstk.is_cuda() && sstk.scalar_type() == at::kShort && sstk.is_contiguous() && sstk.dim() == 2 &&
                  sstk.size(0) >= g.slots && sstk.size(1) == die::GUIDE_SCHEMA_MAX_DEPTH,
              "schema_guide: sstk int16 [slots, 32]");
  HIP_OK(die::launch_schema_guide(bf(logits), logits.stride(0), (int)g.rows, (int)g.vocab, slot.data_ptr<int>(),
                                   (int)g.slots, desc.data_ptr<int>(), trans.data_ptr<int>(), trans.size(0),
                                   accept.data_ptr<uint8_t>(), accept.numel(), tok_off.data_ptr<int>(),
                                   tok_off.numel() - 1, tok_bytes.data_ptr<uint8_t>(), tok_bytes.numel(),
                                   cur.data_ptr<int>(), sdep.data_ptr<int>(), sstk.data_ptr<int16_t>(),
                                   err.data_ptr<int>(), g.ap, g.lp, g.lparts, cur_stream()));
}

// Embedding pooling (pooling.hip): hidden bf16 [T, H] (row stride allowed); segs int32 [S, 8]; acc fp32 [slots, H]
// (optional: only mean pooling reads or writes it); out fp32 [S, H]; part fp32 [P, H] and tickets int32 [>= S]
// (optional, both or neither: the scratch of segments split over max_parts > 1 workgroups). The launcher itself
// refuses H % 8 != 0, a bad stride, bad dims and a bad max_parts.
void pool_embed(Tensor out, c10::optional<Tensor> acc, Tensor hidden, Tensor segs, int64_t dims, bool normalize,
                c10::optional<Tensor> part, c10::optional<Tensor> tickets, int64_t max_parts) {
  CHK_CUDA(hidden);
  CHK_BF16(hidden);
  TORCH_CHECK(hidden.dim() == 2 && hidden.stride(1) == 1, "pool_embed: hidden bf16 [T, H] with contiguous rows");
  const int64_t T = hidden.size(0), H = hidden.size(1);
  TORCH_CHECK(T < (int64_t)1 << 31 && H < (int64_t)1 << 31, "pool_embed: hidden too large");
  TORCH_CHECK(segs.is_cuda() && segs.scalar_type() == at::kInt && segs.is_contiguous() && segs.dim() == 2 &&
                  segs.size(1) == 8, "pool_embed: segs int32 [S, 8]");
  const int64_t S = segs.size(0);
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat && out.is_contiguous() && out.dim() == 2 &&
                  out.size(0) >= S && out.size(1) == H, "pool_embed: out fp32 [S, H]");
  float* ap = nullptr;
  int64_t slots = 0;
  if (acc.has_value()) {
    TORCH_CHECK(acc->is_cuda() && acc->scalar_type() == at::kFloat && acc->is_contiguous() && acc->dim() == 2 &&
                    acc->size(1) == H && acc->size(0) < (int64_t)1 << 31, "pool_embed: acc fp32 [slots, H]");
    ap = acc->data_ptr<float>();
    slots = acc->size(0);
  }
  TORCH_CHECK(part.has_value() == tickets.has_value(), "pool_embed: part and tickets go together");
  float* pp = nullptr;
  int* tp = nullptr;
  int64_t pcap = 0, tcap = 0;
  if (part.has_value()) {
    TORCH_CHECK(part->is_cuda() && part->scalar_type() == at::kFloat && part->is_contiguous() && part->dim() == 2 &&
                    part->size(1) == H && part->size(0) < (int64_t)1 << 31, "pool_embed: part fp32 [P, H]");
    TORCH_CHECK(tickets->is_cuda() && tickets->scalar_type() == at::kInt && tickets->is_contiguous() &&
                    tickets->dim() == 1 && tickets->numel() < (int64_t)1 << 31, "pool_embed: tickets int32 [>= S]");
    pp = part->data_ptr<float>();
    tp = tickets->data_ptr<int>();
    pcap = part->size(0);
    tcap = tickets->numel();
  }
  TORCH_CHECK(dims >= 0 && dims <= H, "pool_embed: dims in [0, H]");
  TORCH_CHECK(max_parts >= 1 && max_parts <= die::POOL_MAX_PARTS, "pool_embed: max_parts in [1, ", die::POOL_MAX_PARTS, "]");
  HIP_OK(die::launch_pool_embed(out.data_ptr<float>(), ap, (int)slots, bf(hidden), hidden.stride(0), (int)T, (int)H,
                                segs.data_ptr<int>(), (int)S, (int)dims, normalize, pp, (int)pcap, tp, (int)tcap,
                                (int)max_parts, cur_stream()));
}

// A decode step's sampling from the LM head's candidates (sample(..., lm_part)) that also advances the step's
// inputs as decode_advance does (ids / pos / ctx / slots / step, the window's token row, the step counter cnt[0]),
// one workgroup per row; ticket: int32 [1], zero, re-armed by the kernel.
void sample_advance(Tensor out, Tensor logits, Tensor temperature, Tensor top_k, Tensor top_p, Tensor seeds,
                    Tensor lm_part, Tensor ids, Tensor pos, Tensor ctx, Tensor slots, Tensor bt, Tensor step,
                    Tensor tokens, Tensor cnt, Tensor n_real, int64_t block_size, Tensor ticket, Tensor table,
                    Tensor h_out, Tensor ssp_out) {
  CHK_CUDA(logits);
  CHK_BF16(logits);
  check_rows(logits, "logits");
  const int64_t rows = logits.size(0);
  for (const Tensor* t : {&out, &ids, &pos, &slots, &step, &tokens, &seeds}) CHK_DTYPE((*t), at::kLong);
  for (const Tensor* t : {&ctx, &bt, &cnt, &n_real, &ticket, &top_k, &lm_part}) CHK_DTYPE((*t), at::kInt);
  CHK_DTYPE(temperature, at::kFloat);
  CHK_DTYPE(top_p, at::kFloat);
  CHK_CONTIG(bt);
  CHK_CONTIG(tokens);
  CHK_CONTIG(lm_part);
  TORCH_CHECK(logits.size(1) % 8 == 0 && lm_part.dim() == 3 && lm_part.size(0) >= rows && lm_part.size(2) == 2,
              "sample_advance: vocab % 8, lm_part [rows, parts, 2]");
  TORCH_CHECK(rows <= out.numel() && rows <= ids.numel() && rows <= pos.numel() && rows <= ctx.numel() &&
                  rows <= slots.numel() && rows <= step.numel() && rows <= seeds.numel() && rows <= temperature.numel() &&
                  rows <= top_k.numel() && rows <= top_p.numel() && bt.dim() == 2 && rows <= bt.size(0) &&
                  tokens.dim() == 2 && rows <= tokens.size(1) && cnt.numel() >= 1 && n_real.numel() >= 1 &&
                  ticket.numel() >= 1,
              "sample_advance: buffers smaller than rows");
  die::SampleAdvance adv;
  adv.ids = ids.data_ptr<int64_t>();
  adv.pos = pos.data_ptr<int64_t>();
  adv.ctx = ctx.data_ptr<int>();
  adv.slots = slots.data_ptr<int64_t>();
  adv.bt = bt.data_ptr<int>();
  adv.bt_width = (int)bt.size(1);
  adv.step = step.data_ptr<int64_t>();
  adv.tokens = tokens.data_ptr<int64_t>();
  adv.tok_stride = (int)tokens.size(1);
  adv.k_max = (int)tokens.size(0);
  adv.cnt = cnt.data_ptr<int>();
  adv.n_real = n_real.data_ptr<int>();
  adv.bs = (int)block_size;
  adv.ticket = ticket.data_ptr<int>();
  if (table.numel()) {  // also the next step's embedding rows + first-norm statistics (as embed_sumsq)
    CHK_BF16(table);
    CHK_BF16(h_out);
    CHK_CONTIG(table);
    CHK_CONTIG(h_out);
    CHK_DTYPE(ssp_out, at::kFloat);
    TORCH_CHECK(table.dim() == 2 && table.size(1) % 8 == 0 && h_out.dim() == 2 && h_out.size(0) >= rows &&
                    h_out.size(1) == table.size(1) && ssp_out.numel() >= rows,
                "sample_advance: table [V, H], h_out [>= rows, H], ssp_out [>= rows]");
    adv.table = bf(table);
    adv.h_out = bf(h_out);
    adv.ssp_out = ssp_out.data_ptr<float>();
    adv.hidden = (int)table.size(1);
  }
  HIP_OK(die::launch_sample(out.data_ptr<int64_t>(), bf(logits), logits.stride(0), (int)rows, (int)logits.size(1),
                             temperature.data_ptr<float>(), top_k.data_ptr<int>(), top_p.data_ptr<float>(),
                             seeds.data_ptr<int64_t>(), step.data_ptr<int64_t>(), cur_stream(), nullptr, nullptr, 1,
                             reinterpret_cast<const uint32_t*>(lm_part.data_ptr<int>()), (int)lm_part.size(1), adv));
}

// pool viewed as [planes, num_blocks, slab]
void copy_blocks(Tensor pool, Tensor pairs) {
  CHK_CUDA(pool);
  CHK_BF16(pool);
  CHK_CONTIG(pool);
  CHK_DTYPE(pairs, at::kLong);
  TORCH_CHECK(pool.dim() >= 3, "pool must be [planes, num_blocks, ...]");
  TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 2, "pairs must be [n, 2]");
  const int64_t planes = pool.size(0), nb = pool.size(1), slab = pool.numel() / (planes * nb);
  HIP_OK(die::launch_copy_blocks(bf(pool), pairs.data_ptr<int64_t>(), (int)pairs.size(0), (int)planes, nb, slab,
                                  cur_stream()));
}

void move_blocks(Tensor pool, Tensor buf, Tensor ids, bool gather) {
  CHK_CUDA(pool);
  CHK_BF16(pool);
  CHK_BF16(buf);
  CHK_CONTIG(pool);
  CHK_CONTIG(buf);
  CHK_DTYPE(ids, at::kLong);
  const int64_t planes = pool.size(0), nb = pool.size(1), slab = pool.numel() / (planes * nb);
  TORCH_CHECK(buf.numel() >= ids.numel() * planes * slab, "staging buffer too small");
  HIP_OK(die::launch_move_blocks(bf(pool), bf(buf), ids.data_ptr<int64_t>(), (int)ids.numel(), (int)planes, nb, slab,
                                  gather, cur_stream()));
}

// pool [planes, blocks, ...]: planes [plane0, plane0 + nplanes) of blocks ids[i] into the packet row at address
// dst[i] (int64 device array; each row holds `planes` slabs). The caller keeps the destinations alive and sized.
void gather_blocks_rows(Tensor pool, Tensor ids, Tensor dst, int64_t plane0, int64_t nplanes) {
  CHK_CUDA(pool);
  CHK_BF16(pool);
  CHK_CONTIG(pool);
  CHK_DTYPE(ids, at::kLong);
  CHK_DTYPE(dst, at::kLong);
  TORCH_CHECK(ids.is_cuda() && dst.is_cuda() && ids.is_contiguous() && dst.is_contiguous() &&
                  ids.numel() == dst.numel(), "ids / dst: int64 device arrays of one length");
  const int64_t planes = pool.size(0), nb = pool.size(1), slab = pool.numel() / (planes * nb);
  TORCH_CHECK(plane0 >= 0 && nplanes >= 0 && plane0 + nplanes <= planes, "plane range outside the pool");
  HIP_OK(die::launch_gather_blocks_rows(bf(pool), ids.data_ptr<int64_t>(), dst.data_ptr<int64_t>(), (int)ids.numel(),
                                         (int)plane0, (int)nplanes, nb, slab, cur_stream()));
}

void topk_softmax(Tensor w, Tensor ids, Tensor gating, bool renorm) {
  CHK_CUDA(gating);
  CHK_BF16(gating);
  CHK_CONTIG(gating);
  CHK_DTYPE(w, at::kFloat);
  CHK_DTYPE(ids, at::kInt);
  TORCH_CHECK(w.sizes() == ids.sizes() && w.size(0) == gating.size(0), "topk_softmax shapes");
  HIP_OK(die::launch_topk_softmax(w.data_ptr<float>(), ids.data_ptr<int>(), bf(gating), (int)gating.size(0),
                                   (int)gating.size(1), (int)w.size(1), renorm, cur_stream()));
}

void moe_align(Tensor offsets, Tensor sorted, Tensor pos, Tensor ids, int64_t num_experts) {
  CHK_DTYPE(offsets, at::kInt);
  CHK_DTYPE(sorted, at::kInt);
  CHK_DTYPE(pos, at::kInt);
  CHK_DTYPE(ids, at::kInt);
  TORCH_CHECK(offsets.numel() >= num_experts + 1 && sorted.numel() >= ids.numel() && pos.numel() >= ids.numel(),
              "moe_align buffers");
  HIP_OK(die::launch_moe_align(offsets.data_ptr<int>(), sorted.data_ptr<int>(), pos.data_ptr<int>(),
                                ids.data_ptr<int>(), (int)ids.numel(), (int)num_experts, cur_stream()));
}

void moe_gather(Tensor xs, Tensor x, Tensor sorted, int64_t topk) {
  CHK_BF16(xs);
  CHK_BF16(x);
  CHK_CONTIG(xs);
  CHK_CONTIG(x);
  CHK_DTYPE(sorted, at::kInt);
  TORCH_CHECK(xs.size(0) == sorted.numel() && xs.size(1) == x.size(1) && sorted.numel() == x.size(0) * topk,
              "moe_gather shapes");
  HIP_OK(die::launch_moe_gather(bf(xs), bf(x), sorted.data_ptr<int>(), (int)xs.size(0), (int)topk, (int)x.size(1),
                                 cur_stream()));
}

void moe_combine(Tensor out, Tensor ys, Tensor pos, Tensor w) {
  CHK_BF16(out);
  CHK_BF16(ys);
  CHK_CONTIG(out);
  CHK_CONTIG(ys);
  CHK_DTYPE(pos, at::kInt);
  CHK_DTYPE(w, at::kFloat);
  const int64_t T = out.size(0), K = w.size(1);
  TORCH_CHECK(w.size(0) == T && pos.numel() == T * K && ys.size(0) == T * K && ys.size(1) == out.size(1),
              "moe_combine shapes");
  HIP_OK(die::launch_moe_combine(bf(out), bf(ys), pos.data_ptr<int>(), w.data_ptr<float>(), (int)T, (int)K,
                                  (int)out.size(1), cur_stream()));
}

// Fused decode routing: w [T, K] fp32, ids [T, K] int32 from x [T, H] (row stride ldx) and the router
// weights wg [E, H] bf16 (moe.hip moe_route_kernel).
void moe_route(Tensor w, Tensor ids, Tensor x, Tensor wg, bool renorm) {
  CHK_CUDA(x);
  CHK_BF16(x);
  CHK_BF16(wg);
  CHK_CONTIG(wg);
  CHK_CONTIG(w);
  CHK_CONTIG(ids);
  CHK_DTYPE(w, at::kFloat);
  CHK_DTYPE(ids, at::kInt);
  check_rows(x, "x");
  TORCH_CHECK(wg.dim() == 2 && wg.size(1) == x.size(1), "moe_route: wg [E, H]");
  TORCH_CHECK(w.dim() == 2 && w.size(0) == x.size(0) && ids.sizes() == w.sizes(), "moe_route: w, ids [T, K]");
  HIP_OK(die::launch_moe_route(w.data_ptr<float>(), ids.data_ptr<int>(), bf(x), x.stride(0), bf(wg),
                                (int)x.size(0), (int)x.size(1), (int)wg.size(0), (int)w.size(1), renorm,
                                cur_stream()));
}

// resid [T, H] += combine(ys, pos, w); ssp [>= T] fp32 = row sums of squares of the new residual.
void moe_combine_residual(Tensor ssp, Tensor resid, Tensor ys, Tensor pos, Tensor w) {
  CHK_CUDA(resid);
  CHK_BF16(resid);
  CHK_BF16(ys);
  CHK_CONTIG(ys);
  CHK_CONTIG(pos);
  CHK_CONTIG(w);
  CHK_CONTIG(ssp);
  CHK_DTYPE(ssp, at::kFloat);
  CHK_DTYPE(pos, at::kInt);
  CHK_DTYPE(w, at::kFloat);
  check_rows(resid, "resid");
  const int64_t T = resid.size(0), H = resid.size(1), K = w.size(1);
  TORCH_CHECK(w.size(0) == T && pos.numel() == T * K && ys.size(0) == T * K && ys.size(1) == H && ssp.numel() >= T,
              "moe_combine_residual shapes");
  HIP_OK(die::launch_moe_combine_residual(ssp.data_ptr<float>(), bf(resid), resid.stride(0), bf(ys),
                                           pos.data_ptr<int>(), w.data_ptr<float>(), (int)T, (int)K, (int)H,
                                           cur_stream()));
}

// Decode GEMM (gemm_decode.hip), x [M <= 128, K] @ w^T. mode 0 bf16 y [M, N]; 1 silu(x gate^T) * (x up^T)
// with w = [gate; up]; 2 fp32 split-K slabs [sk, M, N]; 3 slabs + residual update of `resid` [M, N] and row
// sums of squares `ssp_out` [N/wr, 128] (tickets `counters` [N/wr], zeroed once); 4 = mode 1 with rows
// scaled by the RMSNorm statistics `ssp_in` [T, 128] (eps; the norm weight is folded into w). (wr, kc):
// weight rows and K elements per ring slot of a workgroup. Unused fusion tensors may be empty.
// Diagnostics: when set (non-empty int64 tensor [>= 3 * workgroups]), every decode-GEMM launch writes
// per-workgroup [start, end, xcc] s_memrealtime stamps (100 MHz) there (bench/micro_gd_timeline.py).
static long long* g_gd_ts = nullptr;
// decode-GEMM tiles that are instantiated (gd_tiles.h; gemm_decode.hip launch_gemm_decode dispatches on the same list)
static bool gd_tile_ok(int64_t wr, int64_t kc) {
#define GD_TILE(WR, KC) \
  if (wr == WR && kc == KC) return true;
  GD_TILES(GD_TILE)
#undef GD_TILE
  return false;
}
void gd_set_timestamps(Tensor t) {
  g_gd_ts = t.numel() ? reinterpret_cast<long long*>(t.data_ptr<int64_t>()) : nullptr;
}

void attn_set_few_pair_parts(bool on) { die::attn_set_few_pair_parts(on); }

void attn_set_timestamps(Tensor t) {
  die::attn_set_timestamps(t.numel() ? reinterpret_cast<long long*>(t.data_ptr<int64_t>()) : nullptr);
}

static void gemm_decode_impl(Tensor y, Tensor x, Tensor w, int64_t mode, int64_t wr, int64_t kc, int64_t sk,
                             bool nt, Tensor resid, Tensor ssp_out, Tensor counters, Tensor ssp_in, double eps,
                             die::GemmDecodeFuse fz) {
  CHK_CUDA(x);
  CHK_BF16(x);
  CHK_BF16(w);
  CHK_CONTIG(w);
  check_rows(x, "x");
  const bool tiled = (mode & 32) != 0;  // w pre-packed by ops.gd_pack_weights for this (mode, wr)
  // mode bit 64: the half-LDS ring (mode 3, <= 32 rows), two workgroups resident per CU (GemmDecodeFuse.half_ring)
  fz.half_ring = (mode & 64) != 0 ? 1 : 0;
  // mode bit 128: w in the lossless 13-bit layout (ops.gd_pack_weights_p13), its base7 in mode bits 8..14
  fz.p13 = (mode & 128) != 0 ? 1 : 0;
  fz.p13_base7 = fz.p13 ? (int)((mode >> 8) & 127) : 0;
  TORCH_CHECK(!(fz.p13 && tiled), "gemm_decode: P13 weights are not also TILED");
  mode &= 31;
  const int64_t M = x.size(0), K = x.size(1);
  TORCH_CHECK(M >= 1 && M <= 128, "gemm_decode: 1 <= M <= 128");
  TORCH_CHECK(gd_tile_ok(wr, kc), "gemm_decode: unsupported (wr, kc) tile");
  TORCH_CHECK(mode >= 0 && mode <= 6 && mode != 5, "mode");
  const int64_t wrr = wr;  // rows per workgroup
  TORCH_CHECK(K % kc == 0 && K / kc >= sk, "gemm_decode: K must be a multiple of kc with >= sk K-slots");
  const bool silu = mode == 1 || mode == 4 || mode == 6;
  int64_t N, ldy;
  if (mode == 2 || mode == 3) {
    CHK_DTYPE(y, at::kFloat);
    CHK_CONTIG(y);
    TORCH_CHECK(y.dim() == 3 && y.size(0) == sk && y.size(1) == M, "slab y must be [sk, M, N]");
    N = y.size(2);
    ldy = N;
  } else {
    CHK_BF16(y);
    check_rows(y, "y");
    TORCH_CHECK((sk == 1 || mode == 6) && y.size(0) == M, "bf16 output: sk == 1 (mode 6: any), y [M, N]");
    N = y.size(1);
    ldy = y.stride(0);
  }
  TORCH_CHECK(w.dim() == 2 && w.size(1) == K &&
                  (fz.p13 ? w.size(0) * 16 == (silu ? 2 * N : N) * 13 : w.size(0) == (silu ? 2 * N : N)),
              "gemm_decode w shape");
  TORCH_CHECK(N % (silu ? wrr / 2 : wrr) == 0, "N not a multiple of the column tile");
  TORCH_CHECK((int64_t)sk * M * N * 4 < ((int64_t)1 << 31) || mode != 3, "slab too large");
  fz.ts = g_gd_ts;
  fz.tiled = tiled ? 1 : 0;
  if (mode == 3) {
    TORCH_CHECK(wrr == 32 || wrr == 64 || wrr == 128, "mode 3: wr in {32, 64, 128}");
    CHK_BF16(resid);
    check_rows(resid, "resid");
    TORCH_CHECK(resid.size(0) >= M && resid.size(1) == N, "resid [M, N]");
    CHK_DTYPE(ssp_out, at::kFloat);
    CHK_CONTIG(ssp_out);
    TORCH_CHECK(ssp_out.numel() >= (N / wrr) * die::DECODE_SSP_LD, "ssp_out [N/wr, 128]");
    fz.resid = bf(resid);
    fz.ld_resid = resid.stride(0);
    fz.ssp_out = ssp_out.data_ptr<float>();
    if (sk > 1) {
      CHK_DTYPE(counters, at::kInt);
      TORCH_CHECK(counters.is_cuda() && counters.numel() >= N / wrr, "counters [N/wr] int32");
      fz.counters = counters.data_ptr<int>();
    }
  }
  if (mode == 6 && sk > 1) {  // split-K SiLU: ssp_out carries the fp32 partial slab [sk, M, 2N], counters the tickets
    CHK_DTYPE(ssp_out, at::kFloat);
    CHK_CONTIG(ssp_out);
    TORCH_CHECK(ssp_out.numel() >= sk * M * 2 * N && sk * M * 2 * N * 4 < ((int64_t)1 << 31), "mode 6 slab [sk, M, 2N]");
    CHK_DTYPE(counters, at::kInt);
    TORCH_CHECK(counters.is_cuda() && counters.numel() >= N / (wrr / 2), "mode 6 counters [N / (wr / 2)] int32");
    fz.slab6 = ssp_out.data_ptr<float>();
    fz.ld_slab6 = 2 * N;
    fz.counters = counters.data_ptr<int>();
  }
  if (mode == 4 || mode == 6) {
    CHK_DTYPE(ssp_in, at::kFloat);
    CHK_CONTIG(ssp_in);
    TORCH_CHECK(ssp_in.dim() == 2 && ssp_in.size(1) == die::DECODE_SSP_LD && ssp_in.size(0) >= 1 &&
                    ssp_in.size(0) <= (M <= 32 ? die::DECODE_SSP_MAX_TILES : die::DECODE_SSP_MAX_TILES_WIDE),
                "ssp_in [tiles <= 256 (<= 128 above 32 rows), 128]");
    fz.ssp_in = ssp_in.data_ptr<float>();
    fz.ssp_tiles = (int)ssp_in.size(0);
    fz.inv_n = 1.f / (float)K;
    fz.eps = (float)eps;
  }
  HIP_OK(die::launch_gemm_decode(y.data_ptr(), ldy, bf(x), x.stride(0), bf(w), (int)M, (int)N, (int)K, (int)mode,
                                  (int)wr, (int)kc, (int)sk, nt, fz, cur_stream()));
}

void gemm_decode(Tensor y, Tensor x, Tensor w, int64_t mode, int64_t wr, int64_t kc, int64_t sk, bool nt,
                 Tensor resid, Tensor ssp_out, Tensor counters, Tensor ssp_in, double eps) {
  gemm_decode_impl(y, x, w, mode, wr, kc, sk, nt, resid, ssp_out, counters, ssp_in, eps, die::GemmDecodeFuse{});
}

// Resident workgroups per CU of the decode-GEMM instantiation a launch with these parameters would use (mode word
// as for gemm_decode, bits 32 / 64 included; rows = the step's row count): hipOccupancyMaxActiveBlocksPerMultiprocessor
// on that kernel with its LDS, no launch. -1 if no such instantiation exists. The TP exchange's residency rule
// (CustomAllReduce.fused_ok) is built on it.
int64_t gd_occupancy(int64_t mode, int64_t wr, int64_t kc, int64_t sk, int64_t rows, bool nt) {
  if (!gd_tile_ok(wr, kc) || rows < 1 || rows > 128 || sk < 1) return -1;
  die::GemmDecodeFuse fz;
  fz.half_ring = (mode & 64) != 0 ? 1 : 0;
  fz.p13 = (mode & 128) != 0 ? 1 : 0;
  const int m = (int)(mode & 31);
  // stand-ins for the pointers the launcher validates (never dereferenced: nothing is launched)
  static char dummy[64];
  fz.resid = reinterpret_cast<die::bf16_t*>(dummy);
  fz.ssp_out = reinterpret_cast<float*>(dummy);
  fz.counters = reinterpret_cast<int*>(dummy);
  fz.ssp_in = reinterpret_cast<const float*>(dummy);
  fz.ssp_tiles = 1;
  fz.slab6 = reinterpret_cast<float*>(dummy);
  int occ = 0;
  fz.occupancy = &occ;
  const int silu = (m == 1 || m == 4 || m == 6);
  const int n = (int)(silu ? wr / 2 : wr);  // one column tile: the launcher only checks divisibility
  const int k = (int)(kc * sk);
  const hipError_t e = die::launch_gemm_decode(dummy, n, reinterpret_cast<const die::bf16_t*>(dummy), k,
                                               reinterpret_cast<const die::bf16_t*>(dummy), (int)rows, n, k, m,
                                               (int)wr, (int)kc, (int)sk, nt, fz, cur_stream());
  return e == hipSuccess ? occ : -1;
}

// y = x @ w^T (mode 0, bf16) that also writes each column tile's per-row greedy candidate into amax
// [M, N / wr, 2] int32 (value bits, column): the decode step's LM head, whose argmax then reduces N / wr
// candidates per row (sample(..., lm_part=amax)) instead of re-reading the logits.
// layout: 0 row-major w, 1 tile order (TILED), or a mode word's layout flags (P13 | base7 << 8).
void gemm_decode_argmax(Tensor y, Tensor x, Tensor w, int64_t wr, int64_t kc, int64_t layout, Tensor amax) {
  CHK_DTYPE(amax, at::kInt);
  CHK_CONTIG(amax);
  TORCH_CHECK(amax.is_cuda() && amax.dim() == 3 && amax.size(0) >= x.size(0) && amax.size(2) == 2 &&
                  y.dim() == 2 && amax.size(1) == y.size(1) / wr && y.is_contiguous() && y.size(1) % 8 == 0,
              "gemm_decode_argmax: amax [M, N / wr, 2] int32 with a contiguous y of N % 8 == 0 columns");
  die::GemmDecodeFuse fz;
  fz.amax = reinterpret_cast<uint32_t*>(amax.data_ptr<int>());
  fz.amax_parts = (int)amax.size(1);
  TORCH_CHECK(layout >= 0 && (layout & 31) <= 1, "gemm_decode_argmax: layout");
  gemm_decode_impl(y, x, w, layout == 1 ? 32 : layout, wr, kc, 1, true, x, x, x, x, 0.0, fz);
}

// Tensor-parallel row-parallel projection in ONE launch (decode, mode 3): this rank's K-shard GEMM, the one-shot
// all-reduce of each column tile with the group's peers (the CustomAllReduce's staging buffers, flag pages and
// control words: bufs / sigs / ctl / cap as for car_all_reduce), the residual update and the next norm's per-tile
// statistics. Every rank of the group must make the same call (same shapes, same tile plan).
void gemm_decode_car(Tensor y, Tensor x, Tensor w, int64_t mode, int64_t wr, int64_t kc, int64_t sk, bool nt,
                     Tensor resid, Tensor ssp_out, Tensor counters, int64_t rank, std::vector<int64_t> bufs,
                     std::vector<int64_t> sigs, int64_t ctl, int64_t cap_elems) {
  TORCH_CHECK((mode & 31) == 3, "gemm_decode_car: mode 3 (residual epilogue)");
  const int world = (int)bufs.size();
  TORCH_CHECK(world >= 2 && world <= die::CAR_MAX_RANKS && (int)sigs.size() == world, "2..8 ranks");
  TORCH_CHECK(rank >= 0 && rank < world && ctl != 0, "bad rank / control word");
  TORCH_CHECK(resid.dim() == 2 && x.size(0) * resid.size(1) <= cap_elems, "message larger than the staging half");
  TORCH_CHECK(resid.size(1) / wr <= die::CAR_MAX_BLOCKS, "more column tiles than flag slots");
  die::GemmDecodeFuse fz;
  for (int p = 0; p < world; ++p) {
    TORCH_CHECK(bufs[p] != 0 && sigs[p] != 0, "null peer pointer");
    fz.car.buf[p] = reinterpret_cast<die::bf16_t*>(bufs[p]);
    fz.car.sig[p] = reinterpret_cast<uint32_t*>(sigs[p]);
  }
  fz.car_world = world;
  fz.car_rank = (int)rank;
  fz.car_ctl = reinterpret_cast<uint32_t*>(ctl);
  fz.car_cap = cap_elems;
  fz.car_mode = die::car_mode();
  fz.car_spin = die::car_spin_limit();
  gemm_decode_impl(y, x, w, mode, wr, kc, sk, nt, resid, ssp_out, counters, x, 0.0, fz);
}


// Grouped (MoE) decode GEMM: x [R, K] token-sorted activations (expert e owns rows
// [offsets[e], offsets[e+1]), at most max_rows (<= 128) of them — one decode step), w [E, rows, K] stacked
// expert weights, y [R, N] bf16. mode 1: w[e] = [gate; up] -> silu(gate)*up (N = rows/2);
// mode 0: plain. Experts with no rows stream no weights.
void gemm_decode_grouped(Tensor y, Tensor x, Tensor w, Tensor offsets, int64_t mode, int64_t wr, int64_t kc,
                         Tensor rows, int64_t k, int64_t max_rows, int64_t segs) {
  CHK_CUDA(x);
  CHK_BF16(x);
  CHK_BF16(w);
  CHK_BF16(y);
  CHK_CONTIG(w);
  check_rows(x, "x");
  check_rows(y, "y");
  CHK_DTYPE(offsets, at::kInt);
  TORCH_CHECK(mode == 0 || mode == 1, "grouped: mode 0 or 1");
  TORCH_CHECK(w.dim() == 3 && w.size(2) == x.size(1), "w [E, rows, K]");
  const int64_t E = w.size(0), K = x.size(1);
  // segs > 1: expert e's rows come as segs groups (offsets [E * segs + 1], group g -> expert g / segs), each
  // of at most max_rows rows, for steps whose experts may get more rows than the activation image holds
  TORCH_CHECK(segs >= 1 && offsets.numel() >= E * segs + 1, "offsets [E * segs + 1]");
  const int64_t N = mode == 1 ? w.size(1) / 2 : w.size(1);
  const bool gather = rows.numel() > 0;  // x in token order, row j of the sorted order = rows[j] / k
  if (gather) {
    CHK_DTYPE(rows, at::kInt);
    CHK_CONTIG(rows);
    TORCH_CHECK(k >= 1 && rows.numel() == y.size(0) && x.size(0) * k == y.size(0), "grouped gather: rows [T*k]");
  }
  TORCH_CHECK((gather || y.size(0) == x.size(0)) && y.size(1) == N, "y [R, N]");
  TORCH_CHECK(gd_tile_ok(wr, kc), "grouped: unsupported (wr, kc) tile");
  // max_rows bounds every expert's rows (a token routes to an expert at most once: <= tokens); it picks
  // the activation image (16 / 32 / 64 / 128 rows) and clamps each group to it
  TORCH_CHECK(max_rows >= 1 && max_rows <= 128, "grouped: 1 <= max_rows <= 128");
  TORCH_CHECK(K % kc == 0 && N % (mode == 1 ? wr / 2 : wr) == 0, "tile shape");
  die::GemmDecodeFuse fz;
  fz.grp_off = offsets.data_ptr<int>();
  fz.grp_wstride = w.size(1) * K;
  fz.grp_n = (int)(E * segs);
  fz.grp_div = (int)segs;
  if (gather) {
    fz.grp_rows = rows.data_ptr<int>();
    fz.grp_k = (int)k;
  }
  TORCH_CHECK(y.size(0) >= 1, "grouped: at least one row");
  HIP_OK(die::launch_gemm_decode(y.data_ptr(), y.stride(0), bf(x), x.stride(0), bf(w),
                                  (int)std::min<int64_t>(y.size(0), max_rows), (int)N, (int)K, (int)mode, (int)wr,
                                  (int)kc, 1, true, fz, cur_stream()));
}

// Decode-step input advance (decode_step.hip), for multi-step decode windows.
void decode_advance(Tensor out, Tensor ids, Tensor pos, Tensor ctx, Tensor slots, Tensor bt, Tensor step,
                    Tensor tokens, Tensor cnt, Tensor n_real, int64_t rows, int64_t block_size) {
  CHK_CUDA(out);
  for (const Tensor* t : {&out, &ids, &pos, &slots, &step, &tokens}) CHK_DTYPE((*t), at::kLong);
  for (const Tensor* t : {&ctx, &bt, &cnt, &n_real}) CHK_DTYPE((*t), at::kInt);
  CHK_CONTIG(bt);
  CHK_CONTIG(tokens);
  TORCH_CHECK(rows <= out.numel() && rows <= ids.numel() && rows <= pos.numel() && rows <= ctx.numel() &&
                  rows <= slots.numel() && rows <= step.numel() && rows <= bt.size(0) && rows <= tokens.size(1),
              "decode_advance: buffers smaller than rows");
  TORCH_CHECK(tokens.dim() == 2 && bt.dim() == 2, "tokens [K, S], bt [S, W]");
  HIP_OK(die::launch_decode_advance(out.data_ptr<int64_t>(), ids.data_ptr<int64_t>(), pos.data_ptr<int64_t>(),
                                     ctx.data_ptr<int>(), slots.data_ptr<int64_t>(), bt.data_ptr<int>(),
                                     (int)bt.size(1), step.data_ptr<int64_t>(), tokens.data_ptr<int64_t>(),
                                     (int)tokens.size(1), cnt.data_ptr<int>(), n_real.data_ptr<int>(), (int)rows,
                                     (int)block_size, (int)tokens.size(0), cur_stream()));
}

// Decode-step embedding gather + first-norm statistics (norm_act.hip): out [M, H] = table[ids], ssp[0][m] = sum of
// squares of out[m]
void embed_sumsq(Tensor out, Tensor ssp, Tensor table, Tensor ids) {
  CHK_CUDA(table);
  CHK_BF16(table);
  CHK_BF16(out);
  CHK_CONTIG(table);
  CHK_CONTIG(out);
  CHK_DTYPE(ids, at::kLong);
  CHK_CONTIG(ids);
  CHK_DTYPE(ssp, at::kFloat);
  CHK_CONTIG(ssp);
  const int64_t M = ids.numel(), H = table.size(1);
  TORCH_CHECK(table.dim() == 2 && out.dim() == 2 && out.size(0) == M && out.size(1) == H, "out [M, H], table [V, H]");
  TORCH_CHECK(M >= 1 && M <= die::DECODE_SSP_LD && ssp.numel() >= die::DECODE_SSP_LD && H % 8 == 0,
              "embed_sumsq: 1 <= M <= 128 rows, ssp [1, 128], H % 8 == 0");
  HIP_OK(die::launch_embed_sumsq(bf(out), ssp.data_ptr<float>(), bf(table), ids.data_ptr<int64_t>(), (int)M, (int)H,
                                  cur_stream()));
}

void residual_add_sumsq(Tensor ssp, Tensor resid, Tensor x) {
  CHK_CUDA(x);
  CHK_BF16(x);
  CHK_BF16(resid);
  check_rows(x, "x");
  check_rows(resid, "resid");
  CHK_DTYPE(ssp, at::kFloat);
  CHK_CONTIG(ssp);
  TORCH_CHECK(x.sizes() == resid.sizes() && x.size(0) <= die::DECODE_SSP_LD && ssp.numel() >= x.size(0),
              "residual_add_sumsq shapes");
  HIP_OK(die::launch_residual_add_sumsq(ssp.data_ptr<float>(), bf(resid), bf(x), (int)x.size(0), (int)x.size(1),
                                         resid.stride(0), x.stride(0), cur_stream()));
}

void row_sumsq(Tensor ssp, Tensor x) {
  CHK_CUDA(x);
  CHK_BF16(x);
  check_rows(x, "x");
  CHK_DTYPE(ssp, at::kFloat);
  CHK_CONTIG(ssp);
  TORCH_CHECK(x.size(0) <= die::DECODE_SSP_LD && ssp.numel() >= x.size(0), "row_sumsq: x [<= 128, H], ssp [1, 128]");
  HIP_OK(die::launch_row_sumsq(ssp.data_ptr<float>(), bf(x), (int)x.size(0), (int)x.size(1), x.stride(0),
                                cur_stream()));
}

void fused_add_rms_norm_slab(Tensor out, Tensor slab, Tensor residual, Tensor w, double eps) {
  CHK_CUDA(slab);
  CHK_DTYPE(slab, at::kFloat);
  CHK_CONTIG(slab);
  CHK_BF16(out);
  CHK_BF16(residual);
  CHK_CONTIG(residual);
  check_rows(out, "out");
  TORCH_CHECK(slab.dim() == 3 && slab.size(1) == residual.size(0) && slab.size(2) == residual.size(1),
              "slab [sk, rows, hidden] must match residual");
  TORCH_CHECK(out.size(0) == residual.size(0) && out.size(1) == residual.size(1) && w.numel() == residual.size(1),
              "shapes");
  TORCH_CHECK(residual.size(1) <= 8 * 256 * 8 && residual.size(1) % 8 == 0, "hidden");
  HIP_OK(die::launch_fused_add_rms_norm_slab(bf(out), slab.data_ptr<float>(), (int)slab.size(0), bf(residual), bf(w),
                                              (float)eps, (int)residual.size(0), (int)residual.size(1),
                                              out.stride(0), cur_stream()));
}

void rope_and_cache_slab(Tensor q_out, Tensor slab, Tensor positions, Tensor cos_sin, Tensor slot_mapping,
                         Tensor k_cache, Tensor v_cache, int64_t hq, int64_t hkv, int64_t head_dim) {
  CHK_CUDA(slab);
  CHK_DTYPE(slab, at::kFloat);
  CHK_CONTIG(slab);
  CHK_BF16(q_out);
  CHK_CONTIG(q_out);
  const int64_t T = slab.size(1);
  TORCH_CHECK(slab.dim() == 3 && slab.size(2) == (hq + 2 * hkv) * head_dim, "slab [sk, T, (hq+2hkv)*D]");
  TORCH_CHECK(q_out.numel() >= T * hq * head_dim, "q_out too small");
  check_rope_index(positions, slot_mapping, cos_sin, slab, T, head_dim);
  check_cache(k_cache, hkv, head_dim, "k_cache");
  check_cache(v_cache, hkv, head_dim, "v_cache");
  HIP_OK(die::launch_rope_and_cache_slab(bf(q_out), slab.data_ptr<float>(), (int)slab.size(0),
                                          positions.data_ptr<int64_t>(), cos_sin.data_ptr<float>(),
                                          slot_mapping.data_ptr<int64_t>(), bf(k_cache), bf(v_cache), (int)T,
                                          (int)hq, (int)hkv, (int)head_dim, (int)k_cache.size(2), cur_stream()));
}

// ---- one-shot all-reduce over IPC-mapped peer buffers (src/parallel/custom_allreduce.py)
int64_t car_alloc(int64_t bytes, bool uncached) {
  TORCH_CHECK(bytes > 0 && bytes % 256 == 0, "car_alloc: bytes must be a positive multiple of 256");
  void* p = nullptr;
  HIP_OK(die::car_malloc(&p, (size_t)bytes, uncached));
  return reinterpret_cast<int64_t>(p);
}

// dst_ptr (raw device pointer, e.g. an IPC-mapped peer buffer) <- src (contiguous GPU tensor), by a
// copy kernel on the current stream
void car_copy_to(int64_t dst_ptr, Tensor src) {
  CHK_CUDA(src);
  CHK_CONTIG(src);
  const int64_t nbytes = src.numel() * src.element_size();
  TORCH_CHECK(dst_ptr != 0 && nbytes % 16 == 0, "car_copy_to: null destination or size not a multiple of 16");
  HIP_OK(die::launch_ipc_copy(reinterpret_cast<void*>(dst_ptr), src.data_ptr(), nbytes, cur_stream()));
}

// A byte tensor over raw device memory we own or mapped (IPC landing zones); no deleter: the owner
// frees it with car_release / car_close after the last view is gone.
Tensor car_tensor(int64_t ptr, int64_t nbytes, int64_t device) {
  TORCH_CHECK(ptr != 0 && nbytes > 0, "car_tensor: null pointer or empty");
  return torch::from_blob(reinterpret_cast<void*>(ptr), {nbytes},
                          torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA, (int)device));
}

void car_release(int64_t ptr) { HIP_OK(die::car_free(reinterpret_cast<void*>(ptr))); }

py::bytes car_handle(int64_t ptr) {
  char h[sizeof(hipIpcMemHandle_t)];
  HIP_OK(die::car_ipc_handle(reinterpret_cast<void*>(ptr), h));
  return py::bytes(h, sizeof(h));
}

int64_t car_open(py::bytes handle) {
  std::string s = handle;
  TORCH_CHECK(s.size() == sizeof(hipIpcMemHandle_t), "bad IPC handle size");
  void* p = nullptr;
  const hipError_t e = die::car_ipc_open(s.data(), &p);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // do not leave the error behind for the next (unrelated) HIP call
    TORCH_CHECK(false, "hipIpcOpenMemHandle failed: ", hipGetErrorString(e));
  }
  return reinterpret_cast<int64_t>(p);
}

void car_close(int64_t ptr) { HIP_OK(die::car_ipc_close(reinterpret_cast<void*>(ptr))); }

void car_all_reduce_residual(Tensor x, Tensor resid, Tensor ssp, int64_t rank, std::vector<int64_t> bufs,
                             std::vector<int64_t> sigs, int64_t ctl, int64_t cap_elems) {
  CHK_CUDA(x);
  CHK_BF16(x);
  CHK_BF16(resid);
  CHK_CONTIG(x);
  CHK_CONTIG(resid);
  CHK_DTYPE(ssp, at::kFloat);
  CHK_CONTIG(ssp);
  TORCH_CHECK(x.dim() == 2 && resid.sizes() == x.sizes(), "x and resid must both be [rows, hidden]");
  const int64_t rows = x.size(0), hidden = x.size(1);
  TORCH_CHECK(hidden % 8 == 0 && rows <= die::CAR_MAX_BLOCKS && rows * hidden <= cap_elems,
              "all_reduce_residual: hidden % 8, rows <= 256 (one flag slot per row), size <= cap");
  TORCH_CHECK(ssp.numel() >= rows, "ssp too small");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(resid.data_ptr()) % 16 == 0, "16-byte alignment");
  const int world = (int)bufs.size();
  TORCH_CHECK(world >= 2 && world <= die::CAR_MAX_RANKS && (int)sigs.size() == world, "2..8 ranks");
  TORCH_CHECK(rank >= 0 && rank < world && ctl != 0, "bad rank / control word");
  die::CarPeers peers;
  for (int p = 0; p < world; ++p) {
    TORCH_CHECK(bufs[p] != 0 && sigs[p] != 0, "null peer pointer");
    peers.buf[p] = reinterpret_cast<die::bf16_t*>(bufs[p]);
    peers.sig[p] = reinterpret_cast<uint32_t*>(sigs[p]);
  }
  HIP_OK(die::launch_custom_all_reduce_residual(bf(x), bf(resid), ssp.data_ptr<float>(), (int)rows, (int)hidden,
                                                 (int)rank, world, peers, reinterpret_cast<uint32_t*>(ctl), cap_elems,
                                                 cur_stream()));
}

std::vector<int64_t> car_read_words(int64_t ptr, int64_t n) {  // synchronising host read of uint32 words
  TORCH_CHECK(n > 0 && n <= 64, "car_read_words: 1..64 words");
  std::vector<uint32_t> h((size_t)n);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(h.data(), reinterpret_cast<void*>(ptr), (size_t)n * 4, hipMemcpyDeviceToHost));
  return std::vector<int64_t>(h.begin(), h.end());
}

static die::CarPeers car_peers(const std::vector<int64_t>& bufs, const std::vector<int64_t>& sigs) {
  const int world = (int)bufs.size();
  TORCH_CHECK(world >= 2 && world <= die::CAR_MAX_RANKS && (int)sigs.size() == world, "2..8 ranks");
  die::CarPeers peers;
  for (int p = 0; p < world; ++p) {
    TORCH_CHECK(bufs[p] != 0 && sigs[p] != 0, "null peer pointer");
    peers.buf[p] = reinterpret_cast<die::bf16_t*>(bufs[p]);
    peers.sig[p] = reinterpret_cast<uint32_t*>(sigs[p]);
  }
  return peers;
}

// out [rows, world * cols] = concatenation of every rank's in [rows, cols] along the last dim
void car_all_gather(Tensor in, Tensor out, int64_t rank, std::vector<int64_t> bufs, std::vector<int64_t> sigs,
                    int64_t ctl, int64_t cap_elems, int64_t blocks) {
  CHK_CUDA(in);
  CHK_BF16(in);
  CHK_BF16(out);
  CHK_CONTIG(in);
  CHK_CONTIG(out);
  const int world = (int)bufs.size();
  TORCH_CHECK(in.dim() == 2 && out.dim() == 2 && out.size(0) == in.size(0) && out.size(1) == world * in.size(1),
              "all_gather: in [rows, cols], out [rows, world * cols]");
  TORCH_CHECK(in.size(1) % 8 == 0 && in.numel() <= cap_elems, "all_gather: cols % 8, numel <= cap");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(in.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0, "all_gather: 16-byte alignment");
  TORCH_CHECK(rank >= 0 && rank < world && ctl != 0, "all_gather: bad rank / control word");
  HIP_OK(die::launch_custom_all_gather(bf(in), bf(out), in.size(0), in.size(1), (int)rank, world,
                                        car_peers(bufs, sigs), reinterpret_cast<uint32_t*>(ctl), cap_elems,
                                        (int)blocks, cur_stream()));
}

void car_all_reduce(Tensor in, Tensor out, int64_t rank, std::vector<int64_t> bufs, std::vector<int64_t> sigs,
                    int64_t ctl, int64_t cap_elems, int64_t blocks) {
  CHK_CUDA(in);
  CHK_BF16(in);
  CHK_BF16(out);
  CHK_CONTIG(in);
  CHK_CONTIG(out);
  TORCH_CHECK(in.numel() == out.numel(), "all_reduce: in/out sizes differ");
  TORCH_CHECK(in.numel() % 8 == 0 && in.numel() <= cap_elems, "all_reduce: numel must be a multiple of 8 <= cap");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(in.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0, "all_reduce: 16-byte alignment");
  const int world = (int)bufs.size();
  TORCH_CHECK(world >= 2 && world <= die::CAR_MAX_RANKS && (int)sigs.size() == world, "all_reduce: 2..8 ranks");
  TORCH_CHECK(rank >= 0 && rank < world && ctl != 0, "all_reduce: bad rank / control word");
  die::CarPeers peers;
  for (int p = 0; p < world; ++p) {
    TORCH_CHECK(bufs[p] != 0 && sigs[p] != 0, "all_reduce: null peer pointer");
    peers.buf[p] = reinterpret_cast<die::bf16_t*>(bufs[p]);
    peers.sig[p] = reinterpret_cast<uint32_t*>(sigs[p]);
  }
  HIP_OK(die::launch_custom_all_reduce(bf(in), bf(out), in.numel(), (int)rank, world, peers,
                                        reinterpret_cast<uint32_t*>(ctl), cap_elems, (int)blocks, cur_stream()));
}

}  // namespace


PYBIND11_MODULE(_C, m) {
  m.doc() = "Hand-written gfx950 (MI355X) HIP kernels";
  m.def("rms_norm", &rms_norm);
  m.def("fused_add_rms_norm", &fused_add_rms_norm);
  m.def("silu_and_mul", &silu_and_mul);
  m.def("silu_and_mul_views", &silu_and_mul_views);
  m.def("rope_and_cache", &rope_and_cache);
  m.def("attn_prefill", &attn_prefill);
  m.def("attn_decode", &attn_decode);
  m.def("attn_decode_fused", &attn_decode_fused);
  m.def("decode_partials", &decode_partials);
  m.def("sample", &sample, py::arg("out"), py::arg("logits"), py::arg("temperature") = py::none(),
        py::arg("top_k") = py::none(), py::arg("top_p") = py::none(), py::arg("seeds") = py::none(),
        py::arg("steps") = py::none(), py::arg("part") = py::none(), py::arg("cnt") = py::none(),
        py::arg("lm_part") = py::none());
  m.def("copy_blocks", &copy_blocks);
  m.def("token_logprobs", &token_logprobs);
  m.def("logit_process", &logit_process);
  m.def("token_guide", &token_guide);
  m.def("byte_guide", &byte_guide);
  m.def("json_guide", &json_guide);
  m.def("schema_guide", &schema_guide);
  m.def("pool_embed", &pool_embed);
  m.def("sample_advance", &sample_advance);
  m.def("move_blocks", &move_blocks);
  m.def("gather_blocks_rows", &gather_blocks_rows);
  m.def("topk_softmax", &topk_softmax);
  m.def("moe_align", &moe_align);
  m.def("moe_gather", &moe_gather);
  m.def("moe_combine", &moe_combine);
  m.def("gemm_decode", &gemm_decode);
  m.def("gemm_decode_argmax", &gemm_decode_argmax);
  m.def("gemm_decode_car", &gemm_decode_car);
  m.def("gd_occupancy", &gd_occupancy);
  m.def("rms_row_scale", &rms_row_scale);
  m.def("gd_set_timestamps", &gd_set_timestamps);
  m.def("attn_set_timestamps", &attn_set_timestamps);
  m.def("attn_set_few_pair_parts", &attn_set_few_pair_parts);
  m.def("row_sumsq", &row_sumsq);
  m.def("residual_add_sumsq", &residual_add_sumsq);
  m.def("decode_advance", &decode_advance);
  m.def("embed_sumsq", &embed_sumsq);
  m.def("moe_route", &moe_route);
  m.def("moe_combine_residual", &moe_combine_residual);
  m.def("gemm_decode_grouped", &gemm_decode_grouped);
  m.def("fused_add_rms_norm_slab", &fused_add_rms_norm_slab);
  m.def("rope_and_cache_slab", &rope_and_cache_slab);
  m.def("car_alloc", &car_alloc, py::arg("bytes"), py::arg("uncached") = true);
  m.def("car_tensor", &car_tensor);
  m.def("car_copy_to", &car_copy_to);
  m.def("car_release", &car_release);
  m.def("car_handle", &car_handle);
  m.def("car_open", &car_open);
  m.def("car_close", &car_close);
  m.def("car_all_reduce", &car_all_reduce);
  m.def("car_all_gather", &car_all_gather);
  m.def("car_read_words", &car_read_words);
  m.def("car_all_reduce_residual", &car_all_reduce_residual);
}
