// Torch bindings of the gfx950 kernels (module `src._C`). Each entry point validates device/dtype/shape up front
// and throws on mismatch — a wrong shape never reaches a kernel (a faulting kernel can take down every GPU on the
// host) — then launches on the current HIP stream (graph-capture safe).
//
// The rule: no pointer without a helper. Every tensor goes through the check vocabulary of arg_check.h (Op::dense,
// Op::rows, their optional forms), which returns the typed pointer; this file never asks a tensor for its address
// itself. The raw-address arguments of the car_* ops arrive as integers and are the one exception.
#include <cstdlib>

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "arg_check.h"
#include "kernels/gd_tiles.h"
#include "kernels/launchers.h"

using torch::Tensor;
using chk::ANY;
using chk::ge;
using chk::Op;
using chk::present;
using die::bf16_t;
using chk::u16_of_i16;

namespace {

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_only(bool on) { chk::g_check_only = on; }

constexpr int64_t MAX_HIDDEN = 8 * 256 * 8;  // the norm kernels: 256 lanes of up to 8 16-byte groups

void rms_norm(Tensor out, Tensor x, Tensor w, double eps) {
  const Op a("rms_norm", x, "x");
  const auto xr = a.rows(x, "x");
  const int T = a.i32(x.size(0)), H = a.i32(x.size(1));
  const auto o = a.rows(out, "out", T, H);
  const bf16_t* wp = a.dense<bf16_t>(w, "w", H);
  TORCH_CHECK(w.numel() == H && H <= MAX_HIDDEN, "rms_norm: w [hidden], hidden <= 16384");
  LAUNCH(launch_rms_norm(o.p, xr.p, wp, (float)eps, T, H, xr.ld, o.ld, cur_stream()));
}

void fused_add_rms_norm(Tensor out, Tensor x, Tensor residual, Tensor w, double eps) {
  const Op a("fused_add_rms_norm", x, "x");
  const auto xr = a.rows(x, "x");
  const int T = a.i32(x.size(0)), H = a.i32(x.size(1));
  const auto o = a.rows(out, "out", T, H);
  bf16_t* rp = a.dense<bf16_t>(residual, "residual", 0, {T, H});
  const bf16_t* wp = a.dense<bf16_t>(w, "w", H);
  TORCH_CHECK(w.numel() == H && H <= MAX_HIDDEN, "fused_add_rms_norm: w [hidden], hidden <= 16384");
  LAUNCH(launch_fused_add_rms_norm(o.p, xr.p, rp, wp, (float)eps, T, H, xr.ld, o.ld, cur_stream()));
}

// row_scale (optional, numel 0 = absent): fp32 [T] RMSNorm row scale applied to gate and up (prefill with the
// norm weight folded into Wgate_up)
void silu_and_mul(Tensor out, Tensor x, Tensor row_scale) {
  const Op a("silu_and_mul", x, "x");
  const bf16_t* xp = a.dense<bf16_t>(x, "x", 0, {ANY, ANY});
  const int T = a.i32(x.size(0)), I = a.i32(x.size(1) / 2);
  bf16_t* op = a.dense<bf16_t>(out, "out", 0, {T, I});
  TORCH_CHECK(x.size(1) == 2 * I && I % 8 == 0, "silu_and_mul: x [T, 2I], out [T, I], I a multiple of 8");
  const float* rs = a.dense_opt<float>(row_scale, "row_scale", T);
  LAUNCH(launch_silu_and_mul(op, xp, T, I, cur_stream(), rs));
}

// silu(gate) * up on [T, I] row views (unit column stride, 16-byte aligned rows; gate and up share a row stride).
void silu_and_mul_views(Tensor out, Tensor gate, Tensor up, Tensor row_scale, int64_t per) {
  const Op a("silu_and_mul_views", gate, "gate");
  const auto g = a.rows(gate, "gate");
  const int T = a.i32(gate.size(0)), I = a.i32(gate.size(1));
  const auto u = a.rows(up, "up", T, I);
  const auto o = a.rows(out, "out", T, I);
  TORCH_CHECK(u.ld == g.ld && I % 8 == 0, "silu_and_mul_views: one row stride for gate and up, I a multiple of 8");
  const float* rs = a.dense_opt<float>(row_scale, "row_scale", T);
  LAUNCH(launch_silu_and_mul_views(o.p, o.ld, g.p, u.p, g.ld, T, I, cur_stream(), rs, a.i32(per)));
}

// Prefill RMSNorm as a row scale: resid += x (x empty: no add) and rs [T] = rsqrt(mean(resid^2) + eps).
void rms_row_scale(Tensor rs, Tensor resid, Tensor x, double eps) {
  const Op a("rms_row_scale", resid, "resid");
  const auto r = a.rows(resid, "resid");
  const int T = a.i32(resid.size(0)), H = a.i32(resid.size(1));
  float* rsp = a.dense<float>(rs, "rs", T);
  const auto xr = a.rows_opt(x, "x", T, H);
  TORCH_CHECK(H <= 8192, "rms_row_scale: hidden <= 8192");
  LAUNCH(launch_rms_row_scale(rsp, r.p, xr.p, T, H, r.ld, xr.ld, (float)eps, cur_stream()));
}

bf16_t* check_cache(const Op& a, const Tensor& c, int64_t hkv, int64_t head_dim, const char* name) {
  return a.dense<bf16_t>(c, name, 0, {ANY, hkv, ANY, head_dim});  // [num_blocks, num_kv_heads, block_size, head_dim]
}

// positions, slot_mapping and cos_sin reach the RoPE kernels as raw pointers: dense arrays on the rows' device
struct RopeIndex {
  const int64_t *pos, *slots;
  const float* cos_sin;
};
RopeIndex check_rope_index(const Op& a, const Tensor& positions, const Tensor& slot_mapping, const Tensor& cos_sin,
                           int64_t tokens, int64_t head_dim) {
  return {a.dense<int64_t>(positions, "positions", tokens), a.dense<int64_t>(slot_mapping, "slot_mapping", tokens),
          a.dense<float>(cos_sin, "cos_sin", 0, {ANY, head_dim})};
}

void rope_and_cache(Tensor qkv, Tensor positions, Tensor cos_sin, Tensor slot_mapping, Tensor k_cache,
                    Tensor v_cache, int64_t hq, int64_t hkv, int64_t head_dim, bool rot_q, Tensor row_scale) {
  const Op a("rope_and_cache", qkv, "qkv");
  const auto q = a.rows(qkv, "qkv");
  const int T = a.i32(qkv.size(0));
  TORCH_CHECK(qkv.size(1) >= (hq + 2 * hkv) * head_dim, "rope_and_cache: qkv width < (hq + 2*hkv) * head_dim");
  const RopeIndex ix = check_rope_index(a, positions, slot_mapping, cos_sin, T, head_dim);
  bf16_t* kc = check_cache(a, k_cache, hkv, head_dim, "k_cache");
  bf16_t* vc = check_cache(a, v_cache, hkv, head_dim, "v_cache");
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes(), "rope_and_cache: k/v cache shapes differ");
  const float* rs = a.dense_opt<float>(row_scale, "row_scale", T);
  const int bs = a.i32(k_cache.size(2));
  LAUNCH(launch_rope_and_cache(q.p, q.ld, ix.pos, ix.cos_sin, ix.slots, kc, vc, T, a.i32(hq), a.i32(hkv),
                               a.i32(head_dim), bs, cur_stream(), rot_q, rs));
}

constexpr int64_t HEAD_DIM = 128;  // the attention kernels' head size

void attn_prefill(Tensor out, Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor cu_q,
                  Tensor ctx_lens, int64_t max_q_len, int64_t hq, int64_t hkv, double scale, Tensor cos_sin,
                  Tensor q_scale) {
  const Op a("attn_prefill", q, "q");
  const int64_t D = HEAD_DIM;
  const auto qr = a.rows(q, "q");
  const int64_t T = q.size(0);
  TORCH_CHECK(q.size(1) >= hq * D, "attn_prefill: q width < hq*128 (head_dim must be 128)");
  bf16_t* op = a.dense<bf16_t>(out, "out", T * hq * D);
  TORCH_CHECK(hkv >= 1 && hq % hkv == 0 && (hq / hkv) <= 32 && (32 % (hq / hkv)) == 0,
              "attn_prefill: hq/hkv must divide 32");
  const bf16_t* kc = check_cache(a, k_cache, hkv, D, "k_cache");
  const bf16_t* vc = check_cache(a, v_cache, hkv, D, "v_cache");
  const int* ctx = a.dense<int>(ctx_lens, "ctx_lens", 0);
  const int nseq = a.i32(ctx_lens.numel());
  const int* cu = a.dense<int>(cu_q, "cu_q", nseq + 1);
  const int* bt = a.dense<int>(block_tables, "block_tables", 0, {ge(nseq), ANY});
  // cos_sin (optional, numel 0 = absent): [max_pos, 128] fp32; Q rows are rotated on load (unrotated q)
  const float* cs = a.dense_opt<float>(cos_sin, "cos_sin", 0, {ANY, D});
  const int n_pos = cs ? a.i32(cos_sin.size(0)) : 0;
  const float* qs = a.dense_opt<float>(q_scale, "q_scale", T);
  const int btw = a.i32(block_tables.size(1)), bs = a.i32(k_cache.size(2));
  LAUNCH(launch_attn_prefill(op, qr.p, qr.ld, kc, vc, bt, btw, cu, ctx, nseq, a.i32(max_q_len), a.i32(hq),
                             a.i32(hkv), (int)D, bs, (float)scale, cur_stream(), cs, n_pos, qs));
}

// What the two decode-attention entries check alike: the paged KV (block table, ctx_lens, caches), the split
// partials part_o / part_ml against attn_decode_max_partials(max_ctx) and the tickets. counters: int32
// [>= num_seqs * hkv], zero before first use (the kernel re-arms them); empty = absent.
struct PagedKv {
  bf16_t *k, *v;
  const int *bt, *ctx;
  int bt_stride, nseq, bs, max_ctx;
  float *part_o, *part_ml;
  int* counters;
};
PagedKv paged_kv(const Op& a, const Tensor& k_cache, const Tensor& v_cache, const Tensor& block_tables,
                 const Tensor& ctx_lens, const Tensor& part_o, const Tensor& part_ml, const Tensor& counters,
                 int64_t max_ctx, int64_t hq, int64_t hkv) {
  const int64_t D = HEAD_DIM;
  PagedKv kv;
  kv.ctx = a.dense<int>(ctx_lens, "ctx_lens", 0);
  kv.nseq = a.i32(ctx_lens.numel());
  kv.k = check_cache(a, k_cache, hkv, D, "k_cache");
  kv.v = check_cache(a, v_cache, hkv, D, "v_cache");
  kv.bs = a.i32(k_cache.size(2));
  kv.bt = a.dense<int>(block_tables, "block_tables", 0, {ge(kv.nseq), ANY});
  kv.bt_stride = a.i32(block_tables.size(1));
  kv.max_ctx = a.i32(max_ctx);
  TORCH_CHECK(block_tables.size(1) * kv.bs >= max_ctx, a.op, ": block table narrower than max_ctx");
  const int64_t maxp = die::attn_decode_max_partials(kv.max_ctx);
  kv.part_o = a.dense<float>(part_o, "part_o", kv.nseq * hq * maxp * D);
  kv.part_ml = a.dense<float>(part_ml, "part_ml", kv.nseq * hq * maxp * 2);
  kv.counters = a.dense_opt<int>(counters, "counters", kv.nseq * hkv);
  return kv;
}

// An empty counters tensor selects the two-kernel path (partials + merge launch).
void attn_decode(Tensor out, Tensor part_o, Tensor part_ml, Tensor counters, Tensor q, Tensor k_cache, Tensor v_cache,
                 Tensor block_tables, Tensor ctx_lens, int64_t max_ctx, int64_t hq, int64_t hkv, double scale,
                 bool kv_once) {
  const Op a("attn_decode", q, "q");
  const int64_t D = HEAD_DIM;
  TORCH_CHECK(hkv >= 1 && hq % hkv == 0 && (hq / hkv) <= 32, "attn_decode: hq/hkv <= 32");
  const PagedKv kv = paged_kv(a, k_cache, v_cache, block_tables, ctx_lens, part_o, part_ml, counters, max_ctx, hq, hkv);
  const auto qr = a.rows(q, "q", ge(kv.nseq), ge(hq * D));
  bf16_t* op = a.dense<bf16_t>(out, "out", kv.nseq * hq * D);
  LAUNCH(launch_attn_decode(op, kv.part_o, kv.part_ml, kv.counters, qr.p, qr.ld, kv.k, kv.v, kv.bt, kv.bt_stride,
                            kv.ctx, kv.nseq, kv.max_ctx, a.i32(hq), a.i32(hkv), (int)D, kv.bs, (float)scale, nullptr,
                            kv_once, cur_stream()));
}

// Decode attention with the fused prologue: q / new K,V built from the qkv projection's
// fp32 split-K slabs [sk, M, (hq+2hkv)*128] (RMSNorm row scale from ssp [T, 32], RoPE from
// cos_sin [max_pos, 128] at positions [M]); the new K/V go to the paged cache at slot_mapping.
void attn_decode_fused(Tensor out, Tensor part_o, Tensor part_ml, Tensor counters, Tensor slab, Tensor ssp,
                       Tensor positions, Tensor cos_sin, Tensor slot_mapping, Tensor k_cache, Tensor v_cache,
                       Tensor block_tables, Tensor ctx_lens, int64_t max_ctx, int64_t hq, int64_t hkv, double scale,
                       double eps, int64_t hidden, bool kv_once) {
  const Op a("attn_decode_fused", slab, "slab");
  const int64_t D = HEAD_DIM;
  TORCH_CHECK(hkv >= 1 && hq % hkv == 0, "attn_decode_fused: hq % hkv");
  const int64_t G = hq / hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8, "fused decode attention: G in {1, 2, 4, 8}");
  const PagedKv kv = paged_kv(a, k_cache, v_cache, block_tables, ctx_lens, part_o, part_ml, counters, max_ctx, hq, hkv);
  TORCH_CHECK(kv.bs == 16, "fused decode attention: block_size 16");
  TORCH_CHECK(kv.counters != nullptr || kv.nseq == 0, "attn_decode_fused: counters int32 [>= num_seqs*hkv]");
  die::AttnDecodeFuse fz;
  fz.slab = a.dense<float>(slab, "slab", 0, {ANY, ge(kv.nseq), (hq + 2 * hkv) * D});
  fz.sk = a.i32(slab.size(0));
  fz.slab_stride = slab.size(1) * slab.size(2);
  fz.width = a.i32(slab.size(2));
  bf16_t* op = a.dense<bf16_t>(out, "out", kv.nseq * hq * D);
  fz.ssp = a.dense<float>(ssp, "ssp", 0, {ANY, die::DECODE_SSP_LD});
  TORCH_CHECK(ssp.size(0) >= 1 && ssp.size(0) <= die::DECODE_SSP_MAX_TILES, "attn_decode_fused: ssp [tiles <= 256, 128]");
  fz.ssp_tiles = a.i32(ssp.size(0));
  fz.inv_n = 1.f / (float)hidden;
  fz.eps = (float)eps;
  // decode: every sequence's new token sits at position ctx_len - 1 (the kernel uses that, not positions)
  const RopeIndex ix = check_rope_index(a, positions, slot_mapping, cos_sin, kv.nseq, D);
  fz.cos_sin = ix.cos_sin;
  fz.slot_mapping = ix.slots;
  LAUNCH(launch_attn_decode(op, kv.part_o, kv.part_ml, kv.counters, nullptr, 0, kv.k, kv.v, kv.bt, kv.bt_stride,
                            kv.ctx, kv.nseq, kv.max_ctx, a.i32(hq), a.i32(hkv), (int)D, 16, (float)scale, &fz, kv_once,
                            cur_stream()));
}

int64_t decode_partials(int64_t max_ctx) { return die::attn_decode_max_partials((int)max_ctx); }

// lm_part int32 [>= rows, parts, 2], optional (null = absent): the LM head's per-column-tile greedy candidates
// (gemm_decode_argmax) that sampling reduces and that logit_process and the guide ops rewrite. Returns its pointer
// (null without one) and the parts.
uint32_t* lm_part_arg(const Op& a, int64_t rows, const Tensor* lm_part, int* lparts) {
  *lparts = 0;
  if (lm_part == nullptr) return nullptr;
  uint32_t* p = a.dense<uint32_t>(*lm_part, "lm_part", 0, {ge(rows), ANY, 2});
  *lparts = a.i32(lm_part->size(1));
  return p;
}

void sample(Tensor out, Tensor logits, c10::optional<Tensor> temperature, c10::optional<Tensor> top_k,
            c10::optional<Tensor> top_p, c10::optional<Tensor> seeds, c10::optional<Tensor> steps,
            c10::optional<Tensor> part, c10::optional<Tensor> cnt, c10::optional<Tensor> lm_part) {
  const Op a("sample", logits, "logits");
  const auto lg = a.rows(logits, "logits");
  const int rows = a.i32(logits.size(0)), vocab = a.i32(logits.size(1));
  int64_t* op = a.dense<int64_t>(out, "out", rows);
  TORCH_CHECK(vocab % 8 == 0, "sample: vocab must be a multiple of 8");
  const float* tp = a.dense_opt<float>(temperature, "temperature", rows);
  const int* kp = a.dense_opt<int>(top_k, "top_k", rows);
  const float* pp = a.dense_opt<float>(top_p, "top_p", rows);
  const int64_t* sp = a.dense_opt<int64_t>(seeds, "seeds", rows);
  const int64_t* stp = a.dense_opt<int64_t>(steps, "steps", rows);
  // split greedy argmax: a row per `splits` workgroups, so that the grid reaches ~256 workgroups; part int32
  // [rows * splits * 2] scratch and cnt int32 [rows] tickets, both or neither
  int splits = 1;
  uint32_t* partp = nullptr;
  int* cntp = nullptr;
  if (part.has_value() && cnt.has_value()) {
    splits = (int)std::max<int64_t>(1, std::min<int64_t>(die::SAMPLE_MAX_SPLITS, 256 / std::max<int64_t>(1, rows)));
    partp = a.dense<uint32_t>(*part, "part", (int64_t)rows * splits * 2);
    cntp = a.dense<int>(*cnt, "cnt", rows);
  }
  int lparts = 0;
  const uint32_t* lp = lm_part_arg(a, rows, present(lm_part), &lparts);
  LAUNCH(launch_sample(op, lg.p, lg.ld, rows, vocab, tp, kp, pp, sp, stp, cur_stream(), partp, cntp, splits, lp,
                       lparts));
}

// Log-probabilities of the raw distribution for targets [rows] int64: lp fp32 / rank int32 [>= rows], and the
// top_n most likely tokens into top_lp fp32 / top_id int32 [>= rows, >= top_n] (same row stride, unit column stride).
void token_logprobs(Tensor lp, Tensor rank, Tensor top_lp, Tensor top_id, Tensor logits, Tensor targets,
                    int64_t top_n) {
  const Op a("token_logprobs", logits, "logits");
  const auto lg = a.rows(logits, "logits");
  const int rows = a.i32(logits.size(0)), vocab = a.i32(logits.size(1));
  const int64_t* tg = a.dense<int64_t>(targets, "targets", rows);
  float* lpp = a.dense<float>(lp, "lp", rows);
  int* rp = a.dense<int>(rank, "rank", rows);
  chk::Rows<float> tl;
  chk::Rows<int> ti;
  if (top_n > 0) {
    tl = a.rows<float>(top_lp, "top_lp", ge(rows), ge(top_n), false);
    ti = a.rows<int>(top_id, "top_id", ge(rows), ge(top_n), false);
    TORCH_CHECK(tl.ld == ti.ld && tl.ld >= top_lp.size(1),
                "token_logprobs: top_lp fp32 / top_id int32 [rows, >= top_n] with the same row stride");
  }
  const int n = (int)std::min<int64_t>(std::max<int64_t>(top_n, -1), 1 << 20);
  LAUNCH(launch_token_logprobs(lpp, rp, tl.p, ti.p, tl.ld, lg.p, lg.ld, rows, vocab, tg, n, cur_stream()));
}

// Penalties and logit_bias on logits [rows, vocab] in place (logit_process.hip). slot int32 [>= rows]; state int16
// [slots, vocab] (the kernel reads it as uint16; empty = no table); params fp32 [slots, 4]; bias_cnt int32 [slots];
// bias_ids int32 / bias_vals fp32 [slots, cap]; count_ids int64 [>= rows] and lm_part int32 [>= rows, parts, 2]
// optional. The launcher itself refuses vocab % 8 != 0, cap > 300 and an empty state table.
void logit_process(Tensor logits, Tensor slot, Tensor state, Tensor params, Tensor bias_cnt, Tensor bias_ids,
                   Tensor bias_vals, c10::optional<Tensor> count_ids, c10::optional<Tensor> lm_part) {
  const Op a("logit_process", logits, "logits");
  const auto lg = a.rows(logits, "logits");
  const int rows = a.i32(logits.size(0)), vocab = a.i32(logits.size(1));
  const int* sl = a.dense<int>(slot, "slot", rows);
  uint16_t* st = a.dense_opt<u16_of_i16>(state, "state", 0, {ANY, vocab});
  const int slots = st ? a.i32(state.size(0)) : 0;
  const float* pr = a.dense<float>(params, "params", 4 * (int64_t)slots, {}, 16);
  const int* bc = a.dense<int>(bias_cnt, "bias_cnt", slots);
  const int* bi = a.dense<int>(bias_ids, "bias_ids", 0, {ge(slots), ANY});
  const float* bv = a.dense<float>(bias_vals, "bias_vals", 0, {ge(slots), bias_ids.size(1)});
  const int cap = a.i32(bias_ids.size(1));
  const int64_t* cp = a.dense_opt<int64_t>(count_ids, "count_ids", rows);
  int lparts = 0;
  uint32_t* lp = lm_part_arg(a, rows, present(lm_part), &lparts);
  LAUNCH(launch_logit_process(lg.p, lg.ld, rows, vocab, sl, slots, st, pr, bc, bi, bv, cap, cp, lp, lparts,
                              cur_stream()));
}

// What the four guide ops check alike. The launchers themselves refuse vocab % 8 != 0, a bad stride, null tables and
// oversized arenas.
struct GuideArgs {
  Op a;
  chk::Rows<bf16_t> lg;
  int rows, vocab, slots;
  const int *slot, *desc;
  int *cur, *err;
  const int64_t* ap;  // advance_ids, or null
  uint32_t* lp;       // lm_part, or null
  int lparts;
};

// logits bf16 [rows, vocab] (16-B aligned); slot int32 [>= rows]; desc int32 [slots, 4]; cur / err int32 [slots];
// advance_ids int64 [>= rows] and lm_part int32 [>= rows, parts, 2] optional
GuideArgs guide_args(const char* op, const Tensor& logits, const Tensor& slot, const Tensor& desc, const Tensor& cur,
                     const Tensor& err, const c10::optional<Tensor>& advance_ids,
                     const c10::optional<Tensor>& lm_part) {
  GuideArgs g{Op(op, logits, "logits")};
  const Op& a = g.a;
  g.lg = a.rows(logits, "logits");
  g.rows = a.i32(logits.size(0));
  g.vocab = a.i32(logits.size(1));
  g.slot = a.dense<int>(slot, "slot", g.rows);
  g.desc = a.dense<int>(desc, "desc", 0, {ANY, 4}, 16);
  g.slots = a.i32(desc.size(0));
  g.cur = a.dense<int>(cur, "cur", g.slots);
  g.err = a.dense<int>(err, "err", g.slots);
  g.ap = a.dense_opt<int64_t>(advance_ids, "advance_ids", g.rows);
  g.lp = lm_part_arg(a, g.rows, present(lm_part), &g.lparts);
  return g;
}

// the vocabulary's byte table of the byte guides: tok_off int32 [n_tok + 1]; tok_bytes uint8 [B]
struct TokTable {
  const int* off;
  int64_t n_tok;
  const uint8_t* bytes;
  int64_t n_bytes;
};
TokTable guide_tok_table(const Op& a, const Tensor& tok_off, const Tensor& tok_bytes) {
  return {a.dense<int>(tok_off, "tok_off", 0, {ANY}), tok_off.numel() - 1,
          a.dense<uint8_t>(tok_bytes, "tok_bytes", 0, {ANY}), tok_bytes.numel()};
}

// Constrained decoding on logits [rows, vocab] in place (token_guide.hip). desc int32 [slots, 4]; rowptr int32 [R];
// edges int32 [E, 2]; the rest as guide_args takes it.
void token_guide(Tensor logits, Tensor slot, Tensor desc, Tensor rowptr, Tensor edges, Tensor cur, Tensor err,
                 c10::optional<Tensor> advance_ids, c10::optional<Tensor> lm_part) {
  const GuideArgs g = guide_args("token_guide", logits, slot, desc, cur, err, advance_ids, lm_part);
  const int* rp = g.a.dense<int>(rowptr, "rowptr", 0, {ANY});
  const int* ep = g.a.dense<int>(edges, "edges", 0, {ANY, 2}, 8);
  LAUNCH(launch_token_guide(g.lg.p, g.lg.ld, g.rows, g.vocab, g.slot, g.slots, g.desc, rp, rowptr.numel(), ep,
                            edges.size(0), g.cur, g.err, g.ap, g.lp, g.lparts, cur_stream()));
}

// Constrained decoding over a multi-byte vocabulary on logits [rows, vocab] in place (byte_guide.hip). desc int32
// [slots, 4] = (state_base, n_states, eos, 0); trans int16 [A, 256]; accept uint8 [A]; tok_off / tok_bytes as
// guide_tok_table takes them; cur / err are token_guide's.
void byte_guide(Tensor logits, Tensor slot, Tensor desc, Tensor trans, Tensor accept, Tensor tok_off, Tensor tok_bytes,
                Tensor cur, Tensor err, c10::optional<Tensor> advance_ids, c10::optional<Tensor> lm_part) {
  const GuideArgs g = guide_args("byte_guide", logits, slot, desc, cur, err, advance_ids, lm_part);
  const int16_t* tr = g.a.dense<int16_t>(trans, "trans", 0, {ANY, 256});
  const uint8_t* ac = g.a.dense<uint8_t>(accept, "accept", 0, {ANY});
  const TokTable t = guide_tok_table(g.a, tok_off, tok_bytes);
  LAUNCH(launch_byte_guide(g.lg.p, g.lg.ld, g.rows, g.vocab, g.slot, g.slots, g.desc, tr, trans.size(0), ac,
                           accept.numel(), t.off, t.n_tok, t.bytes, t.n_bytes, g.cur, g.err, g.ap, g.lp, g.lparts,
                           cur_stream()));
}

// JSON mode on logits [rows, vocab] in place (json_guide.hip). desc int32 [slots, 4] = (n_states, done, eos, 0); trans
// int16 [S, 256], the pushdown table; tok_off / tok_bytes: byte_guide's tables; cur / err are token_guide's; jstk
// int32 [slots, 2] = (depth, stack bits).
void json_guide(Tensor logits, Tensor slot, Tensor desc, Tensor trans, Tensor tok_off, Tensor tok_bytes, Tensor cur,
                Tensor jstk, Tensor err, c10::optional<Tensor> advance_ids, c10::optional<Tensor> lm_part) {
  const GuideArgs g = guide_args("json_guide", logits, slot, desc, cur, err, advance_ids, lm_part);
  const int16_t* tr = g.a.dense<int16_t>(trans, "trans", 0, {ANY, 256});
  const TokTable t = guide_tok_table(g.a, tok_off, tok_bytes);
  int* js = g.a.dense<int>(jstk, "jstk", 0, {ge(g.slots), 2});
  LAUNCH(launch_json_guide(g.lg.p, g.lg.ld, g.rows, g.vocab, g.slot, g.slots, g.desc, tr, trans.size(0), t.off,
                           t.n_tok, t.bytes, t.n_bytes, g.cur, js, g.err, g.ap, g.lp, g.lparts, cur_stream()));
}

// Structured outputs on logits [rows, vocab] in place (schema_guide.hip). desc int32 [slots, 4] = (state_base,
// n_states, eos, 0); trans int32 [A, 256] and accept uint8 [A], the pushdown arenas; tok_off / tok_bytes: byte_guide's
// tables; cur / err are token_guide's; sdep int32 [slots] and sstk int16 [slots, 32], the depth and the return states.
void schema_guide(Tensor logits, Tensor slot, Tensor desc, Tensor trans, Tensor accept, Tensor tok_off,
                  Tensor tok_bytes, Tensor cur, Tensor sdep, Tensor sstk, Tensor err,
                  c10::optional<Tensor> advance_ids, c10::optional<Tensor> lm_part) {
  const GuideArgs g = guide_args("schema_guide", logits, slot, desc, cur, err, advance_ids, lm_part);
  const int* tr = g.a.dense<int>(trans, "trans", 0, {ANY, 256});
  const uint8_t* ac = g.a.dense<uint8_t>(accept, "accept", 0, {ANY});
  const TokTable t = guide_tok_table(g.a, tok_off, tok_bytes);
  int* sd = g.a.dense<int>(sdep, "sdep", g.slots);
  int16_t* ss = g.a.dense<int16_t>(sstk, "sstk", 0, {ge(g.slots), die::GUIDE_SCHEMA_MAX_DEPTH});
  LAUNCH(launch_schema_guide(g.lg.p, g.lg.ld, g.rows, g.vocab, g.slot, g.slots, g.desc, tr, trans.size(0), ac,
                             accept.numel(), t.off, t.n_tok, t.bytes, t.n_bytes, g.cur, sd, ss, g.err, g.ap, g.lp,
                             g.lparts, cur_stream()));
}

// Embedding pooling (pooling.hip): hidden bf16 [T, H] (row stride allowed); segs int32 [S, 8]; acc fp32 [slots, H]
// (optional: only mean pooling reads or writes it); out fp32 [S, H]; part fp32 [P, H] and tickets int32 [>= S]
// (optional, both or neither: the scratch of segments split over max_parts > 1 workgroups). The launcher itself
// refuses H % 8 != 0, a bad stride, bad dims and a bad max_parts.
void pool_embed(Tensor out, c10::optional<Tensor> acc, Tensor hidden, Tensor segs, int64_t dims, bool normalize,
                c10::optional<Tensor> part, c10::optional<Tensor> tickets, int64_t max_parts) {
  const Op a("pool_embed", hidden, "hidden");
  const auto h = a.rows(hidden, "hidden", ANY, ANY, false);
  const int T = a.i32(hidden.size(0)), H = a.i32(hidden.size(1));
  const int* sg = a.dense<int>(segs, "segs", 0, {ANY, 8});
  const int S = a.i32(segs.size(0));
  float* op = a.dense<float>(out, "out", 0, {ge(S), H});
  float* ap = a.dense_opt<float>(acc, "acc", 0, {ANY, H});
  const int slots = ap ? a.i32(acc->size(0)) : 0;
  TORCH_CHECK(part.has_value() == tickets.has_value(), "pool_embed: part and tickets go together");
  float* pp = a.dense_opt<float>(part, "part", 0, {ANY, H});
  int* tp = a.dense_opt<int>(tickets, "tickets", 0, {ANY});
  const int pcap = part.has_value() ? a.i32(part->size(0)) : 0, tcap = tickets.has_value() ? a.i32(tickets->numel()) : 0;
  TORCH_CHECK(dims >= 0 && dims <= H, "pool_embed: dims in [0, H]");
  TORCH_CHECK(max_parts >= 1 && max_parts <= die::POOL_MAX_PARTS, "pool_embed: max_parts in [1, ", die::POOL_MAX_PARTS, "]");
  LAUNCH(launch_pool_embed(op, ap, slots, h.p, h.ld, T, H, sg, S, (int)dims, normalize, pp, pcap, tp, tcap,
                           (int)max_parts, cur_stream()));
}

// The buffers a decode window's step advances (decode_step.hip; sampling.hip with a SampleAdvance): ids / pos / slots
// / step int64 and ctx int32 [>= rows], bt int32 [>= rows, W], tokens int64 [K, >= rows], cnt / n_real int32 [>= 1].
die::SampleAdvance advance_args(const Op& a, int64_t rows, const Tensor& ids, const Tensor& pos, const Tensor& ctx,
                                const Tensor& slots, const Tensor& bt, const Tensor& step, const Tensor& tokens,
                                const Tensor& cnt, const Tensor& n_real, int64_t block_size) {
  die::SampleAdvance adv;
  adv.ids = a.dense<int64_t>(ids, "ids", rows);
  adv.pos = a.dense<int64_t>(pos, "pos", rows);
  adv.ctx = a.dense<int>(ctx, "ctx", rows);
  adv.slots = a.dense<int64_t>(slots, "slots", rows);
  adv.bt = a.dense<int>(bt, "bt", 0, {ge(rows), ANY});
  adv.bt_width = a.i32(bt.size(1));
  adv.step = a.dense<int64_t>(step, "step", rows);
  adv.tokens = a.dense<int64_t>(tokens, "tokens", 0, {ANY, ge(rows)});
  adv.tok_stride = a.i32(tokens.size(1));
  adv.k_max = a.i32(tokens.size(0));
  adv.cnt = a.dense<int>(cnt, "cnt", 1);
  adv.n_real = a.dense<int>(n_real, "n_real", 1);
  adv.bs = a.i32(block_size);
  return adv;
}

// A decode step's sampling from the LM head's candidates (sample(..., lm_part)) that also advances the step's
// inputs as decode_advance does (ids / pos / ctx / slots / step, the window's token row, the step counter cnt[0]),
// one workgroup per row; ticket: int32 [1], zero, re-armed by the kernel.
void sample_advance(Tensor out, Tensor logits, Tensor temperature, Tensor top_k, Tensor top_p, Tensor seeds,
                    Tensor lm_part, Tensor ids, Tensor pos, Tensor ctx, Tensor slots, Tensor bt, Tensor step,
                    Tensor tokens, Tensor cnt, Tensor n_real, int64_t block_size, Tensor ticket, Tensor table,
                    Tensor h_out, Tensor ssp_out) {
  const Op a("sample_advance", logits, "logits");
  const auto lg = a.rows(logits, "logits");
  const int rows = a.i32(logits.size(0)), vocab = a.i32(logits.size(1));
  TORCH_CHECK(vocab % 8 == 0, "sample_advance: vocab must be a multiple of 8");
  int64_t* op = a.dense<int64_t>(out, "out", rows);
  const float* tp = a.dense<float>(temperature, "temperature", rows);
  const int* kp = a.dense<int>(top_k, "top_k", rows);
  const float* pp = a.dense<float>(top_p, "top_p", rows);
  const int64_t* sp = a.dense<int64_t>(seeds, "seeds", rows);
  int lparts = 0;
  const uint32_t* lp = lm_part_arg(a, rows, &lm_part, &lparts);
  die::SampleAdvance adv = advance_args(a, rows, ids, pos, ctx, slots, bt, step, tokens, cnt, n_real, block_size);
  adv.ticket = a.dense<int>(ticket, "ticket", 1);
  if (present(table)) {  // also the next step's embedding rows + first-norm statistics (as embed_sumsq)
    adv.table = a.dense<bf16_t>(table, "table", 0, {ANY, ANY});
    adv.hidden = a.i32(table.size(1));
    TORCH_CHECK(adv.hidden % 8 == 0, "sample_advance: table [V, H], H a multiple of 8");
    adv.h_out = a.dense<bf16_t>(h_out, "h_out", 0, {ge(rows), adv.hidden});
    adv.ssp_out = a.dense<float>(ssp_out, "ssp_out", rows);
  }
  LAUNCH(launch_sample(op, lg.p, lg.ld, rows, vocab, tp, kp, pp, sp, adv.step, cur_stream(), nullptr, nullptr, 1, lp,
                       lparts, adv));
}

// Decode-step input advance (decode_step.hip), for multi-step decode windows.
void decode_advance(Tensor out, Tensor ids, Tensor pos, Tensor ctx, Tensor slots, Tensor bt, Tensor step,
                    Tensor tokens, Tensor cnt, Tensor n_real, int64_t rows, int64_t block_size) {
  const Op a("decode_advance", out, "out");
  const int64_t* op = a.dense<int64_t>(out, "out", rows);
  const die::SampleAdvance v = advance_args(a, rows, ids, pos, ctx, slots, bt, step, tokens, cnt, n_real, block_size);
  LAUNCH(launch_decode_advance(op, v.ids, v.pos, v.ctx, v.slots, v.bt, v.bt_width, v.step, v.tokens, v.tok_stride,
                               v.cnt, v.n_real, a.i32(rows), v.bs, v.k_max, cur_stream()));
}

// The KV pool [planes, num_blocks, ...] as the block movers see it: [planes, num_blocks, slab]
struct Pool {
  bf16_t* p;
  int planes;
  int64_t nb, slab;
};
Pool pool_arg(const Op& a, const Tensor& pool) {
  TORCH_CHECK(pool.dim() >= 3, a.op, ": pool must be [planes, num_blocks, ...]");
  const int64_t blocks = pool.size(0) * pool.size(1);
  return {a.dense<bf16_t>(pool, "pool", 0), a.i32(pool.size(0)), pool.size(1), blocks ? pool.numel() / blocks : 0};
}

void copy_blocks(Tensor pool, Tensor pairs) {
  const Op a("copy_blocks", pool, "pool");
  const Pool p = pool_arg(a, pool);
  const int64_t* pr = a.dense<int64_t>(pairs, "pairs", 0, {ANY, 2});
  LAUNCH(launch_copy_blocks(p.p, pr, a.i32(pairs.size(0)), p.planes, p.nb, p.slab, cur_stream()));
}

void move_blocks(Tensor pool, Tensor buf, Tensor ids, bool gather) {
  const Op a("move_blocks", pool, "pool");
  const Pool p = pool_arg(a, pool);
  const int64_t* ip = a.dense<int64_t>(ids, "ids", 0);
  const int n = a.i32(ids.numel());
  bf16_t* bp = a.dense<bf16_t>(buf, "buf", n * p.planes * p.slab);
  LAUNCH(launch_move_blocks(p.p, bp, ip, n, p.planes, p.nb, p.slab, gather, cur_stream()));
}

// pool [planes, blocks, ...]: planes [plane0, plane0 + nplanes) of blocks ids[i] into the packet row at address
// dst[i] (int64 device array; each row holds `planes` slabs). The caller keeps the destinations alive and sized.
void gather_blocks_rows(Tensor pool, Tensor ids, Tensor dst, int64_t plane0, int64_t nplanes) {
  const Op a("gather_blocks_rows", pool, "pool");
  const Pool p = pool_arg(a, pool);
  const int64_t* ip = a.dense<int64_t>(ids, "ids", 0);
  const int64_t* dp = a.dense<int64_t>(dst, "dst", ids.numel());
  const int n = a.i32(ids.numel());
  TORCH_CHECK(dst.numel() == n, "gather_blocks_rows: ids / dst: int64 device arrays of one length");
  TORCH_CHECK(plane0 >= 0 && nplanes >= 0 && plane0 + nplanes <= p.planes, "plane range outside the pool");
  LAUNCH(launch_gather_blocks_rows(p.p, ip, dp, n, (int)plane0, (int)nplanes, p.nb, p.slab, cur_stream()));
}

void topk_softmax(Tensor w, Tensor ids, Tensor gating, bool renorm) {
  const Op a("topk_softmax", gating, "gating");
  const bf16_t* gp = a.dense<bf16_t>(gating, "gating", 0, {ANY, ANY});
  const int T = a.i32(gating.size(0)), E = a.i32(gating.size(1));
  float* wp = a.dense<float>(w, "w", 0, {T, ANY});
  int* ip = a.dense<int>(ids, "ids", 0, {T, w.size(1)});
  LAUNCH(launch_topk_softmax(wp, ip, gp, T, E, a.i32(w.size(1)), renorm, cur_stream()));
}

void moe_align(Tensor offsets, Tensor sorted, Tensor pos, Tensor ids, int64_t num_experts) {
  const Op a("moe_align", offsets, "offsets");
  const int n = a.i32(ids.numel());
  int* op = a.dense<int>(offsets, "offsets", num_experts + 1);
  int* sp = a.dense<int>(sorted, "sorted", n);
  int* pp = a.dense<int>(pos, "pos", n);
  const int* ip = a.dense<int>(ids, "ids", 0);
  LAUNCH(launch_moe_align(op, sp, pp, ip, n, a.i32(num_experts), cur_stream()));
}

void moe_gather(Tensor xs, Tensor x, Tensor sorted, int64_t topk) {
  const Op a("moe_gather", xs, "xs");
  const bf16_t* xp = a.dense<bf16_t>(x, "x", 0, {ANY, ANY});
  const int H = a.i32(x.size(1)), n = a.i32(x.size(0) * topk);
  bf16_t* xsp = a.dense<bf16_t>(xs, "xs", 0, {n, H});
  const int* sp = a.dense<int>(sorted, "sorted", n);
  TORCH_CHECK(sorted.numel() == n, "moe_gather: sorted [T * topk]");
  LAUNCH(launch_moe_gather(xsp, xp, sp, n, a.i32(topk), H, cur_stream()));
}

// what moe_combine and moe_combine_residual check alike: ys bf16 [T * K, H], pos int32 [T * K], w fp32 [T, K]
struct Combine {
  const bf16_t* ys;
  const int* pos;
  const float* w;
  int K;
};
Combine combine_args(const Op& a, const Tensor& ys, const Tensor& pos, const Tensor& w, int T, int H) {
  Combine c;
  c.w = a.dense<float>(w, "w", 0, {T, ANY});
  c.K = a.i32(w.size(1));
  c.pos = a.dense<int>(pos, "pos", (int64_t)T * c.K);
  TORCH_CHECK(pos.numel() == (int64_t)T * c.K, a.op, ": pos [T * K]");
  c.ys = a.dense<bf16_t>(ys, "ys", 0, {(int64_t)T * c.K, H});
  return c;
}

void moe_combine(Tensor out, Tensor ys, Tensor pos, Tensor w) {
  const Op a("moe_combine", out, "out");
  bf16_t* op = a.dense<bf16_t>(out, "out", 0, {ANY, ANY});
  const int T = a.i32(out.size(0)), H = a.i32(out.size(1));
  const Combine c = combine_args(a, ys, pos, w, T, H);
  LAUNCH(launch_moe_combine(op, c.ys, c.pos, c.w, T, c.K, H, cur_stream()));
}

// Fused decode routing: w [T, K] fp32, ids [T, K] int32 from x [T, H] (row stride ldx) and the router
// weights wg [E, H] bf16 (moe.hip moe_route_kernel).
void moe_route(Tensor w, Tensor ids, Tensor x, Tensor wg, bool renorm) {
  const Op a("moe_route", x, "x");
  const auto xr = a.rows(x, "x");
  const int T = a.i32(x.size(0)), H = a.i32(x.size(1));
  const bf16_t* gp = a.dense<bf16_t>(wg, "wg", 0, {ANY, H});
  float* wp = a.dense<float>(w, "w", 0, {T, ANY});
  int* ip = a.dense<int>(ids, "ids", 0, {T, w.size(1)});
  LAUNCH(launch_moe_route(wp, ip, xr.p, xr.ld, gp, T, H, a.i32(wg.size(0)), a.i32(w.size(1)), renorm,
                          cur_stream()));
}

// resid [T, H] += combine(ys, pos, w); ssp [>= T] fp32 = row sums of squares of the new residual.
void moe_combine_residual(Tensor ssp, Tensor resid, Tensor ys, Tensor pos, Tensor w) {
  const Op a("moe_combine_residual", resid, "resid");
  const auto r = a.rows(resid, "resid");
  const int T = a.i32(resid.size(0)), H = a.i32(resid.size(1));
  const Combine c = combine_args(a, ys, pos, w, T, H);
  float* sp = a.dense<float>(ssp, "ssp", T);
  LAUNCH(launch_moe_combine_residual(sp, r.p, r.ld, c.ys, c.pos, c.w, T, c.K, H, cur_stream()));
}

// Decode GEMM (gemm_decode.hip), x [M <= 128, K] @ w^T. mode 0 bf16 y [M, N]; 1 silu(x gate^T) * (x up^T)
// with w = [gate; up]; 2 fp32 split-K slabs [sk, M, N]; 3 slabs + residual update of `resid` [M, N] and row
// sums of squares `ssp_out` [N/wr, 128] (tickets `counters` [N/wr], zeroed once); 4 = mode 1 with rows
// scaled by the RMSNorm statistics `ssp_in` [T, 128] (eps; the norm weight is folded into w). (wr, kc):
// weight rows and K elements per ring slot of a workgroup. Unused fusion tensors may be empty.
// Diagnostics: when set (non-empty int64 tensor [>= 3 * workgroups]), every decode-GEMM launch writes
// per-workgroup [start, end, xcc] s_memrealtime stamps (100 MHz) there (bench/micro_gd_timeline.py).
long long* g_gd_ts = nullptr;
// decode-GEMM tiles that are instantiated (gd_tiles.h; gemm_decode.hip launch_gemm_decode dispatches on the same list)
bool gd_tile_ok(int64_t wr, int64_t kc) {
#define GD_TILE(WR, KC) \
  if (wr == WR && kc == KC) return true;
  GD_TILES(GD_TILE)
#undef GD_TILE
  return false;
}

// a diagnostics buffer: int64 stamps on a GPU, empty = off
long long* stamps_arg(const char* op, const Tensor& t) {
  return present(t) ? reinterpret_cast<long long*>(Op(op, t, "t").dense<int64_t>(t, "t", 0)) : nullptr;
}
void gd_set_timestamps(Tensor t) { g_gd_ts = stamps_arg("gd_set_timestamps", t); }
void attn_set_timestamps(Tensor t) { die::attn_set_timestamps(stamps_arg("attn_set_timestamps", t)); }
void attn_set_few_pair_parts(bool on) { die::attn_set_few_pair_parts(on); }

// The layout flags of a gemm mode word into fz; returns the mode proper (bits 0..4). Bit 32: w pre-packed by
// ops.gd_pack_weights for this (mode, wr) (TILED); bit 64: the half-LDS ring (mode 3, <= 32 rows), two workgroups
// resident per CU; bit 128: w in the lossless 13-bit layout (ops.gd_pack_weights_p13), its base7 in bits 8..14.
int64_t gd_mode(int64_t mode, die::GemmDecodeFuse& fz) {
  fz.tiled = (mode & 32) != 0 ? 1 : 0;
  fz.half_ring = (mode & 64) != 0 ? 1 : 0;
  fz.p13 = (mode & 128) != 0 ? 1 : 0;
  fz.p13_base7 = fz.p13 ? (int)((mode >> 8) & 127) : 0;
  return mode & 31;
}

void gemm_decode_impl(Tensor y, Tensor x, Tensor w, int64_t mode, int64_t wr, int64_t kc, int64_t sk, bool nt,
                      Tensor resid, Tensor ssp_out, Tensor counters, Tensor ssp_in, double eps,
                      die::GemmDecodeFuse fz) {
  const Op a("gemm_decode", x, "x");
  const auto xr = a.rows(x, "x");
  mode = gd_mode(mode, fz);
  TORCH_CHECK(!(fz.p13 && fz.tiled), "gemm_decode: P13 weights are not also TILED");
  const int M = a.i32(x.size(0)), K = a.i32(x.size(1));
  TORCH_CHECK(M >= 1 && M <= 128, "gemm_decode: 1 <= M <= 128");
  TORCH_CHECK(gd_tile_ok(wr, kc), "gemm_decode: unsupported (wr, kc) tile");
  TORCH_CHECK(mode >= 0 && mode <= 6 && mode != 5, "gemm_decode: mode");
  TORCH_CHECK(sk >= 1 && K % kc == 0 && K / kc >= sk, "gemm_decode: K must be a multiple of kc with >= sk K-slots");
  const bool silu = mode == 1 || mode == 4 || mode == 6;
  void* yp;
  int64_t N, ldy;
  if (mode == 2 || mode == 3) {
    yp = a.dense<float>(y, "y", 0, {sk, M, ANY});  // slabs [sk, M, N]
    N = ldy = y.size(2);
  } else {
    TORCH_CHECK(sk == 1 || mode == 6, "gemm_decode: bf16 output: sk == 1 (mode 6: any)");
    const auto yr = a.rows(y, "y", M, ANY);
    yp = yr.p;
    N = y.size(1);
    ldy = yr.ld;
  }
  const int64_t wrows = silu ? 2 * N : N;
  const bf16_t* wp = a.dense<bf16_t>(w, "w", 0, {fz.p13 ? wrows * 13 / 16 : wrows, K});
  TORCH_CHECK(!fz.p13 || wrows * 13 % 16 == 0, "gemm_decode: P13 w rows");
  TORCH_CHECK(N % (silu ? wr / 2 : wr) == 0, "gemm_decode: N not a multiple of the column tile");
  TORCH_CHECK((int64_t)sk * M * N * 4 < ((int64_t)1 << 31) || mode != 3, "gemm_decode: slab too large");
  fz.ts = g_gd_ts;
  if (mode == 3) {
    TORCH_CHECK(wr == 32 || wr == 64 || wr == 128, "gemm_decode: mode 3: wr in {32, 64, 128}");
    const auto r = a.rows(resid, "resid", ge(M), N);
    fz.resid = r.p;
    fz.ld_resid = r.ld;
    fz.ssp_out = a.dense<float>(ssp_out, "ssp_out", (N / wr) * die::DECODE_SSP_LD);
    if (sk > 1) fz.counters = a.dense<int>(counters, "counters", N / wr);
  }
  if (mode == 6 && sk > 1) {  // split-K SiLU: ssp_out carries the fp32 partial slab [sk, M, 2N], counters the tickets
    TORCH_CHECK(sk * M * 2 * N * 4 < ((int64_t)1 << 31), "gemm_decode: mode 6 slab too large");
    fz.slab6 = a.dense<float>(ssp_out, "ssp_out", sk * M * 2 * N);
    fz.ld_slab6 = 2 * N;
    fz.counters = a.dense<int>(counters, "counters", N / (wr / 2));
  }
  if (mode == 4 || mode == 6) {
    fz.ssp_in = a.dense<float>(ssp_in, "ssp_in", 0, {ANY, die::DECODE_SSP_LD});
    TORCH_CHECK(ssp_in.size(0) >= 1 &&
                    ssp_in.size(0) <= (M <= 32 ? die::DECODE_SSP_MAX_TILES : die::DECODE_SSP_MAX_TILES_WIDE),
                "gemm_decode: ssp_in [tiles <= 256 (<= 128 above 32 rows), 128]");
    fz.ssp_tiles = a.i32(ssp_in.size(0));
    fz.inv_n = 1.f / (float)K;
    fz.eps = (float)eps;
  }
  LAUNCH(launch_gemm_decode(yp, ldy, xr.p, xr.ld, wp, M, a.i32(N), K, (int)mode, (int)wr, (int)kc, a.i32(sk), nt, fz,
                            cur_stream()));
}

void gemm_decode(Tensor y, Tensor x, Tensor w, int64_t mode, int64_t wr, int64_t kc, int64_t sk, bool nt,
                 Tensor resid, Tensor ssp_out, Tensor counters, Tensor ssp_in, double eps) {
  gemm_decode_impl(y, x, w, mode, wr, kc, sk, nt, resid, ssp_out, counters, ssp_in, eps, die::GemmDecodeFuse{});
}

// Resident workgroups per CU of the decode-GEMM instantiation a launch with these parameters would use (mode word
// as for gemm_decode, layout bits included; rows = the step's row count): hipOccupancyMaxActiveBlocksPerMultiprocessor
// on that kernel with its LDS, no launch. -1 if no such instantiation exists. The TP exchange's residency rule
// (CustomAllReduce.fused_ok) is built on it.
int64_t gd_occupancy(int64_t mode, int64_t wr, int64_t kc, int64_t sk, int64_t rows, bool nt) {
  if (!gd_tile_ok(wr, kc) || rows < 1 || rows > 128 || sk < 1) return -1;
  die::GemmDecodeFuse fz;
  const int m = (int)gd_mode(mode, fz);
  // stand-ins for the pointers the launcher validates (never dereferenced: nothing is launched)
  static char dummy[64];
  fz.resid = reinterpret_cast<bf16_t*>(dummy);
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
  const hipError_t e = die::launch_gemm_decode(dummy, n, reinterpret_cast<const bf16_t*>(dummy), k,
                                               reinterpret_cast<const bf16_t*>(dummy), (int)rows, n, k, m,
                                               (int)wr, (int)kc, (int)sk, nt, fz, cur_stream());
  return e == hipSuccess ? occ : -1;
}

// y = x @ w^T (mode 0, bf16) that also writes each column tile's per-row greedy candidate into amax
// [M, N / wr, 2] int32 (value bits, column): the decode step's LM head, whose argmax then reduces N / wr
// candidates per row (sample(..., lm_part=amax)) instead of re-reading the logits.
// layout: 0 row-major w, 1 tile order (TILED), or a mode word's layout flags (P13 | base7 << 8).
void gemm_decode_argmax(Tensor y, Tensor x, Tensor w, int64_t wr, int64_t kc, int64_t layout, Tensor amax) {
  const Op a("gemm_decode_argmax", x, "x");
  TORCH_CHECK(x.dim() == 2 && y.dim() == 2 && y.is_contiguous() && y.size(1) % 8 == 0 && wr >= 1,
              "gemm_decode_argmax: x [M, K] with a contiguous y of N % 8 == 0 columns");
  die::GemmDecodeFuse fz;
  fz.amax = a.dense<uint32_t>(amax, "amax", 0, {ge(x.size(0)), y.size(1) / wr, 2});
  fz.amax_parts = a.i32(amax.size(1));
  TORCH_CHECK(layout >= 0 && (layout & 31) <= 1, "gemm_decode_argmax: layout");
  gemm_decode_impl(y, x, w, layout == 1 ? 32 : layout, wr, kc, 1, true, x, x, x, x, 0.0, fz);
}

// The group's peers of the one-shot collectives: every rank's staging buffer and flag page as raw addresses
// (IPC-mapped by src/parallel/custom_allreduce.py), with this rank and the control words.
struct Car {
  die::CarPeers peers;
  int world, rank;
  uint32_t* ctl;
};
Car car_peers(const char* op, int64_t rank, const std::vector<int64_t>& bufs, const std::vector<int64_t>& sigs,
              int64_t ctl) {
  Car c;
  c.world = (int)bufs.size();
  TORCH_CHECK(c.world >= 2 && c.world <= die::CAR_MAX_RANKS && (int)sigs.size() == c.world, op, ": 2..8 ranks");
  TORCH_CHECK(rank >= 0 && rank < c.world && ctl != 0, op, ": bad rank / control word");
  for (int p = 0; p < c.world; ++p) {
    TORCH_CHECK(bufs[p] != 0 && sigs[p] != 0, op, ": null peer pointer");
    c.peers.buf[p] = reinterpret_cast<bf16_t*>(bufs[p]);
    c.peers.sig[p] = reinterpret_cast<uint32_t*>(sigs[p]);
  }
  c.rank = (int)rank;
  c.ctl = reinterpret_cast<uint32_t*>(ctl);
  return c;
}

// Tensor-parallel row-parallel projection in ONE launch (decode, mode 3): this rank's K-shard GEMM, the one-shot
// all-reduce of each column tile with the group's peers (the CustomAllReduce's staging buffers, flag pages and
// control words: bufs / sigs / ctl / cap as for car_all_reduce), the residual update and the next norm's per-tile
// statistics. Every rank of the group must make the same call (same shapes, same tile plan).
void gemm_decode_car(Tensor y, Tensor x, Tensor w, int64_t mode, int64_t wr, int64_t kc, int64_t sk, bool nt,
                     Tensor resid, Tensor ssp_out, Tensor counters, int64_t rank, std::vector<int64_t> bufs,
                     std::vector<int64_t> sigs, int64_t ctl, int64_t cap_elems) {
  TORCH_CHECK((mode & 31) == 3, "gemm_decode_car: mode 3 (residual epilogue)");
  const Car c = car_peers("gemm_decode_car", rank, bufs, sigs, ctl);
  TORCH_CHECK(x.dim() == 2 && resid.dim() == 2 && x.size(0) * resid.size(1) <= cap_elems,
              "gemm_decode_car: message larger than the staging half");
  TORCH_CHECK(wr >= 1 && resid.size(1) / wr <= die::CAR_MAX_BLOCKS, "gemm_decode_car: more column tiles than flag slots");
  die::GemmDecodeFuse fz;
  fz.car = c.peers;
  fz.car_world = c.world;
  fz.car_rank = c.rank;
  fz.car_ctl = c.ctl;
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
  const Op a("gemm_decode_grouped", x, "x");
  const auto xr = a.rows(x, "x");
  const int K = a.i32(x.size(1));
  TORCH_CHECK(mode == 0 || mode == 1, "grouped: mode 0 or 1");
  const bf16_t* wp = a.dense<bf16_t>(w, "w", 0, {ANY, ANY, K});  // [E, rows, K]
  const int64_t E = w.size(0), N = mode == 1 ? w.size(1) / 2 : w.size(1);
  // segs > 1: expert e's rows come as segs groups (offsets [E * segs + 1], group g -> expert g / segs), each
  // of at most max_rows rows, for steps whose experts may get more rows than the activation image holds
  TORCH_CHECK(segs >= 1, "grouped: segs >= 1");
  die::GemmDecodeFuse fz;
  fz.grp_off = a.dense<int>(offsets, "offsets", E * segs + 1);
  fz.grp_wstride = w.size(1) * K;
  fz.grp_n = a.i32(E * segs);
  fz.grp_div = a.i32(segs);
  // rows (optional, numel 0 = absent): x in token order, row j of the sorted order = rows[j] / k
  const auto yr = a.rows(y, "y", ANY, N);
  fz.grp_rows = a.dense_opt<int>(rows, "rows", y.size(0));
  if (fz.grp_rows) {
    TORCH_CHECK(k >= 1 && rows.numel() == y.size(0) && x.size(0) * k == y.size(0), "grouped gather: rows [T*k]");
    fz.grp_k = a.i32(k);
  }
  TORCH_CHECK((fz.grp_rows || y.size(0) == x.size(0)) && y.size(0) >= 1, "grouped: y [R, N], at least one row");
  TORCH_CHECK(gd_tile_ok(wr, kc), "grouped: unsupported (wr, kc) tile");
  // max_rows bounds every expert's rows (a token routes to an expert at most once: <= tokens); it picks
  // the activation image (16 / 32 / 64 / 128 rows) and clamps each group to it
  TORCH_CHECK(max_rows >= 1 && max_rows <= 128, "grouped: 1 <= max_rows <= 128");
  TORCH_CHECK(K % kc == 0 && N % (mode == 1 ? wr / 2 : wr) == 0, "grouped: tile shape");
  LAUNCH(launch_gemm_decode(yr.p, yr.ld, xr.p, xr.ld, wp, (int)std::min<int64_t>(y.size(0), max_rows), a.i32(N), K,
                            (int)mode, (int)wr, (int)kc, 1, true, fz, cur_stream()));
}

// Decode-step embedding gather + first-norm statistics (norm_act.hip): out [M, H] = table[ids], ssp[0][m] = sum of
// squares of out[m]
void embed_sumsq(Tensor out, Tensor ssp, Tensor table, Tensor ids) {
  const Op a("embed_sumsq", table, "table");
  const bf16_t* tp = a.dense<bf16_t>(table, "table", 0, {ANY, ANY});
  const int64_t* ip = a.dense<int64_t>(ids, "ids", 0);
  const int M = a.i32(ids.numel()), H = a.i32(table.size(1));
  bf16_t* op = a.dense<bf16_t>(out, "out", 0, {M, H});
  float* sp = a.dense<float>(ssp, "ssp", die::DECODE_SSP_LD);
  TORCH_CHECK(M >= 1 && M <= die::DECODE_SSP_LD && H % 8 == 0,
              "embed_sumsq: 1 <= M <= 128 rows, ssp [1, 128], H % 8 == 0");
  LAUNCH(launch_embed_sumsq(op, sp, tp, ip, M, H, cur_stream()));
}

void residual_add_sumsq(Tensor ssp, Tensor resid, Tensor x) {
  const Op a("residual_add_sumsq", x, "x");
  const auto xr = a.rows(x, "x");
  const int T = a.i32(x.size(0)), H = a.i32(x.size(1));
  const auto r = a.rows(resid, "resid", T, H);
  float* sp = a.dense<float>(ssp, "ssp", T);
  TORCH_CHECK(T <= die::DECODE_SSP_LD, "residual_add_sumsq: x [<= 128, H]");
  LAUNCH(launch_residual_add_sumsq(sp, r.p, xr.p, T, H, r.ld, xr.ld, cur_stream()));
}

void row_sumsq(Tensor ssp, Tensor x) {
  const Op a("row_sumsq", x, "x");
  const auto xr = a.rows(x, "x");
  const int T = a.i32(x.size(0));
  float* sp = a.dense<float>(ssp, "ssp", T);
  TORCH_CHECK(T <= die::DECODE_SSP_LD, "row_sumsq: x [<= 128, H], ssp [1, 128]");
  LAUNCH(launch_row_sumsq(sp, xr.p, T, a.i32(x.size(1)), xr.ld, cur_stream()));
}

void fused_add_rms_norm_slab(Tensor out, Tensor slab, Tensor residual, Tensor w, double eps) {
  const Op a("fused_add_rms_norm_slab", slab, "slab");
  bf16_t* rp = a.dense<bf16_t>(residual, "residual", 0, {ANY, ANY});
  const int T = a.i32(residual.size(0)), H = a.i32(residual.size(1));
  const float* sp = a.dense<float>(slab, "slab", 0, {ANY, T, H});  // [sk, rows, hidden]
  const auto o = a.rows(out, "out", T, H);
  const bf16_t* wp = a.dense<bf16_t>(w, "w", H);
  TORCH_CHECK(w.numel() == H && H <= MAX_HIDDEN && H % 8 == 0, "fused_add_rms_norm_slab: w [hidden], hidden");
  LAUNCH(launch_fused_add_rms_norm_slab(o.p, sp, a.i32(slab.size(0)), rp, wp, (float)eps, T, H, o.ld, cur_stream()));
}

void rope_and_cache_slab(Tensor q_out, Tensor slab, Tensor positions, Tensor cos_sin, Tensor slot_mapping,
                         Tensor k_cache, Tensor v_cache, int64_t hq, int64_t hkv, int64_t head_dim) {
  const Op a("rope_and_cache_slab", slab, "slab");
  const float* sp = a.dense<float>(slab, "slab", 0, {ANY, ANY, (hq + 2 * hkv) * head_dim});  // [sk, T, (hq+2hkv)*D]
  const int T = a.i32(slab.size(1));
  bf16_t* qp = a.dense<bf16_t>(q_out, "q_out", T * hq * head_dim);
  const RopeIndex ix = check_rope_index(a, positions, slot_mapping, cos_sin, T, head_dim);
  bf16_t* kc = check_cache(a, k_cache, hkv, head_dim, "k_cache");
  bf16_t* vc = check_cache(a, v_cache, hkv, head_dim, "v_cache");
  const int bs = a.i32(k_cache.size(2));
  LAUNCH(launch_rope_and_cache_slab(qp, sp, a.i32(slab.size(0)), ix.pos, ix.cos_sin, ix.slots, kc, vc, T, a.i32(hq),
                                    a.i32(hkv), a.i32(head_dim), bs, cur_stream()));
}

// ---- one-shot all-reduce over IPC-mapped peer buffers (src/parallel/custom_allreduce.py)
int64_t car_alloc(int64_t bytes, bool uncached) {
  TORCH_CHECK(bytes > 0 && bytes % 256 == 0, "car_alloc: bytes must be a positive multiple of 256");
  void* p = nullptr;
  HIP_OK(die::car_malloc(&p, (size_t)bytes, uncached));
  return reinterpret_cast<int64_t>(p);
}

// dst_ptr (raw device pointer, e.g. an IPC-mapped peer buffer) <- src (contiguous GPU tensor of any dtype), by a
// copy kernel on the current stream
void car_copy_to(int64_t dst_ptr, Tensor src) {
  const Op a("car_copy_to", src, "src");
  const int64_t nbytes = src.numel() * src.element_size();
  TORCH_CHECK(dst_ptr != 0 && nbytes % 16 == 0, "car_copy_to: null destination or size not a multiple of 16");
  const void* sp = a.dense<void>(src, "src", 0);
  LAUNCH(launch_ipc_copy(reinterpret_cast<void*>(dst_ptr), sp, nbytes, cur_stream()));
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

std::vector<int64_t> car_read_words(int64_t ptr, int64_t n) {  // synchronising host read of uint32 words
  TORCH_CHECK(n > 0 && n <= 64, "car_read_words: 1..64 words");
  std::vector<uint32_t> h((size_t)n);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(h.data(), reinterpret_cast<void*>(ptr), (size_t)n * 4, hipMemcpyDeviceToHost));
  return std::vector<int64_t>(h.begin(), h.end());
}

void car_all_reduce_residual(Tensor x, Tensor resid, Tensor ssp, int64_t rank, std::vector<int64_t> bufs,
                             std::vector<int64_t> sigs, int64_t ctl, int64_t cap_elems) {
  const Op a("all_reduce_residual", x, "x");
  const bf16_t* xp = a.dense<bf16_t>(x, "x", 0, {ANY, ANY}, 16);
  const int rows = a.i32(x.size(0)), hidden = a.i32(x.size(1));
  bf16_t* rp = a.dense<bf16_t>(resid, "resid", 0, {rows, hidden}, 16);
  TORCH_CHECK(hidden % 8 == 0 && rows <= die::CAR_MAX_BLOCKS && (int64_t)rows * hidden <= cap_elems,
              "all_reduce_residual: hidden % 8, rows <= 256 (one flag slot per row), size <= cap");
  float* sp = a.dense<float>(ssp, "ssp", rows);
  const Car c = car_peers(a.op, rank, bufs, sigs, ctl);
  LAUNCH(launch_custom_all_reduce_residual(xp, rp, sp, rows, hidden, c.rank, c.world, c.peers, c.ctl, cap_elems,
                                           cur_stream()));
}

// out [rows, world * cols] = concatenation of every rank's in [rows, cols] along the last dim
void car_all_gather(Tensor in, Tensor out, int64_t rank, std::vector<int64_t> bufs, std::vector<int64_t> sigs,
                    int64_t ctl, int64_t cap_elems, int64_t blocks) {
  const Op a("all_gather", in, "in");
  const bf16_t* ip = a.dense<bf16_t>(in, "in", 0, {ANY, ANY}, 16);
  bf16_t* op = a.dense<bf16_t>(out, "out", 0, {in.size(0), (int64_t)bufs.size() * in.size(1)}, 16);
  TORCH_CHECK(in.size(1) % 8 == 0 && in.numel() <= cap_elems, "all_gather: cols % 8, numel <= cap");
  const Car c = car_peers(a.op, rank, bufs, sigs, ctl);
  LAUNCH(launch_custom_all_gather(ip, op, in.size(0), in.size(1), c.rank, c.world, c.peers, c.ctl, cap_elems,
                                  a.i32(blocks), cur_stream()));
}

void car_all_reduce(Tensor in, Tensor out, int64_t rank, std::vector<int64_t> bufs, std::vector<int64_t> sigs,
                    int64_t ctl, int64_t cap_elems, int64_t blocks) {
  const Op a("all_reduce", in, "in");
  const bf16_t* ip = a.dense<bf16_t>(in, "in", 0, {}, 16);
  bf16_t* op = a.dense<bf16_t>(out, "out", in.numel(), {}, 16);
  TORCH_CHECK(in.numel() == out.numel(), "all_reduce: in/out sizes differ");
  TORCH_CHECK(in.numel() % 8 == 0 && in.numel() <= cap_elems, "all_reduce: numel must be a multiple of 8 <= cap");
  const Car c = car_peers(a.op, rank, bufs, sigs, ctl);
  LAUNCH(launch_custom_all_reduce(ip, op, in.numel(), c.rank, c.world, c.peers, c.ctl, cap_elems, a.i32(blocks),
                                  cur_stream()));
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
  m.def("check_only", &check_only);
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
