// Torch bindings of the W8A16 decode GEMM, its wide (33 to 128 rows) and its grouped (MoE) forms (module `src._C_w8`,
// csrc/kernels/gemm_decode_w8.hip, gemm_decode_w8_wide.hip, gemm_decode_w8_grouped.hip and its _wide). A third module next
// to `_C` and `_C_kv8` with the same rules (bindings.cpp): every argument is validated through the vocabulary of
// arg_check.h before anything is launched on the current stream, and no tensor is asked for its address here.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "arg_check.h"
#include "kernels/gd_w8.h"
#include "kernels/gd_w8_launch.h"
#include "kernels/gd_w8_wide.h"

using torch::Tensor;
using chk::Op;
using die::bf16_t;

namespace {

namespace w8 = die::gd::w8;

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_only(bool on) { chk::g_check_only = on; }

bool tile_exists(int64_t wr, int64_t kc) {
#define GD_W8_TILE(WR, KC) \
  if (wr == WR && kc == KC) return true;
  GD_W8_TILES(GD_W8_TILE)
#undef GD_W8_TILE
  return false;
}

// out: mode 0 bf16 [M, N]; mode 1 bf16 [M, N / 2]; mode 2 fp32 [sk, M, N]. wq: [N, K] e4m3 bytes (uint8 or
// float8_e4m3fn) packed by gd_pack_weights_w8 for (wr, kc); scales: [N] fp32.
void gemm_decode_w8(Tensor out, Tensor x, Tensor wq, Tensor scales, int64_t mode, int64_t wr, int64_t kc, int64_t sk) {
  const Op a("gemm_decode_w8", x, "x");
  const auto xr = a.rows(x, "x");
  const int M = a.i32(x.size(0)), K = a.i32(x.size(1));
  TORCH_CHECK(M <= w8::MAX_M, "gemm_decode_w8: at most ", w8::MAX_M, " rows, got ", M);
  TORCH_CHECK(mode == 0 || mode == 1 || mode == 2, "gemm_decode_w8: mode 0 (bf16), 1 (SiLU) or 2 (slab), got ", mode);
  TORCH_CHECK(tile_exists(wr, kc), "gemm_decode_w8: no W8 tile (", wr, ", ", kc, ")");
  TORCH_CHECK(wq.scalar_type() == at::kByte || wq.scalar_type() == at::kFloat8_e4m3fn,
              "gemm_decode_w8: wq must be uint8 or float8_e4m3fn, got ", wq.scalar_type());
  const uint8_t* wp = static_cast<const uint8_t*>(a.dense<void>(wq, "wq", 0, {chk::ge(1), K}, 16));
  const int N = a.i32(wq.size(0));
  TORCH_CHECK(mode != 1 || N % 2 == 0, "gemm_decode_w8: the SiLU form takes [gate; up], an even row count");
  const int64_t n_out = mode == 1 ? N / 2 : N, cols = mode == 1 ? wr / 2 : wr;
  TORCH_CHECK(K >= kc && K % kc == 0, "gemm_decode_w8: K = ", K, " must be a multiple of kc = ", kc);
  TORCH_CHECK(n_out % cols == 0, "gemm_decode_w8: ", n_out, " output columns are no multiple of the tile's ", cols);
  TORCH_CHECK(sk >= 1 && sk <= K / kc && (mode == 2 || sk == 1), "gemm_decode_w8: sk = ", sk,
              " must be in [1, K / kc] and 1 unless mode 2");
  const float* sp = a.dense<float>(scales, "scales", N, {N}, 16);
  if (mode == 2) {
    float* op = a.dense<float>(out, "out", 0, {sk, M, n_out}, 16);
    LAUNCH(launch_gemm_decode_w8(op, n_out, xr.p, xr.ld, wp, sp, M, N, K, (int)mode, (int)wr, (int)kc, (int)sk,
                                 cur_stream()));
  } else {
    const auto o = a.rows(out, "out", M, n_out);
    LAUNCH(launch_gemm_decode_w8(o.p, o.ld, xr.p, xr.ld, wp, sp, M, N, K, (int)mode, (int)wr, (int)kc, 1,
                                 cur_stream()));
  }
}

// The wide form (gemm_decode_w8_wide.hip): the same arguments, checks and packed bytes on 33 <= M <= 128 rows.
void gemm_decode_w8_wide(Tensor out, Tensor x, Tensor wq, Tensor scales, int64_t mode, int64_t wr, int64_t kc,
                         int64_t sk) {
  const Op a("gemm_decode_w8_wide", x, "x");
  const auto xr = a.rows(x, "x");
  const int M = a.i32(x.size(0)), K = a.i32(x.size(1));
  TORCH_CHECK(M >= w8::wide::MIN_M && M <= w8::wide::MAX_M, "gemm_decode_w8_wide: ", w8::wide::MIN_M, " to ",
              w8::wide::MAX_M, " rows (up to ", w8::MAX_M, ": gemm_decode_w8), got ", M);
  TORCH_CHECK(mode == 0 || mode == 1 || mode == 2, "gemm_decode_w8_wide: mode 0 (bf16), 1 (SiLU) or 2 (slab), got ",
              mode);
  TORCH_CHECK(tile_exists(wr, kc), "gemm_decode_w8_wide: no W8 tile (", wr, ", ", kc, ")");
  TORCH_CHECK(wq.scalar_type() == at::kByte || wq.scalar_type() == at::kFloat8_e4m3fn,
              "gemm_decode_w8_wide: wq must be uint8 or float8_e4m3fn, got ", wq.scalar_type());
  const uint8_t* wp = static_cast<const uint8_t*>(a.dense<void>(wq, "wq", 0, {chk::ge(1), K}, 16));
  const int N = a.i32(wq.size(0));
  TORCH_CHECK(mode != 1 || N % 2 == 0, "gemm_decode_w8_wide: the SiLU form takes [gate; up], an even row count");
  const int64_t n_out = mode == 1 ? N / 2 : N, cols = mode == 1 ? wr / 2 : wr;
  TORCH_CHECK(K >= kc && K % kc == 0, "gemm_decode_w8_wide: K = ", K, " must be a multiple of kc = ", kc);
  TORCH_CHECK(n_out % cols == 0, "gemm_decode_w8_wide: ", n_out, " output columns are no multiple of the tile's ",
              cols);
  TORCH_CHECK(sk >= 1 && sk <= K / kc && (mode == 2 || sk == 1), "gemm_decode_w8_wide: sk = ", sk,
              " must be in [1, K / kc] and 1 unless mode 2");
  const float* sp = a.dense<float>(scales, "scales", N, {N}, 16);
  if (mode == 2) {
    float* op = a.dense<float>(out, "out", 0, {sk, M, n_out}, 16);
    LAUNCH(launch_gemm_decode_w8_wide(op, n_out, xr.p, xr.ld, wp, sp, M, N, K, (int)mode, (int)wr, (int)kc, (int)sk,
                                      cur_stream()));
  } else {
    const auto o = a.rows(out, "out", M, n_out);
    LAUNCH(launch_gemm_decode_w8_wide(o.p, o.ld, xr.p, xr.ld, wp, sp, M, N, K, (int)mode, (int)wr, (int)kc, 1,
                                      cur_stream()));
  }
}

// The grouped (MoE) forms: y [R, N] (mode 1: [R, N / 2]) bf16, group e = rows [offsets[e], offsets[e + 1]) of y, at most
// max_rows of them; wq [E, N, K] e4m3 bytes, each expert packed by gd_pack_weights_w8 for (wr, kc) (mode 1: silu=True);
// scales [E, N] fp32. rows (int32 [R], numel 0 = no gather): x is [T, K] in token order with T k == R and the group's
// row j is x[rows[offsets[e] + j] / k]; without it x is [R, K] in the sorted order. One body of checks for the two
// bindings: WIDE chooses the binding's name, its largest max_rows and its launcher.
template <bool WIDE>
void grouped(Tensor y, Tensor x, Tensor wq, Tensor scales, Tensor offsets, int64_t mode, int64_t wr, int64_t kc,
             Tensor rows, int64_t k, int64_t max_rows) {
  constexpr const char* name = WIDE ? "gemm_decode_w8_grouped_wide" : "gemm_decode_w8_grouped";
  constexpr int limit = WIDE ? w8::wide::MAX_M : w8::MAX_M;
  const Op a(name, x, "x");
  const auto xr = a.rows(x, "x");
  const int T = a.i32(x.size(0)), K = a.i32(x.size(1));
  TORCH_CHECK(mode == 0 || mode == 1, name, ": mode 0 (bf16) or 1 (SiLU), got ", mode);
  TORCH_CHECK(tile_exists(wr, kc), name, ": no W8 tile (", wr, ", ", kc, ")");
  TORCH_CHECK(max_rows >= 1 && max_rows <= limit, name, ": 1 <= max_rows <= ", limit, ", got ", max_rows);
  TORCH_CHECK(wq.scalar_type() == at::kByte || wq.scalar_type() == at::kFloat8_e4m3fn, name,
              ": wq must be uint8 or float8_e4m3fn, got ", wq.scalar_type());
  const uint8_t* wp = static_cast<const uint8_t*>(a.dense<void>(wq, "wq", 0, {chk::ge(1), chk::ge(1), K}, 16));
  const int E = a.i32(wq.size(0)), N = a.i32(wq.size(1));
  TORCH_CHECK(E <= 65535, name, ": at most 65535 groups");
  TORCH_CHECK(mode != 1 || N % 2 == 0, name, ": the SiLU form takes [gate; up], an even row count");
  const int64_t n_out = mode == 1 ? N / 2 : N, cols = mode == 1 ? wr / 2 : wr;
  TORCH_CHECK(K >= kc && K % kc == 0, name, ": K = ", K, " must be a multiple of kc = ", kc);
  TORCH_CHECK(n_out % cols == 0, name, ": ", n_out, " output columns are no multiple of the tile's ", cols);
  const float* sp = a.dense<float>(scales, "scales", (int64_t)E * N, {E, N}, 16);
  const int* op = a.dense<int>(offsets, "offsets", E + 1, {E + 1});
  const auto yr = a.rows(y, "y", chk::ge(1), n_out);
  const int R = a.i32(y.size(0));
  const int* rp = a.dense_opt<int>(rows, "rows", R, {R});
  if (rp) {
    TORCH_CHECK(k >= 1 && (int64_t)T * k == R, name, ": a gather takes rows [T k] and y [T k, N]");
  } else {
    TORCH_CHECK(T == R, name, ": without rows, x and y have the same rows");
  }
  const int kk = rp ? (int)k : 1;
  if constexpr (WIDE)
    LAUNCH(launch_gemm_decode_w8_grouped_wide(yr.p, yr.ld, xr.p, xr.ld, wp, sp, op, rp, kk, E, T, R, N, K, (int)mode,
                                              (int)wr, (int)kc, (int)max_rows, cur_stream()));
  else
    LAUNCH(launch_gemm_decode_w8_grouped(yr.p, yr.ld, xr.p, xr.ld, wp, sp, op, rp, kk, E, T, R, N, K, (int)mode,
                                         (int)wr, (int)kc, (int)max_rows, cur_stream()));
}

// groups of at most max_rows <= 32 rows (gemm_decode_w8_grouped.hip)
void gemm_decode_w8_grouped(Tensor y, Tensor x, Tensor wq, Tensor scales, Tensor offsets, int64_t mode, int64_t wr,
                            int64_t kc, Tensor rows, int64_t k, int64_t max_rows) {
  grouped<false>(y, x, wq, scales, offsets, mode, wr, kc, rows, k, max_rows);
}

// groups of at most max_rows <= 128 rows (gemm_decode_w8_grouped_wide.hip): the same arguments, checks and packed bytes
void gemm_decode_w8_grouped_wide(Tensor y, Tensor x, Tensor wq, Tensor scales, Tensor offsets, int64_t mode, int64_t wr,
                                 int64_t kc, Tensor rows, int64_t k, int64_t max_rows) {
  grouped<true>(y, x, wq, scales, offsets, mode, wr, kc, rows, k, max_rows);
}

int64_t ring_slots(int64_t wr, int64_t kc, int64_t xr) { return w8::ring_slots((int)wr, (int)xr, (int)kc); }

}  // namespace

PYBIND11_MODULE(_C_w8, m) {
  m.doc() = "gfx950 HIP kernels of the W8A16 (FP8 e4m3 weights) decode GEMM, dense and grouped";
  m.def("gemm_decode_w8", &gemm_decode_w8);
  m.def("gemm_decode_w8_wide", &gemm_decode_w8_wide);
  m.def("gemm_decode_w8_grouped", &gemm_decode_w8_grouped);
  m.def("gemm_decode_w8_grouped_wide", &gemm_decode_w8_grouped_wide);
  m.def("ring_slots", &ring_slots);
  m.def("check_only", &check_only);
}
