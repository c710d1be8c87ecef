// Torch bindings of the grouped (MoE) W4A16 decode GEMM on MXFP4 weights and its wide (33 to 128 rows) form (module
// `src._C_w4`, csrc/kernels/gemm_decode_w4_grouped.hip and its _wide). A module of its own next to `_C`, `_C_kv8` and `_C_w8` with the same rules
// (bindings.cpp): every argument is validated through the vocabulary of arg_check.h before anything is launched on the
// current stream, and no tensor is asked for its address here.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "arg_check.h"
#include "kernels/gd_w4.h"
#include "kernels/gd_w4_launch.h"
#include "kernels/gd_w4_wide.h"

using torch::Tensor;
using chk::Op;

namespace {

namespace w4 = die::gd::w4;

inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_only(bool on) { chk::g_check_only = on; }

bool tile_exists(int64_t wr, int64_t kc) {
#define GD_W4_TILE(WR, KC) \
  if (wr == WR && kc == KC) return true;
  GD_W4_TILES(GD_W4_TILE)
#undef GD_W4_TILE
  return false;
}

// y [R, N] (mode 1: [R, N / 2]) bf16, group e = rows [offsets[e], offsets[e + 1]) of y, at most max_rows of them;
// wq [E, N, K / 2 + K / 32] uint8, each expert's codes and scale bytes packed by gd_pack_experts_w4 for (wr, kc) (mode 1:
// silu=True). rows (int32 [R], numel 0 = no gather): x is [T, K] in token order with T k == R and the group's row j is
// x[rows[offsets[e] + j] / k]; without it x is [R, K] in the sorted order.
template <bool WIDE>
void grouped(Tensor y, Tensor x, Tensor wq, Tensor offsets, int64_t mode, int64_t wr, int64_t kc, Tensor rows,
             int64_t k, int64_t max_rows) {
  constexpr const char* name = WIDE ? "gemm_decode_w4_grouped_wide" : "gemm_decode_w4_grouped";
  constexpr int max_m = WIDE ? w4::wide::MAX_M : w4::MAX_M;
  const Op a(name, x, "x");
  const auto xr = a.rows(x, "x");
  const int T = a.i32(x.size(0)), K = a.i32(x.size(1));
  TORCH_CHECK(mode == 0 || mode == 1, name, ": mode 0 (bf16) or 1 (SiLU), got ", mode);
  TORCH_CHECK(tile_exists(wr, kc), name, ": no W4 tile (", wr, ", ", kc, ")");
  TORCH_CHECK(max_rows >= 1 && max_rows <= max_m, name, ": 1 <= max_rows <= ", max_m, ", got ", max_rows);
  TORCH_CHECK(K >= kc && K % kc == 0, name, ": K = ", K, " must be a multiple of kc = ", kc);
  const uint8_t* wp = a.dense<uint8_t>(wq, "wq", 0, {chk::ge(1), chk::ge(1), w4::row_bytes(K)}, 16);
  const int E = a.i32(wq.size(0)), N = a.i32(wq.size(1));
  TORCH_CHECK(E <= 65535, name, ": at most 65535 groups");
  TORCH_CHECK(mode != 1 || N % 2 == 0, name, ": the SiLU form takes [gate; up], an even row count");
  const int64_t n_out = mode == 1 ? N / 2 : N, cols = mode == 1 ? wr / 2 : wr;
  TORCH_CHECK(n_out % cols == 0, name, ": ", n_out, " output columns are no multiple of the tile's ", cols);
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
  if constexpr (WIDE) {
    LAUNCH(launch_gemm_decode_w4_grouped_wide(yr.p, yr.ld, xr.p, xr.ld, wp, op, rp, kk, E, T, R, N, K, (int)mode,
                                              (int)wr, (int)kc, (int)max_rows, cur_stream()));
  } else {
    LAUNCH(launch_gemm_decode_w4_grouped(yr.p, yr.ld, xr.p, xr.ld, wp, op, rp, kk, E, T, R, N, K, (int)mode, (int)wr,
                                         (int)kc, (int)max_rows, cur_stream()));
  }
}

// groups of at most max_rows <= 32 rows (gemm_decode_w4_grouped.hip)
void gemm_decode_w4_grouped(Tensor y, Tensor x, Tensor wq, Tensor offsets, int64_t mode, int64_t wr, int64_t kc,
                            Tensor rows, int64_t k, int64_t max_rows) {
  grouped<false>(y, x, wq, offsets, mode, wr, kc, rows, k, max_rows);
}

// groups of at most max_rows <= 128 rows (gemm_decode_w4_grouped_wide.hip): the same arguments, checks and packed bytes
void gemm_decode_w4_grouped_wide(Tensor y, Tensor x, Tensor wq, Tensor offsets, int64_t mode, int64_t wr, int64_t kc,
                                 Tensor rows, int64_t k, int64_t max_rows) {
  grouped<true>(y, x, wq, offsets, mode, wr, kc, rows, k, max_rows);
}

int64_t ring_slots(int64_t wr, int64_t kc, int64_t xr) { return w4::ring_slots((int)wr, (int)xr, (int)kc); }
int64_t ring_slots_wide(int64_t wr, int64_t xr) { return w4::wide::ring_slots((int)wr, (int)xr); }

}  // namespace

PYBIND11_MODULE(_C_w4, m) {
  m.doc() = "gfx950 HIP kernels of the grouped W4A16 (MXFP4 weights) decode GEMM";
  m.def("gemm_decode_w4_grouped", &gemm_decode_w4_grouped);
  m.def("gemm_decode_w4_grouped_wide", &gemm_decode_w4_grouped_wide);
  m.def("ring_slots", &ring_slots);
  m.def("ring_slots_wide", &ring_slots_wide);
  m.def("check_only", &check_only);
}
