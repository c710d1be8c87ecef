// Torch binding of the grouped (MoE) W4A16 decode GEMM on MXFP4 weights (module `src._C_w4`,
// csrc/kernels/gemm_decode_w4_grouped.hip). A module of its own next to `_C`, `_C_kv8` and `_C_w8` with the same rules
// (bindings.cpp): every argument is validated through the vocabulary of arg_check.h before anything is launched on the
// current stream, and no tensor is asked for its address here.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "arg_check.h"
#include "kernels/gd_w4.h"
#include "kernels/gd_w4_launch.h"

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

// y [R, N] (mode 1: [R, N / 2]) bf16, group e = rows [offsets[e], offsets[e + 1]) of y, at most max_rows <= 32 of them;
// wq [E, N, K / 2 + K / 32] uint8, each expert's codes and scale bytes packed by gd_pack_experts_w4 for (wr, kc) (mode 1:
// silu=True). rows (int32 [R], numel 0 = no gather): x is [T, K] in token order with T k == R and the group's row j is
// x[rows[offsets[e] + j] / k]; without it x is [R, K] in the sorted order.
void gemm_decode_w4_grouped(Tensor y, Tensor x, Tensor wq, Tensor offsets, int64_t mode, int64_t wr, int64_t kc,
                            Tensor rows, int64_t k, int64_t max_rows) {
  constexpr const char* name = "gemm_decode_w4_grouped";
  const Op a(name, x, "x");
  const auto xr = a.rows(x, "x");
  const int T = a.i32(x.size(0)), K = a.i32(x.size(1));
  TORCH_CHECK(mode == 0 || mode == 1, name, ": mode 0 (bf16) or 1 (SiLU), got ", mode);
  TORCH_CHECK(tile_exists(wr, kc), name, ": no W4 tile (", wr, ", ", kc, ")");
  TORCH_CHECK(max_rows >= 1 && max_rows <= w4::MAX_M, name, ": 1 <= max_rows <= ", w4::MAX_M, ", got ", max_rows);
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
  LAUNCH(launch_gemm_decode_w4_grouped(yr.p, yr.ld, xr.p, xr.ld, wp, op, rp, rp ? (int)k : 1, E, T, R, N, K, (int)mode,
                                       (int)wr, (int)kc, (int)max_rows, cur_stream()));
}

int64_t ring_slots(int64_t wr, int64_t kc, int64_t xr) { return w4::ring_slots((int)wr, (int)xr, (int)kc); }

}  // namespace

PYBIND11_MODULE(_C_w4, m) {
  m.doc() = "gfx950 HIP kernel of the grouped W4A16 (MXFP4 weights) decode GEMM";
  m.def("gemm_decode_w4_grouped", &gemm_decode_w4_grouped);
  m.def("ring_slots", &ring_slots);
  m.def("check_only", &check_only);
}
