// Grouped (MoE) W4A16 decode GEMM on OCP MXFP4 weights for steps of up to 128 tokens: for every expert e with rows in
// this step
//   Y[off[e] : off[e + 1], :] = Xrows · dequant(q[e])^T
// Operands, packed expert images (gd_pack_experts_w4, GD_W4_TILES, gd_w4.h's record order), gather through rows / k,
// index clamping and the two epilogues are gemm_decode_w4_grouped.hip's: the very bytes that serve steps of up to 32
// tokens serve these, with no second copy and no re-layout. That kernel holds a group in a 16- or 32-row image; a step
// of 33 to 128 tokens can route up to 128 rows to one expert. What is this kernel's own is the row image chosen per
// group at run time, out of four, and the wide body that reads a K-split record without splitting K.
//
// Grid. (N_out / NO, 1, E), 256 threads, one workgroup per CU. Workgroup (bx, e) owns WR image rows of expert e over
// all of K and reads its own M = off[e + 1] - off[e], clamped to [0, 128] and to R. M == 0: it returns before it
// issues any DMA. Then a wave-uniform branch between four instantiations:
//   M <= 16, M <= 32   gd_w4_grouped_dev.h's K-split body, unchanged: a slot is a whole chunk (256 columns), the four
//                      waves split its K, every wave holds every accumulator, the partials meet in LDS.
//   M <= 64, M <= 128  the wide body below, on gd_w4_wide.h's geometry.
//
// The wide body. gd_w4.h's record was laid out for four waves that split K: nibbles [w][step][p][lane] x 16 B, then
// scales [w][fr][nt][step]. With 64 or 128 activation rows a whole-chunk slot no longer fits (the X image alone is
// 64 KiB at 128 rows), and a K-split would keep every accumulator in every wave. So:
//   * A ring slot is HALF a chunk (128 columns): the record's waves w in {2 h, 2 h + 1}. Both parts of the record are
//     in ascending w, so the half's nibbles are the WR * 64 contiguous bytes at h * WR * 64 and its scales the 4 WR
//     contiguous bytes at chunk_bytes + h * 4 WR. A slot in LDS is [nibbles WR * 64][scale area 1 KiB][X image
//     XR x 256 B]; an activation row's sixteen 16-byte chunks are XOR-ed with row & 15 on the DMA source address and
//     on the read, as in the wide W8 kernel. A slot's weight and scale sources advance by REC per chunk and by a
//     constant per half, both worked out once per lane before the ring is primed.
//   * The four waves split the OUTPUT tile, 2 column groups x 2 row groups, and every wave runs all four k-steps of a
//     slot (w' x step): no cross-wave reduction. Wave (cg, rg) holds WR / 32 column tiles x XR / 32 row tiles, at most
//     4 x 4 accumulators, which leave through the padded fp32 stage[XR][WR + 4] that reuses the ring.
//       WR = 128: a wave's four tiles are exactly tile group p = cg, one ds_read_b128 per k-step.
//       WR = 64: the only 16-byte group holds all four tiles of the workgroup. The two options were two column groups
//       that each use half of it (an 8-byte read at lane * 16 + cg * 8) or one column group and four row groups. The
//       second makes every wave convert every B fragment: 16 v_cvt_scalef32_pk_bf16_fp4 per wave and k-step for 8
//       MFMAs, where the first has 8 for 8 and the same split as WR = 128 (one body, one stage layout). The first is
//       built; the second was not, so there is no resource report to compare.
//   * Fragment build unchanged: v_cvt_scalef32_pk_bf16_fp4 with the block scale as its operand, 2^e as byte << 23.
//     The scales are in the products; the epilogue has no scale pass.
//   * Scales. The counted wait needs every wave to issue the same number of vector-memory instructions per slot. The
//     half's 4 WR scale bytes are brought by one 4-byte-per-lane global_load_lds per wave: wave v fetches quarter v
//     (WR bytes) into its own 256-byte area, lanes past WR / 4 repeating earlier dwords into the area's slack. So
//     per_wave = pieces / 4 + 1 for every form. Within a half the order is still [w'][fr][nt][step]: lane (fr, cg)
//     finds the scales of its tiles for one w' as one run of 2 * tiles bytes (gd_w4_wide.h scale_read: quarter
//     2 w' + fr / 8), two small LDS reads per slot; lanes of equal fr read the same address, a broadcast.
//
// Slot sizes, ring depths (gd_w4_wide.h asserts them) and the weight bytes in flight per CU, (S - 1) slots of
// nibbles + scales:
//   (128, 128 rows)  41 KiB  3 slots  11 instructions per wave and slot   17 KiB in flight
//   (128,  64 rows)  25 KiB  5 slots   7                                  34 KiB
//   ( 64, 128 rows)  37 KiB  3 slots  10                                   8.5 KiB
//   ( 64,  64 rows)  21 KiB  6 slots   6                                  21.25 KiB
// The known weak spot: a 128-row slot is four fifths activations, which come from L2, and the weight stream in flight
// is shallow. Measured at (128, 256) on Mixtral-8x7B's experts (docs/performance.md): 3.2 / 3.0 TB/s of packed bytes
// at 64 tokens (gate/up / down; groups in the 16- and 32-row bodies), 2.4 / 1.7 TB/s at 128 tokens (32- and 64-row
// bodies), where the 32-row kernel moves 3.5 / 3.45 at 32 tokens. A 64-column grain (a quarter chunk: 7 slots at
// (128, 128 rows)) is the obvious follow-up; it is not built.
#include "common.h"
#include "gd_w4.h"
#include "gd_w4_grouped_dev.h"
#include "gd_w4_launch.h"
#include "gd_w4_wide.h"

namespace die {
namespace gd {
namespace w4 {
namespace wide {

template <int WR, int XR, int EPI>
__device__ __forceinline__ void grouped_body_wide(const Group& g, char* smem) {
  static_assert(valid(WR, XR), "a gd_w4_wide.h form");
  constexpr int S = ring_slots(WR, XR);
  constexpr int WIMG = wimg_bytes(WR);        // bytes of the nibble sub-image in a slot
  constexpr int REC = record_bytes(WR, KC);   // bytes of a chunk in memory: nibble image, then scales
  constexpr int XOFF = WIMG + SCALE_LDS;      // the X image in a slot
  constexpr int SLOT = slot_bytes(WR, XR);
  constexpr int XROWB = GRAIN * 2;            // bytes per activation row of a slot: sixteen 16-byte chunks
  constexpr int WPIECES = WIMG / 1024;
  constexpr int PER_WAVE = per_wave(WR, XR);  // vector-memory instructions a wave issues per slot
  constexpr int PW = PER_WAVE - 1;            // of them 1-KiB pieces
  constexpr int CG = COL_GROUPS, RG = 4 / CG;
  constexpr int NTW = tiles_per_wave(WR);     // a wave's 16-column MFMA tiles: 4 (a whole 16-byte group) or 2 (half)
  constexpr int MTW = XR / 16 / RG;           // a wave's 16-row MFMA tiles
  constexpr int SQ = scale_quarter(WR);       // scale bytes a wave brings per slot
  constexpr bool SILU = EPI == 1;
  constexpr int NO = SILU ? WR / 2 : WR;      // output columns per workgroup
  static_assert((S - 1) * PER_WAVE <= 63 && S >= 3 && S <= MAX_SLOTS, "vmcnt field is 6 bits");
  static_assert(WPIECES % 4 == 0, "a wave's piece p is a weight piece or an activation piece for all 4 waves");
  static_assert((NTW == 4 && WR == 128) || (NTW == 2 && WR == 64), "a wave's tiles: group cg, or half cg of group 0");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cg = wave % CG, rg = wave / CG;
  const int bx = blockIdx.x, M = g.M;
  const int n0 = bx * NO;
  const int tch = g.K / KC;
  const int nsl = 2 * tch;  // slots of the group: two per chunk

  // per-lane source of this wave's pieces q = wave + 4 p of slot 0, as byte pointers. Slot h = 2 c + hh: weights and
  // scales step by REC per chunk c and by WIMG / 4 WR per half hh; activations by GRAIN elements per slot. An
  // activation piece holds four image rows, gathered here, once: image row j <- token rows[r0 + j] / k, or sorted row
  // r0 + j
  const char* tile0 = reinterpret_cast<const char*>(g.Wq) + (int64_t)bx * tch * REC;
  const char* src[PW];
#pragma unroll
  for (int p = 0; p < PW; ++p) {
    const int q = wave + 4 * p;
    if (4 * p < WPIECES) {
      src[p] = tile0 + q * 1024 + lane * 16;
    } else {
      const int row = 4 * (q - WPIECES) + lane / 16;
      const int lch = (lane % 16) ^ (row & 15);
      const int j = min(row, M - 1);
      const int xrow = g.rows != nullptr ? min(max(g.rows[j] / g.k, 0), g.T - 1) : g.r0 + j;
      src[p] = reinterpret_cast<const char*>(g.X + (int64_t)xrow * g.ldx + lch * 8);
    }
  }
  // the wave's quarter of a half's scales: SQ bytes, 4 per lane (lanes past SQ / 4 repeat earlier dwords)
  const char* ssrc = tile0 + scale_src(WR, 0) + wave * SQ + (lane % (SQ / 4)) * 4;
  auto issue = [&](int h) {
    char* slot = smem + (h % S) * SLOT;
    const int64_t c = h >> 1;
    const int hh = h & 1;
#pragma unroll
    for (int p = 0; p < PW; ++p) {
      if (4 * p < WPIECES)
        glds16<2>(src[p] + c * REC + hh * WIMG, slot + (wave + 4 * p) * 1024);  // non-temporal
      else
        glds16<0>(src[p] + (int64_t)h * XROWB, slot + XOFF + (wave + 4 * p - WPIECES) * 1024);
    }
    glds4(ssrc + c * REC + hh * scale_bytes(WR), slot + WIMG + wave * 256);
  };

  f4 acc[MTW][NTW];
#pragma unroll
  for (int a = 0; a < MTW; ++a)
#pragma unroll
    for (int b = 0; b < NTW; ++b) acc[a][b] = f4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int h = 0; h < S - 1; ++h)
    if (h < nsl) issue(h);

  const int fr = lane & 15, kg = lane >> 4;
  // the lane's B fragments of a k-step: its group's 16 bytes, or its half of them
  const int boff = NTW == 4 ? read_off(WR, 0, cg, lane) : read_off(WR, 0, 0, lane) + cg * 8;
  const int soff = scale_read(WR, 0, fr, cg * NTW);
#pragma unroll 1
  for (int h = 0; h < nsl; ++h) {
    if (h + S - 1 < nsl) issue(h + S - 1);
    wait_chunk<S, PER_WAVE>(min(S - 1, nsl - 1 - h));  // the slots issued after h stay in flight
    __builtin_amdgcn_s_barrier();  // every wave's pieces of slot h have landed
    const char* slot = smem + (h % S) * SLOT;
    const char* ximg = slot + XOFF;
#pragma unroll
    for (int wp = 0; wp < 2; ++wp) {
      uint32_t sc[NTW / 2];  // the lane's scale bytes of (slot, w'): byte 2 i + step of its tile i
      const char* sp = slot + WIMG + soff + (scale_read(WR, 1, 0, 0) - scale_read(WR, 0, 0, 0)) * wp;
      if constexpr (NTW == 4) {
        const uint2 v = *reinterpret_cast<const uint2*>(sp);
        sc[0] = v.x, sc[1] = v.y;
      } else {
        sc[0] = *reinterpret_cast<const uint32_t*>(sp);
      }
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const int ks = 2 * wp + st;   // the slot's k-step
        const int lch = 4 * ks + kg;  // the lane's 16-byte chunk of an activation row
        bf16x8 a[MTW], b[NTW];
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) {
          const int r = 16 * (rg * MTW + mt) + fr;
          a[mt] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(ximg + r * XROWB + 16 * (lch ^ (r & 15))));
        }
        uint32_t d[NTW];
        if constexpr (NTW == 4) {
          const uint4 v = *reinterpret_cast<const uint4*>(slot + boff + read_off(WR, ks, 0, 0));
          d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
          const uint2 v = *reinterpret_cast<const uint2*>(slot + boff + read_off(WR, ks, 0, 0));
          d[0] = v.x, d[1] = v.y;
        }
#pragma unroll
        for (int i = 0; i < NTW; ++i) b[i] = cvt8(d[i], e8m0(sc[i / 2], 2 * (i & 1) + st));
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // slot h % S is refilled by the next iteration's issue
  }

  // the waves' tiles into stage[XR][LD] fp32 (every DMA has landed and every read is done)
  constexpr int LD = stage_ld(WR);
  float* stage = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)  // C: column lane & 15, row 4 (lane >> 4) + r
        stage[(16 * (rg * MTW + mt) + 4 * kg + r) * LD + 16 * (cg * NTW + nt) + fr] = acc[mt][nt][r];
  __syncthreads();

  // four output columns per thread, then the epilogue (the scales are in the products)
  constexpr int Q = NO / 4;
  for (int e = tid; e < XR * Q; e += NTH) {
    const int m = e / Q, j = 4 * (e % Q);
    if (m >= M) continue;
    f4 v = *reinterpret_cast<const f4*>(stage + m * LD + j);
    if constexpr (SILU) {
      const f4 u = *reinterpret_cast<const f4*>(stage + m * LD + NO + j);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = silu_mul(v[i], u[i]);
    }
    uint2 o;
    o.x = pack2(v[0], v[1]);
    o.y = pack2(v[2], v[3]);
    *reinterpret_cast<uint2*>(g.Y + (int64_t)m * g.ldy + n0 + j) = o;
  }
}

// off [E + 1]: group e's rows; rows [R] or null; T rows of X, R rows of Y
template <int WR, int KC_, int EPI>
__global__ void __launch_bounds__(NTH) gemm_decode_w4_grouped_wide_kernel(const uint8_t* __restrict__ Wq,
                                                                          const bf16_t* __restrict__ X, int64_t ldx,
                                                                          bf16_t* __restrict__ Y, int64_t ldy,
                                                                          const int* __restrict__ off,
                                                                          const int* __restrict__ rows, int k, int T,
                                                                          int R, int N_out, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int e = blockIdx.z;
  const int r0 = min(max(off[e], 0), R);
  const int M = min(min(off[e + 1], R) - r0, MAX_M);
  if (M <= 0) return;  // an idle expert: no DMA was issued
  const int64_t img_rows = EPI == 1 ? 2 * (int64_t)N_out : N_out;
  Group g;
  g.Wq = Wq + (int64_t)e * img_rows * row_bytes(K);
  g.X = X;
  g.Y = Y + (int64_t)r0 * ldy;
  g.rows = rows != nullptr ? rows + r0 : nullptr;
  g.ldx = ldx;
  g.ldy = ldy;
  g.r0 = r0;
  g.M = M;
  g.k = k;
  g.T = T;
  g.K = K;
  if (M <= 16)
    w4::grouped_body<WR, KC_, 16, EPI>(g, smem);
  else if (M <= w4::MAX_M)
    w4::grouped_body<WR, KC_, 32, EPI>(g, smem);
  else if (M <= 64)
    grouped_body_wide<WR, 64, EPI>(g, smem);
  else
    grouped_body_wide<WR, 128, EPI>(g, smem);
}

constexpr size_t max2(size_t a, size_t b) { return a > b ? a : b; }

template <int WR, int KC_, int EPI>
static hipError_t launch_grouped(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                 const int* off, const int* rows, int k, int E, int T, int R, int N_out, int K,
                                 hipStream_t s) {
  static_assert(KC_ == KC && w4::valid(WR, 16, KC_) && w4::valid(WR, 32, KC_) && valid(WR, 64) && valid(WR, 128),
                "GD_W4_TILES lists tiles with all four images");
  constexpr int NO = EPI == 1 ? WR / 2 : WR;
  if (N_out % NO || K % KC || K < KC) return hipErrorInvalidValue;
  // all four bodies live in the kernel: the launch asks for the largest ring
  constexpr size_t lds = max2(max2(w4::lds_bytes(WR, 16, KC_), w4::lds_bytes(WR, 32, KC_)),
                              max2(lds_bytes(WR, 64), lds_bytes(WR, 128)));
  static_assert(lds <= RING_BYTES, "one workgroup per CU");
  const dim3 grid(N_out / NO, 1, E);
  hipLaunchKernelGGL((gemm_decode_w4_grouped_wide_kernel<WR, KC_, EPI>), grid, dim3(NTH), lds, s, Wq, X, ldx, Y, ldy,
                     off, rows, k, T, R, N_out, K);
  return hipGetLastError();
}

}  // namespace wide
}  // namespace w4
}  // namespace gd

hipError_t launch_gemm_decode_w4_grouped_wide(bf16_t* Y, int64_t ldy, const bf16_t* X, int64_t ldx, const uint8_t* Wq,
                                              const int* offsets, const int* rows, int k, int E, int T, int R, int N,
                                              int K, int mode, int wr, int kc, int max_rows, hipStream_t s) {
  using namespace gd::w4::wide;
  if (max_rows < 1 || max_rows > MAX_M || E < 1 || E > 65535 || T < 1 || R < 1 || N <= 0 || K <= 0 ||
      (mode != 0 && mode != 1) || (mode == 1 && N % 2) || (rows != nullptr && k < 1))
    return hipErrorInvalidValue;
  const int n_out = mode == 1 ? N / 2 : N;
#define GD_W4_TILE(WR, KC_)                                                                                     \
  if (wr == WR && kc == KC_) {                                                                                  \
    if (mode == 0) return launch_grouped<WR, KC_, 0>(Y, ldy, X, ldx, Wq, offsets, rows, k, E, T, R, n_out, K, s); \
    return launch_grouped<WR, KC_, 1>(Y, ldy, X, ldx, Wq, offsets, rows, k, E, T, R, n_out, K, s);              \
  }
  GD_W4_TILES(GD_W4_TILE)
#undef GD_W4_TILE
  return hipErrorInvalidValue;
}

}  // namespace die
