// Embedding pooling for gfx950: the final-norm hidden rows [T, H] (bf16) of a prefill step are pooled per request
// segment into fp32 vectors, one launch for all segments of the step. grid = (segments, max parts), 1024 threads.
// Segment descriptor (8 int32, device): (first row, row count, accumulator slot, total prompt length, flags,
// part base, parts, 0), flags = POOL_MEAN (else the last row) | POOL_FIRST | POOL_FINAL.
// Contract (tests/pool_embed_reference.py is the oracle):
//   * last: v = the segment's last row as fp32 (no other row of the segment is read);
//   * mean: s = (FIRST ? 0 : acc[slot]) + sum of the rows in fp32. A non-FINAL segment stores s to acc[slot] and
//     writes nothing to out; a FINAL one takes v = s / total (IEEE fp32 division);
//   * v is cut to its first D = (dims ? dims : H) components; only out[seg, :D] (and acc[slot, :D]) is written and
//     only those columns of hidden are read;
//   * normalize: v / max(||v||_2, 1e-12) (torch.nn.functional.normalize: a zero vector stays zero).
// A descriptor that does not fit the tensors (rows outside [0, T), a slot outside [0, slots), total < 1, parts
// beyond the grid or the scratch) makes its workgroups exit before any access: out / acc / tickets keep what they
// held. Rows outside every segment are never read.
// Work split inside a workgroup: thread = one 16-byte column group; while H / 8 < 1024 the idle threads form up
// to PL_MAX_RG row groups (row r of the part belongs to group r % R), combined through LDS in group order. Every
// lane keeps PL_U row loads in flight.
// Row split (mean segments with parts > 1; one workgroup reads ~90 GB/s, so an 8,192-row segment alone took 0.72
// ms at H = 4096): part p of a segment sums rows [p * ceil(rows / parts), ...) and writes its fp32 partial to
// part[part base + p] with write-through stores; the segment's last arriver (agent-scope ticket tickets[segment],
// re-armed for the next launch) reads ALL partials back past the L1 in part order 0, 1, ... and finishes. Which
// workgroup arrives last does not change a bit of the result; there are no float atomics.
// The norm is a wave shuffle + LDS block reduction; the unnormalised vector is parked in out by the thread that
// scales it afterwards.
#include "common.h"
#include "launchers.h"

namespace die {

constexpr int PLT = 1024;
constexpr int PL_U = 8;        // 16-byte row loads in flight per lane
constexpr int PL_MAX_RG = 16;  // row groups when H / 8 < PLT: bounds the serial LDS combine
constexpr int PL_PU = 4;       // partials in flight per lane in the last arriver's combine

typedef __attribute__((ext_vector_type(4))) unsigned pl_u4;

__device__ __forceinline__ void pl_add(float* a, const float4& lo, const float4& hi) {
  a[0] += lo.x, a[1] += lo.y, a[2] += lo.z, a[3] += lo.w;
  a[4] += hi.x, a[5] += hi.y, a[6] += hi.z, a[7] += hi.w;
}

__global__ void __launch_bounds__(PLT) pool_embed_kernel(const bf16_t* __restrict__ hidden, int64_t stride, int T, int H,
                                                         const int* __restrict__ segs, float* __restrict__ acc,
                                                         int slots, float* __restrict__ out, int D, int normalize,
                                                         float* part, int part_cap, int* tickets) {
  extern __shared__ __attribute__((aligned(16))) float4 s_part[];  // [R][vd][2] row-group partials (R > 1)
  __shared__ float red[PLT / 64];
  __shared__ int s_last;
  const int seg = blockIdx.x, p = blockIdx.y;
  const int* ds = segs + (int64_t)seg * 8;
  const int first = ds[0], count = ds[1], slot = ds[2], total = ds[3], flags = ds[4], pbase = ds[5];
  const bool mean = flags & POOL_MEAN, is_first = flags & POOL_FIRST, fin = !mean || (flags & POOL_FINAL);
  const int np = mean && ds[6] > 1 ? ds[6] : 1;
  // uniform: every thread of every workgroup of the segment read the same words
  if (first < 0 || count < 1 || (int64_t)first + count > (int64_t)T) return;
  if (mean && (slot < 0 || slot >= slots || total < 1)) return;
  if (np > (int)gridDim.y) return;
  if (np > 1 && (part == nullptr || tickets == nullptr || pbase < 0 || (int64_t)pbase + np > (int64_t)part_cap)) return;
  if (p >= np) return;
  const int vd = D / 8;  // column groups that are read and written
  const int R = vd >= PLT ? 1 : min(PLT / vd, PL_MAX_RG);
  // this part's rows [r_lo, r_lo + r_n); last pooling: the one-row segment [first + count - 1, first + count)
  const int chunk = (count + np - 1) / np;
  const int r_lo = mean ? first + p * chunk : first + count - 1;
  const int r_n = mean ? max(0, min(chunk, count - p * chunk)) : 1;
  const int g = R > 1 ? (int)threadIdx.x / vd : 0, c = R > 1 ? (int)threadIdx.x % vd : (int)threadIdx.x;
  // the fp32 partials of this segment: byte offsets below stay under parts * H * 4 (the launcher bounds it)
  __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(np > 1 ? part + (int64_t)pbase * H : part, 0,
                                                                0x7fffffff, 0x00020000);
  float ss = 0.f;

  // s -> acc[slot] (not FINAL), or s / total -> out[seg] and its squares into ss
  auto finish = [&](int col, float* a) {
    if (mean) {
      float4* ap = reinterpret_cast<float4*>(acc + (int64_t)slot * H + (int64_t)col * 8);
      if (!is_first) pl_add(a, ap[0], ap[1]);
      if (!fin) {
        ap[0] = make_float4(a[0], a[1], a[2], a[3]);
        ap[1] = make_float4(a[4], a[5], a[6], a[7]);
        return;
      }
      const float n = (float)total;
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = __fdiv_rn(a[j], n);
    }
    float4* op = reinterpret_cast<float4*>(out + (int64_t)seg * H + (int64_t)col * 8);
    op[0] = make_float4(a[0], a[1], a[2], a[3]);
    op[1] = make_float4(a[4], a[5], a[6], a[7]);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += a[j] * a[j];
  };

  for (int col0 = 0; col0 < vd; col0 += PLT) {  // uniform trip count; one pass when R > 1
    const int col = col0 + c;
    const bool live = col < vd && g < R;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
      const bf16_t* base = hidden + (int64_t)r_lo * stride + (int64_t)col * 8;
      for (int r = g; r < r_n; r += R * PL_U) {
        uint4 v[PL_U];
#pragma unroll
        for (int u = 0; u < PL_U; ++u) {
          const int rr = r + u * R;
          if (rr < r_n) v[u] = *reinterpret_cast<const uint4*>(base + (int64_t)rr * stride);
        }
#pragma unroll
        for (int u = 0; u < PL_U; ++u) {
          if (r + u * R < r_n) {
            float f[8];
            unpack8(v[u], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] += f[j];
          }
        }
      }
    }
    if (R > 1) {  // uniform
      if (live) {
        s_part[((int64_t)g * vd + c) * 2] = make_float4(a[0], a[1], a[2], a[3]);
        s_part[((int64_t)g * vd + c) * 2 + 1] = make_float4(a[4], a[5], a[6], a[7]);
      }
      __syncthreads();
      if (live && g == 0)
        for (int q = 1; q < R; ++q)  // group order: fixed
          pl_add(a, s_part[((int64_t)q * vd + c) * 2], s_part[((int64_t)q * vd + c) * 2 + 1]);
    }
    if (live && g == 0) {
      if (np == 1) {
        finish(col, a);
      } else {  // write-through (sc1): no release fence
        const int o = (int)(((int64_t)p * H + (int64_t)col * 8) * 4);
        __builtin_amdgcn_raw_buffer_store_b128(
            pl_u4{__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]), __float_as_uint(a[3])}, rp, o, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b128(
            pl_u4{__float_as_uint(a[4]), __float_as_uint(a[5]), __float_as_uint(a[6]), __float_as_uint(a[7])}, rp, o + 16,
            0, 16);
      }
    }
  }

  if (np > 1) {  // uniform
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's partial stores are acknowledged
    __syncthreads();
    if (threadIdx.x == 0)
      s_last = __hip_atomic_fetch_add(tickets + seg, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == np - 1;
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) __hip_atomic_store(tickets + seg, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // last arriver: every part's partial (its own too: one order for everybody), sc1 loads past this CU's L1
    for (int col = threadIdx.x; col < vd; col += PLT) {
      float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int q0 = 0; q0 < np; q0 += PL_PU) {
        pl_u4 lo[PL_PU], hi[PL_PU];
#pragma unroll
        for (int u = 0; u < PL_PU; ++u) {
          if (q0 + u < np) {
            const int o = (int)(((int64_t)(q0 + u) * H + (int64_t)col * 8) * 4);
            lo[u] = __builtin_amdgcn_raw_buffer_load_b128(rp, o, 0, 16);
            hi[u] = __builtin_amdgcn_raw_buffer_load_b128(rp, o + 16, 0, 16);
          }
        }
#pragma unroll
        for (int u = 0; u < PL_PU; ++u) {
          if (q0 + u < np)
            pl_add(a, __builtin_bit_cast(float4, lo[u]), __builtin_bit_cast(float4, hi[u]));
        }
      }
      finish(col, a);
    }
  }

  if (!fin || !normalize) return;  // uniform
  ss = block_sum<PLT>(ss, red);
  const float den = fmaxf(__fsqrt_rn(ss), 1e-12f);
  for (int col = threadIdx.x; col < vd; col += PLT) {  // the columns this thread wrote above
    float4* op = reinterpret_cast<float4*>(out + (int64_t)seg * H + (int64_t)col * 8);
    float4 lo = op[0], hi = op[1];
    lo.x = __fdiv_rn(lo.x, den), lo.y = __fdiv_rn(lo.y, den), lo.z = __fdiv_rn(lo.z, den), lo.w = __fdiv_rn(lo.w, den);
    hi.x = __fdiv_rn(hi.x, den), hi.y = __fdiv_rn(hi.y, den), hi.z = __fdiv_rn(hi.z, den), hi.w = __fdiv_rn(hi.w, den);
    op[0] = lo;
    op[1] = hi;
  }
}

hipError_t launch_pool_embed(float* out, float* acc, int slots, const bf16_t* hidden, int64_t stride, int T, int H,
                             const int* segs, int num_segs, int dims, bool normalize, float* part, int part_cap,
                             int* tickets, int ticket_cap, int max_parts, hipStream_t s) {
  if (H <= 0 || H % 8 || T < 0 || num_segs < 0 || slots < 0) return hipErrorInvalidValue;
  if (stride < H || stride % 8) return hipErrorInvalidValue;
  if (dims < 0 || dims % 8 || dims > H) return hipErrorInvalidValue;
  if (hidden == nullptr || segs == nullptr || out == nullptr || (slots > 0 && acc == nullptr))
    return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(hidden) % 16 || reinterpret_cast<uintptr_t>(out) % 16 ||
      reinterpret_cast<uintptr_t>(acc) % 16 || reinterpret_cast<uintptr_t>(part) % 16)
    return hipErrorInvalidValue;
  if (max_parts < 1 || max_parts > POOL_MAX_PARTS || part_cap < 0 || ticket_cap < 0) return hipErrorInvalidValue;
  if (max_parts > 1 && (part == nullptr || tickets == nullptr || part_cap < 2 || ticket_cap < num_segs))
    return hipErrorInvalidValue;
  if ((int64_t)POOL_MAX_PARTS * H * 4 > 0x7fffffffLL) return hipErrorInvalidValue;  // 32-bit partial offsets
  if (num_segs == 0) return hipSuccess;
  const int D = dims ? dims : H, vd = D / 8;
  const int R = vd >= PLT ? 1 : (PLT / vd < PL_MAX_RG ? PLT / vd : PL_MAX_RG);
  const size_t lds = R > 1 ? (size_t)R * vd * 32 : 0;  // <= PLT * 32 = 32 KiB
  hipLaunchKernelGGL(pool_embed_kernel, dim3(num_segs, max_parts), dim3(PLT), lds, s, hidden, stride, T, H, segs, acc,
                     slots, out, D, normalize ? 1 : 0, max_parts > 1 ? part : nullptr, part_cap,
                     max_parts > 1 ? tickets : nullptr);
  return hipGetLastError();
}

}  // namespace die
