// Token sampling for gfx950: greedy argmax, temperature, top-k and top-p in
// ONE kernel (one 1024-thread workgroup per sequence), exact and sort-free:
//
//  * top-k / top-p thresholds by 4-pass radix select over order-preserving
//    32-bit keys of the scaled logits (8-bit digit histograms in LDS; counts
//    for top-k, probability mass for top-p) — no sort of the 128K vocabulary;
//  * the draw is Gumbel-max, argmax(z_i + G_i) over the kept set with
//    G_i = -log(-log(u_i)), u from a counter-based hash of
//    (request seed, generation step, token id): reproducible per request and
//    independent of batch composition, and needs no prefix sum. u is one of the
//    2^23 values (h + 0.5) * 2^-23 (rng_hash.h), never 0 and never 1, so G_i is
//    finite (-2.82 .. 16.64) and no token wins on noise alone.
// Contract of the filters (tests/sampling_reference.py is its float64 oracle,
// tests/test_sampling_kernel_gpu.py compares draw by draw): zz = z * (1 / t) in
// fp32; top-k keeps every zz >= the k-th largest (ties kept; k <= 0 or >= vocab
// keeps all); top-p keeps the value levels, from the top, whose mass WITHIN the
// top-k set first reaches p (whole levels, at least the top one); the floor is
// the higher of the two. Drawn tokens depend on the uniform's mapping: they are
// reproducible per build of this file, not across changes to rng_hash.h.
// Rows stream from L2 (a 128256-entry bf16 row is 250 KiB), 16 B per lane.
#include "common.h"
#include "launchers.h"

namespace die {

constexpr int SNT = 1024;

__device__ __forceinline__ uint32_t f2key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}

struct ArgMax {
  float v;
  int i;
};
__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) {
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

__device__ ArgMax block_argmax(ArgMax x, ArgMax* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ArgMax y;
    y.v = __shfl_xor(x.v, o, 64);
    y.i = __shfl_xor(x.i, o, 64);
    x = better(x, y);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = x;
  __syncthreads();
  ArgMax r = red[0];
  for (int w = 1; w < SNT / 64; ++w) r = better(r, red[w]);
  __syncthreads();
  return r;
}

__device__ float block_sumf(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = v;
  __syncthreads();
  float t = 0.f;
  for (int w = 0; w < SNT / 64; ++w) t += red[w];
  __syncthreads();
  return t;
}

// Radix-select the threshold key. MASS=false: the k-th largest key among
// keys >= floor_key (target = k). MASS=true: the largest key t such that the
// probability mass of {z >= t, z >= floor} reaches `target` (weights exp(z - m)).
template <bool MASS>
__device__ uint32_t radix_threshold(const bf16_t* row, int vocab, float inv_t, float m, uint32_t floor_key,
                                    float target, float* hist, uint32_t* sh) {
  uint32_t prefix = 0, pmask = 0;
  float remaining = target;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int b = threadIdx.x; b < 256; b += SNT) hist[b] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x * 8; i < vocab; i += SNT * 8) {
      float z[8];
      unpack8(*reinterpret_cast<const uint4*>(row + i), z);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float zz = z[j] * inv_t;
        const uint32_t k = f2key(zz);
        if (k >= floor_key && (k & pmask) == prefix)
          atomicAdd(&hist[(k >> shift) & 255u], MASS ? __expf(zz - m) : 1.f);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float cum = 0.f;
      int b = 255;
      for (; b > 0; --b) {
        if (cum + hist[b] >= remaining) break;
        cum += hist[b];
      }
      sh[0] = (uint32_t)b;
      reinterpret_cast<float*>(sh)[1] = remaining - cum;
    }
    __syncthreads();
    prefix |= sh[0] << shift;
    pmask |= 255u << shift;
    remaining = reinterpret_cast<float*>(sh)[1];
    __syncthreads();
  }
  return prefix;
}

// argmax over row[lo, hi) (lo a multiple of 8): AU 16-B loads per lane in flight at once instead of one
// dependent round trip per 16 KiB of the row
__device__ __forceinline__ ArgMax row_argmax(const bf16_t* row, int lo, int hi, ArgMax* red) {
  constexpr int AU = 8;
  ArgMax best{-INFINITY, 0x7fffffff};
  for (int i0 = lo + threadIdx.x * 8; i0 < hi; i0 += SNT * 8 * AU) {
    uint4 v[AU];
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int i = i0 + u * SNT * 8;
      v[u] = i < hi ? *reinterpret_cast<const uint4*>(row + i) : make_uint4(0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u);
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      float z[8];
      unpack8(v[u], z);
      const int i = i0 + u * SNT * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) best = better(best, ArgMax{z[j], i + j});
    }
  }
  return block_argmax(best, red);
}

// grid = (rows, splits). splits > 1: a GREEDY row is cut into `splits` slices, one workgroup each (a decode
// step's 32 rows then use 256 CUs instead of 32: the argmax is bound by the CUs that read the row); each
// slice's (max, index) goes to part[r][split] with write-through stores and the slice's last arriver (agent-
// scope ticket cnt[r], re-armed) picks the row's winner — MI355X_MICROARCH.md inter-workgroup table, first
// row. A sampled (non-greedy) row is handled whole by split 0, the others exit.
// Argument order: the file is built with kernarg preload (the first 14 argument dwords arrive in SGPRs with the
// wave), so what is read before the first load of a candidate or a logit comes first; the outputs, the draw's
// seeds and the advance follow.
__global__ void __launch_bounds__(SNT) sample_kernel(const float* __restrict__ temperature,
                                                     const int* __restrict__ top_k, const float* __restrict__ top_p,
                                                     const uint32_t* __restrict__ lm_part, int lm_parts, int vocab,
                                                     const bf16_t* __restrict__ logits, int64_t stride,
                                                     int64_t* __restrict__ out, const int64_t* __restrict__ seeds,
                                                     const int64_t* __restrict__ steps, uint32_t* __restrict__ part,
                                                     int* __restrict__ cnt, SampleAdvance adv) {
  __shared__ ArgMax red[SNT / 64];
  __shared__ float redf[SNT / 64];
  __shared__ float hist[256];
  __shared__ uint32_t sh[2];
  const int r = blockIdx.x, splits = gridDim.y, sp = blockIdx.y;
  const bf16_t* row = logits + (int64_t)r * stride;
  // thread 0: out[r] = t and (adv.ids) this row's share of the step's input advance (decode_advance_kernel)
  __shared__ int64_t s_next;  // the row's next input id (for the embedding below)
  auto finish = [&](int64_t t) {
    out[r] = t;
    if (adv.ids == nullptr) return;
    const int k = __hip_atomic_load(adv.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int n = adv.n_real[0];
    s_next = r < n ? t : adv.ids[r];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // k is read before this row's ticket below
    if (k < adv.k_max) adv.tokens[(int64_t)k * adv.tok_stride + r] = t;
    if (r < n) {
      adv.ids[r] = t;
      const int64_t p = adv.pos[r] + 1;
      adv.pos[r] = p;
      adv.ctx[r] += 1;
      const int b = (int)(p / adv.bs);
      adv.slots[r] = b < adv.bt_width ? (int64_t)adv.bt[(int64_t)r * adv.bt_width + b] * adv.bs + p % adv.bs : -1;
      adv.step[r] += 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (__hip_atomic_fetch_add(adv.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
      __hip_atomic_store(adv.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(adv.cnt, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  // every thread, after finish(): the next step's embedding row and its sum of squares, exactly as embed_sumsq
  // (the first 256 threads, the same chunk walk and reduction order, so the values are bit-identical)
  __shared__ float ered[4];
  auto embed_next = [&]() {
    if (adv.table == nullptr) return;  // uniform
    __syncthreads();                   // s_next
    float ss = 0.f;
    if (threadIdx.x < 256) {
      const int64_t id = s_next;
      const uint4* src = reinterpret_cast<const uint4*>(adv.table + id * adv.hidden);
      uint4* dst = reinterpret_cast<uint4*>(adv.h_out + (int64_t)r * adv.hidden);
      for (int c = threadIdx.x; c < (adv.hidden >> 3); c += 256) {
        const uint4 u = src[c];
        dst[c] = u;
        float v[8];
        unpack8(u, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 256) ered[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) adv.ssp_out[r] = ered[0] + ered[1] + ered[2] + ered[3];
  };
  const float temp = temperature ? temperature[r] : 0.f;
  const int k = top_k ? top_k[r] : 0;
  const float p = top_p ? top_p[r] : 1.f;
  const bool greedy = temp <= 0.f || k == 1;

  if (lm_part != nullptr && greedy) {
    // the LM head wrote each column tile's (max, lowest column) of this row (gemm_decode mode 0 with fz.amax):
    // reduce lm_parts candidates (8 B each) instead of re-reading the 128K-entry row
    if (sp != 0) return;
    ArgMax best{-INFINITY, 0x7fffffff};
    const uint32_t* pr = lm_part + (int64_t)r * lm_parts * 2;
    for (int i = threadIdx.x; i < lm_parts; i += SNT) {
      const uint2 c = *reinterpret_cast<const uint2*>(pr + 2 * i);
      best = better(best, ArgMax{__uint_as_float(c.x), (int)c.y});
    }
    best = block_argmax(best, red);
    if (threadIdx.x == 0) finish(best.i < vocab ? best.i : 0);
    embed_next();
    return;
  }
  if (splits > 1) {
    if (!greedy && sp != 0) return;
    if (greedy) {
      const int per = ((vocab / 8 + splits - 1) / splits) * 8;
      const int lo = min(vocab, sp * per), hi = min(vocab, lo + per);
      const ArgMax b = row_argmax(row, lo, hi, red);
      __shared__ int is_last;
      if (threadIdx.x == 0) {
        uint32_t* pr = part + ((int64_t)r * splits + sp) * 2;
        __hip_atomic_store(pr, __float_as_uint(b.v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pr + 1, (uint32_t)b.i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        is_last = __hip_atomic_fetch_add(cnt + r, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == splits - 1;
      }
      __syncthreads();
      if (!is_last || threadIdx.x >= 64) return;
      // last arriver: lane q loads slice q's (max, index) — every slice in ONE round trip (a loop over the slices
      // in one lane waited for each agent-scope load in turn: ~11 us for 8 slices) — reduced in the wave;
      // better() is a total order (value, then lowest index), so the result does not depend on the order
      const int lane = threadIdx.x;
      ArgMax w{-INFINITY, 0x7fffffff};
      if (lane < splits) {
        const uint32_t* pq = part + ((int64_t)r * splits + lane) * 2;
        w = ArgMax{__uint_as_float(__hip_atomic_load(pq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)),
                   (int)__hip_atomic_load(pq + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)};
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        ArgMax y;
        y.v = __shfl_xor(w.v, o, 64);
        y.i = __shfl_xor(w.i, o, 64);
        w = better(w, y);
      }
      if (lane == 0) {
        out[r] = w.i < vocab ? w.i : 0;
        __hip_atomic_store(cnt + r, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      return;
    }
  }
  ArgMax best = row_argmax(row, 0, vocab, red);
  // an all-NaN / all -inf row (e.g. a padded graph row over uninitialised KV) still yields a
  // valid token id: an out-of-range id would turn into an out-of-bounds embedding read next step
  if (best.i >= vocab) best.i = 0;
  if (greedy) {
    if (threadIdx.x == 0) finish(best.i);
    embed_next();
    return;
  }
  const float inv_t = 1.f / temp;
  const float m = best.v * inv_t;
  uint32_t floor_key = 0;
  if (k > 0 && k < vocab) floor_key = radix_threshold<false>(row, vocab, inv_t, m, 0u, (float)k, hist, sh);
  if (p < 1.f) {
    float z_mass = 0.f;
    for (int i = threadIdx.x * 8; i < vocab; i += SNT * 8) {
      float z[8];
      unpack8(*reinterpret_cast<const uint4*>(row + i), z);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float zz = z[j] * inv_t;
        if (f2key(zz) >= floor_key) z_mass += __expf(zz - m);
      }
    }
    z_mass = block_sumf(z_mass, redf);
    const uint32_t pk = radix_threshold<true>(row, vocab, inv_t, m, floor_key, p * z_mass, hist, sh);
    floor_key = pk > floor_key ? pk : floor_key;
  }
  const uint64_t seed = seeds ? (uint64_t)seeds[r] : 0x5eedull;
  const uint64_t step = steps ? (uint64_t)steps[r] : 0ull;
  ArgMax g{-INFINITY, 0x7fffffff};
  for (int i = threadIdx.x * 8; i < vocab; i += SNT * 8) {
    float z[8];
    unpack8(*reinterpret_cast<const uint4*>(row + i), z);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float zz = z[j] * inv_t;
      if (f2key(zz) >= floor_key) {
        const float u = hash_uniform(seed, step, (uint64_t)(i + j));
        g = better(g, ArgMax{zz - __logf(-__logf(u)), i + j});
      }
    }
  }
  g = block_argmax(g, red);
  if (threadIdx.x == 0) finish(g.i < vocab ? g.i : best.i);
  embed_next();
}

hipError_t launch_sample(int64_t* out, const bf16_t* logits, int64_t stride, int rows, int vocab,
                         const float* temperature, const int* top_k, const float* top_p, const int64_t* seeds,
                         const int64_t* steps, hipStream_t s, uint32_t* part, int* cnt, int splits,
                         const uint32_t* lm_part, int lm_parts, const SampleAdvance& adv) {
  if (rows == 0) return hipSuccess;
  if (vocab % 8 || splits < 1 || splits > SAMPLE_MAX_SPLITS || (splits > 1 && (part == nullptr || cnt == nullptr)))
    return hipErrorInvalidValue;
  if (lm_part != nullptr && lm_parts < 1) return hipErrorInvalidValue;
  // the advance rides on one workgroup per row: only with the LM head's candidates (no split argmax)
  if (adv.ids != nullptr && (lm_part == nullptr || adv.cnt == nullptr || adv.ticket == nullptr || adv.n_real == nullptr))
    return hipErrorInvalidValue;
  // the embedding gather reads the advanced id: it needs the advance and its outputs
  if (adv.table != nullptr &&
      (adv.ids == nullptr || adv.h_out == nullptr || adv.ssp_out == nullptr || adv.hidden <= 0 || adv.hidden % 8))
    return hipErrorInvalidValue;
  // with the LM head's candidates a greedy row is one short reduction: no split (a sampled row is whole anyway)
  if (lm_part != nullptr) splits = 1;
  hipLaunchKernelGGL(sample_kernel, dim3(rows, splits), dim3(SNT), 0, s, temperature, top_k, top_p, lm_part, lm_parts,
                     vocab, logits, stride, out, seeds, steps, part, cnt, adv);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Per-token log-probabilities of the RAW distribution (log_softmax of the bf16 row in fp32, before temperature
// and filters): the target's logprob and rank and the top_n most likely tokens, one workgroup per row.
// Total order: larger logit first, then lower token id (better()). Passes over the row (from L2):
//   1. row max (row_argmax);  2. sum of exp(z - max) and the count of entries before the target — and, for
//      top_n > 0, a histogram of the entries whose key is among the 256 bf16 values just below the max's (a bf16
//      entry's 32-bit key is fixed by its upper 16 bits, so this window is two octaves of logit values);
//   3. the key T of the top_n-th largest entry: a wave's prefix scan over that window — no pass over the row.
//      Only when the window holds fewer than top_n entries (e.g. one outlier above a flat row) does
//      radix_threshold<false> find T in four more passes;
//   4. one walk with contiguous slabs per wave: entries above T go to an LDS list (fewer than top_n), entries
//      equal to T are numbered in index order inside each wave (prefix scan of the lanes' counts); the places
//      left go to the waves' ties in wave order;  5. wave 0 ranks the top_n entries among themselves.
// Every id written is an index the walk visited (or the slot number, if a row of NaN keys yields fewer
// entries than asked), so it is inside [0, vocab) whatever the row holds.

// f2key with -0.0 == +0.0, as a float compare (and the sort of the reference) has it
__device__ __forceinline__ uint32_t lp_key(float f) {
  return f2key(__float_as_uint(f) == 0x80000000u ? 0.f : f);
}

__device__ int block_sumi(int v, int* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = v;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < SNT / 64; ++w) t += red[w];
  __syncthreads();
  return t;
}

__global__ void __launch_bounds__(SNT) token_logprobs_kernel(float* __restrict__ lp, int* __restrict__ rank,
                                                             float* __restrict__ top_lp, int* __restrict__ top_id,
                                                             int64_t top_stride, const bf16_t* __restrict__ logits,
                                                             int64_t stride, int vocab,
                                                             const int64_t* __restrict__ targets, int top_n) {
  constexpr int NW = SNT / 64;
  __shared__ ArgMax red[NW];
  __shared__ float redf[NW];
  __shared__ int redi[NW];
  __shared__ float hist[256];
  __shared__ uint32_t sh[2];
  __shared__ uint32_t whist[256];  // entries per 16-bit key, from the max's key downwards
  __shared__ uint32_t l_key[LOGPROBS_MAX_TOP];  // entries above the threshold, unordered
  __shared__ int l_id[LOGPROBS_MAX_TOP];
  __shared__ int n_above;
  __shared__ int w_tie[NW][LOGPROBS_MAX_TOP];   // each wave's first ties, in index order
  __shared__ int w_ntie[NW];
  const int r = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bf16_t* row = logits + (int64_t)r * stride;
  const int64_t t64 = targets[r];
  const bool t_ok = t64 >= 0 && t64 < vocab;
  const int ti = t_ok ? (int)t64 : 0;
  const float zt = t_ok ? bf2f(row[ti]) : 0.f;
  const uint32_t kt = lp_key(zt);

  if (threadIdx.x < 256) whist[threadIdx.x] = 0u;  // row_argmax's barrier orders this before the adds below
  const float m = row_argmax(row, 0, vocab, red).v;
  const uint32_t kmax16 = lp_key(m) >> 16;

  constexpr int AU = 4;
  float s = 0.f;
  int before = 0;
  for (int i0 = threadIdx.x * 8; i0 < vocab; i0 += SNT * 8 * AU) {
    uint4 v[AU];
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int i = i0 + u * SNT * 8;
      v[u] = i < vocab ? *reinterpret_cast<const uint4*>(row + i) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int i = i0 + u * SNT * 8;
      if (i < vocab) {
        float z[8];
        unpack8(v[u], z);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s += __expf(z[j] - m);
          const uint32_t k = lp_key(z[j]);
          before += (k > kt || (k == kt && i + j < ti)) ? 1 : 0;
          const uint32_t d = kmax16 - (k >> 16);  // wraps to a large value for a (NaN) key above the max's
          if (top_n > 0 && d < 256u) atomicAdd(&whist[d], 1u);
        }
      }
    }
  }
  s = block_sumf(s, redf);
  before = block_sumi(before, redi);
  const float lse = logf(s);
  if (threadIdx.x == 0) {
    lp[r] = t_ok ? (zt - m) - lse : -INFINITY;
    rank[r] = t_ok ? before : vocab;
  }
  if (top_n <= 0) return;

  // wave 0: lane l sums window bins [4l, 4l + 4), a prefix scan finds the bin that holds the top_n-th entry
  if (wid == 0) {
    uint32_t c4[4], mine = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      c4[q] = whist[lane * 4 + q];
      mine += c4[q];
    }
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    uint32_t cum = incl - mine;
    if (lane == 63 && incl < (uint32_t)top_n) sh[0] = 0xffffffffu;
    if (cum < (uint32_t)top_n && incl >= (uint32_t)top_n) {  // exactly one lane
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (cum < (uint32_t)top_n && cum + c4[q] >= (uint32_t)top_n) sh[0] = (uint32_t)(lane * 4 + q);
        cum += c4[q];
      }
    }
  }
  __syncthreads();
  const uint32_t bin = sh[0];
  __syncthreads();  // sh is reused by radix_threshold
  uint32_t T;
  if (bin != 0xffffffffu) {
    const uint32_t t16 = kmax16 - bin;  // a bf16 entry's key: its upper 16 bits, then all zeros (>= 0) or all ones
    T = (t16 << 16) | ((t16 & 0x8000u) ? 0u : 0xffffu);
  } else {
    T = radix_threshold<false>(row, vocab, 1.f, m, 0u, (float)top_n, hist, sh);
    if (T == 0x7fffffffu) T = 0x80000000u;  // the key of -0.0: lp_key() files those under +0.0
  }
  if (threadIdx.x < LOGPROBS_MAX_TOP) {
    l_key[threadIdx.x] = 0u;
    l_id[threadIdx.x] = threadIdx.x < vocab ? threadIdx.x : 0;
  }
  if (threadIdx.x < NW) w_ntie[threadIdx.x] = 0;
  if (threadIdx.x == 0) n_above = 0;
  __syncthreads();

  // wave `wid` owns row[lo, hi): its ties are met in index order (chunk by chunk, lane by lane, entry by entry)
  const int slab = ((vocab / 8 + NW - 1) / NW) * 8;
  const int lo = min(vocab, wid * slab), hi = min(vocab, lo + slab);
  int c = 0;  // this wave's ties so far (wave-uniform)
  for (int i0 = lo; i0 < hi; i0 += 512 * AU) {
    uint4 v[AU];
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int i = i0 + u * 512 + lane * 8;
      v[u] = i < hi ? *reinterpret_cast<const uint4*>(row + i) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < AU; ++u) {
      const int i = i0 + u * 512 + lane * 8;
      uint32_t tie = 0u;
      if (i < hi) {
        float z[8];
        unpack8(v[u], z);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t k = lp_key(z[j]);
          if (k > T) {
            const int slot = atomicAdd(&n_above, 1);
            if (slot < LOGPROBS_MAX_TOP) {
              l_key[slot] = k;
              l_id[slot] = i + j;
            }
          }
          tie |= (k == T ? 1u : 0u) << j;
        }
      }
      if (c < top_n && __ballot(tie != 0u) != 0ull) {  // wave-uniform
        const int cnt = __popc(tie);
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int y = __shfl_up(incl, o, 64);
          if (lane >= o) incl += y;
        }
        int ord = c + incl - cnt;
        for (int j = 0; j < 8; ++j) {
          if ((tie >> j) & 1u) {
            if (ord < LOGPROBS_MAX_TOP) w_tie[wid][ord] = i + j;
            ++ord;
          }
        }
        c += __shfl(incl, 63, 64);
      }
    }
  }
  if (lane == 0) w_ntie[wid] = min(c, LOGPROBS_MAX_TOP);
  __syncthreads();
  if (wid != 0) return;

  const int above = min(n_above, top_n);
  uint32_t key = 0u;
  int id = lane < vocab ? lane : 0;
  if (lane < above) {
    key = l_key[lane];
    id = l_id[lane];
  } else if (lane < top_n) {
    int q = lane - above;
    for (int w = 0; w < NW; ++w) {
      const int nw = w_ntie[w];
      if (q < nw) {
        key = T;
        id = w_tie[w][q];
        break;
      }
      q -= nw;
    }
  }
  // place = the number of entries that come before this one (the lane breaks a tie of equal pairs, which only a
  // short-filled list can hold, so the places are always a permutation)
  int place = 0;
  for (int o = 0; o < top_n; ++o) {
    const uint32_t ko = __shfl(key, o, 64);
    const int io = __shfl(id, o, 64);
    place += (ko > key || (ko == key && (io < id || (io == id && o < lane)))) ? 1 : 0;
  }
  if (lane < top_n) {
    top_lp[(int64_t)r * top_stride + place] = (key2f(key) - m) - lse;
    top_id[(int64_t)r * top_stride + place] = id;
  }
}

hipError_t launch_token_logprobs(float* lp, int* rank, float* top_lp, int* top_id, int64_t top_stride,
                                 const bf16_t* logits, int64_t stride, int rows, int vocab, const int64_t* targets,
                                 int top_n, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  if (rows < 0 || vocab <= 0 || vocab % 8 || stride < vocab || stride % 8 || top_n < 0 || top_n > LOGPROBS_MAX_TOP ||
      top_n > vocab || lp == nullptr || rank == nullptr || targets == nullptr || logits == nullptr)
    return hipErrorInvalidValue;
  if (top_n > 0 && (top_lp == nullptr || top_id == nullptr || top_stride < top_n)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(token_logprobs_kernel, dim3(rows), dim3(SNT), 0, s, lp, rank, top_lp, top_id, top_stride, logits,
                     stride, vocab, targets, top_n);
  return hipGetLastError();
}

}  // namespace die
