// Constrained decoding for gfx950: a step's bf16 logits rows are masked IN PLACE to the tokens a per-sequence token
// automaton allows next (src/guided.py compiles allowed_token_ids / guided_choice / guided_regex to it), before the
// sampler reads them. One 1024-thread workgroup per batch row, in logit_process.hip's idiom; row r maps through
// slot_of_row[r] (< 0, or beyond the table: the workgroup exits at once and the row's bytes stay as they are).
// Per-slot device tables:
//   * desc[slot] = (state_base, n_states, edge_base, n_edges): offsets into two arenas shared by all slots,
//     rowptr (int32; the automaton's CSR row pointers, n_states + 1 of them from state_base, relative to
//     edge_base) and edges ((tok, next) int32 pairs);
//   * cur[slot]: the automaton's current state;  err[slot]: sticky error bits.
// Contract (tests/token_guide_reference.py is the oracle; tests/test_token_guide_kernel_gpu.py compares bit for
// bit):
//   1. advance_ids != nullptr: advance_ids[r] is this step's INPUT token (the previous step's sample); the state
//      becomes next(cur, tok), found by one thread per edge over the state's edge range (tokens are unique within
//      a state). No such edge: err |= GUIDE_ERR_NO_EDGE and the state is kept.
//   2. The (new) state's edge tokens become a bitmap in LDS (vocab / 8 bytes, one BYTE per 16-B group). Both edge
//      loops keep TG_EU loads per lane in flight.
//   3. One dense pass (guide_common.h's guide_mask_row): a barred entry becomes bf16 -inf (0xFF80), an allowed entry
//      keeps its exact bits. A group with no allowed entry is stored without being loaded, a group with all eight
//      allowed is not stored.
//   4. lm_part != nullptr: the row's LM-head candidates are rewritten by the same pass (guide_common.h's
//      write_best_candidate): candidate 0 = the best ALLOWED entry in better()'s order (sampling.hip), the others
//      (-inf, 0x7fffffff).
//   5. Every index is checked against its descriptor and every descriptor against the arena sizes BEFORE use: a
//      descriptor outside its arena, a state outside [0, n_states), a row pointer outside [0, n_edges] or
//      descending, a next state outside [0, n_states), an edge token outside [0, vocab): err |= GUIDE_ERR_TABLE,
//      the row, the candidates and cur stay untouched. No table content leads to an out-of-range access.
// A slot belongs to one row of a launch (the runner maps one sequence to one slot), so cur / err have one writer.
// Rows stream 16 B per lane: at most one load and one store per group, 500 KiB per 128256-entry row.
#include "guide_common.h"

namespace die {

constexpr int TG_EU = 8;  // edges per lane in flight in the two edge loops

__global__ void __launch_bounds__(GUIDE_T) token_guide_kernel(bf16_t* __restrict__ logits, int64_t stride, int vocab,
                                                              const int* __restrict__ slot_of_row, int num_slots,
                                                              const int4* __restrict__ desc,
                                                              const int* __restrict__ rowptr, int rowptr_len,
                                                              const int2* __restrict__ edges, int edges_len,
                                                              int* __restrict__ cur, int* __restrict__ err,
                                                              const int64_t* __restrict__ advance_ids,
                                                              uint32_t* __restrict__ lm_part, int lm_parts) {
  extern __shared__ uint32_t s_map[];  // bit t: token t is allowed
  __shared__ int s_hit, s_next, s_bad;
  const int r = blockIdx.x;
  const int slot = slot_of_row[r];
  if (slot < 0 || slot >= num_slots) return;  // uniform
  const int4 d = desc[slot];
  const int state_base = d.x, n_states = d.y, edge_base = d.z, n_edges = d.w;
  int c = cur[slot];
  // everything below is uniform across the workgroup: all threads read the same words
  bool bad = state_base < 0 || n_states < 1 || (int64_t)state_base + n_states + 1 > (int64_t)rowptr_len ||
             edge_base < 0 || n_edges < 0 || (int64_t)edge_base + n_edges > (int64_t)edges_len || c < 0 ||
             c >= n_states;
  if (bad) {
    if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
    return;
  }
  const int* rp = rowptr + state_base;
  const int2* ed = edges + edge_base;
  int flags = 0;
  if (advance_ids != nullptr) {
    const int64_t tok = advance_ids[r];
    const int lo = rp[c], hi = rp[c + 1];
    if (lo < 0 || hi < lo || hi > n_edges) {
      if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
      return;
    }
    if (threadIdx.x == 0) s_hit = 0;
    __syncthreads();
    for (int e0 = lo + threadIdx.x; e0 < hi; e0 += GUIDE_T * TG_EU) {
      int2 ev[TG_EU];
#pragma unroll
      for (int u = 0; u < TG_EU; ++u) {
        const int e = e0 + u * GUIDE_T;
        if (e < hi) ev[u] = ed[e];
      }
#pragma unroll
      for (int u = 0; u < TG_EU; ++u) {
        // unique within a state by contract; were it not, one of the writers wins
        if (e0 + u * GUIDE_T < hi && (int64_t)ev[u].x == tok) {
          s_next = ev[u].y;
          s_hit = 1;
        }
      }
    }
    __syncthreads();
    if (s_hit) {
      const int nx = s_next;
      if (nx < 0 || nx >= n_states) {
        if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
        return;
      }
      c = nx;
    } else {
      flags = GUIDE_ERR_NO_EDGE;
    }
  }
  const int lo = rp[c], hi = rp[c + 1];
  if (lo < 0 || hi < lo || hi > n_edges) {
    if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
    return;
  }
  const int words = (vocab / 8 + 3) / 4;
  for (int w = threadIdx.x; w < words; w += GUIDE_T) s_map[w] = 0u;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  // Tokens ascend within a state, so the lanes of a wave that hit one bitmap word are neighbours: a segmented OR
  // over the wave (doubling shuffles) leaves one LDS atomic per word and wave instead of up to 32 on one address
  // (a full-vocabulary state took 114 us per launch at 32 rows with one atomic per edge, 89 us this way). A list
  // that does not ascend only makes more segments: every bit still reaches a segment head. What remains is the
  // shuffles' own LDS throughput, 13 per 64 edges (running the TG_EU chains level by level changed nothing, and a
  // single row costs the same as 32): a state with n edges adds about n / 1500 us. Next step, not taken here:
  // stage the tokens through LDS so that a lane combines 8 consecutive edges in registers, without shuffles.
  const int lane = threadIdx.x & 63;
  for (int e0 = lo; e0 < hi; e0 += GUIDE_T * TG_EU) {  // uniform trip count: the shuffles need every lane
    int tk[TG_EU];
#pragma unroll
    for (int u = 0; u < TG_EU; ++u) {
      const int e = e0 + u * GUIDE_T + (int)threadIdx.x;
      if (e < hi) tk[u] = ed[e].x;
    }
#pragma unroll
    for (int u = 0; u < TG_EU; ++u) {
      if (e0 + u * GUIDE_T >= hi) break;  // uniform
      const int e = e0 + u * GUIDE_T + (int)threadIdx.x;
      uint32_t w = 0x80000000u | (uint32_t)lane, b = 0u;  // no edge, or a bad one: a word of its own, no bit
      if (e < hi) {
        const int t = tk[u];
        if (t < 0 || t >= vocab) {
          s_bad = 1;
        } else {
          w = (uint32_t)t >> 5;
          b = 1u << (t & 31);
        }
      }
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t ow = __shfl_down(w, off, 64), ob = __shfl_down(b, off, 64);
        if (lane + off < 64 && ow == w) b |= ob;
      }
      const uint32_t pw = __shfl_up(w, 1, 64);
      if (b != 0u && (lane == 0 || pw != w)) atomicOr(&s_map[w], b);  // b != 0: t is in [0, vocab), w in the map
    }
  }
  __syncthreads();
  if (s_bad) {
    if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
    return;
  }
  if (threadIdx.x == 0) {
    cur[slot] = c;
    if (flags) err[slot] |= flags;
  }
  guide_mask_row<GUIDE_T>(logits + (int64_t)r * stride, vocab, s_map,
                          lm_part != nullptr ? lm_part + (int64_t)r * lm_parts * 2 : nullptr, lm_parts);
}

hipError_t launch_token_guide(bf16_t* logits, int64_t stride, int rows, int vocab, const int* slot, int num_slots,
                              const int* desc, const int* rowptr, int64_t rowptr_len, const int* edges,
                              int64_t edges_len, int* cur, int* err, const int64_t* advance_ids, uint32_t* lm_part,
                              int lm_parts, hipStream_t s) {
  int map_words;
  if (!guide_row_args_ok(vocab, stride, rows, num_slots, lm_part, lm_parts, &map_words)) return hipErrorInvalidValue;
  if (logits == nullptr || slot == nullptr || desc == nullptr || rowptr == nullptr || edges == nullptr ||
      cur == nullptr || err == nullptr)
    return hipErrorInvalidValue;
  if (rowptr_len < 2 || rowptr_len > GUIDE_ROWPTR_ARENA || edges_len < 1 || edges_len > GUIDE_EDGE_ARENA)
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(token_guide_kernel, dim3(rows), dim3(GUIDE_T), map_words * 4, s, logits, stride, vocab, slot,
                     num_slots, reinterpret_cast<const int4*>(desc), rowptr, (int)rowptr_len,
                     reinterpret_cast<const int2*>(edges), (int)edges_len, cur, err, advance_ids, lm_part, lm_parts);
  return hipGetLastError();
}

}  // namespace die
