// JSON mode for gfx950: a step's bf16 logits rows are masked IN PLACE to the tokens whose BYTES a byte PUSHDOWN
// automaton can still read (src/guided.py compiles guided_json_object to a JsonGuide; JSON nests, so byte_guide.hip's
// DFA cannot hold it). byte_guide.hip's idiom: one 1024-thread workgroup per batch row; row r maps through
// slot_of_row[r] (< 0, or beyond the table: the workgroup exits at once and the row's bytes stay as they are).
// Device tables:
//   * the vocabulary's bytes, byte_guide's own tensors: tok_off int32 [n_tok + 1], tok_bytes uint8 [bytes_len];
//   * trans int16 [table_states, 256], one table for all slots, uploaded once. An entry is -1 (no transition) or
//       bits 0..7  the next state            bits 8..9  the action: 0 none, 1 push-object, 2 push-array, 3 pop
//     and nothing above bit 9. A push at depth GUIDE_JSON_MAX_DEPTH is no transition. A pop clears the top and lands
//     on (state field) + 0 when the new top is an object, + 1 when it is an array, + 2 at depth 0: the builder puts
//     "after a value in an object", "after a value in an array" and DONE there, in this order;
//   * desc[slot] = (n_states, done, eos, 0): DONE is the only accepting state; state n_states is a virtual SINK,
//     entered by EOS from DONE, only EOS is legal in it and keeps it (windows run past a finished sequence);
//   * cur[slot] / err[slot]: the arrays token_guide and byte_guide use; jstk int32 [slots, 2] = (depth, stack bits):
//     bit d - 1 is the kind (0 object, 1 array) of the container at depth d. A slot belongs to one sequence, so
//     every entry keeps one writer.
// Contract (tests/json_guide_reference.py is the oracle; tests/test_json_guide_kernel_gpu.py compares bit for bit):
//   1. advance_ids != nullptr: the configuration (state, depth, stack) first advances over advance_ids[r], this
//      step's INPUT token. EOS: DONE or the sink go to the sink, any other state err |= GUIDE_ERR_NO_EDGE. Any other
//      token walks its bytes with pushes and pops applied; a dead transition, a push at the cap, a token with no
//      bytes, beyond the table or the vocabulary, or over GUIDE_MAX_TOKEN_BYTES, and any non-EOS token in the sink:
//      err |= GUIDE_ERR_NO_EDGE. The configuration is kept in every such case.
//   2. Token t is allowed next: in the sink only EOS; else EOS iff the state is DONE; else iff t < min(vocab, n_tok),
//      it has 1..GUIDE_MAX_TOKEN_BYTES bytes and its walk from the current configuration never dies (one token may
//      push and pop several times).
//   3. One lane per token, GUIDE_TU independent chains per lane in flight, level by level, a chain's bytes fetched
//      eight at a time; state, depth and stack are updated by selects, not branches (byte_guide.hip's header has the
//      measurement behind that); a wave's 64 verdicts become two bitmap words by ballot (guide_common.h has the fetch
//      and the ballot write-out). The table always fits LDS (GUIDE_JSON_MAX_STATES * 512 bytes behind the bitmap) and
//      is copied there first.
//   4. The dense pass over the row and the rewrite of the LM-head candidates are guide_common.h's guide_mask_row: a
//      barred entry becomes bf16 -inf (0xFF80), an allowed entry keeps its exact bits; a 16-B group with no allowed
//      entry is stored without being loaded, one with all eight is not stored; lm_part != nullptr: candidate 0 = the
//      best ALLOWED entry in sampling.hip's better() order, the others (-inf, 0x7fffffff).
//   5. Everything is checked BEFORE it is used as an index: n_states in [3, table_states], done in [0, n_states),
//      state in [0, n_states], depth in [0, 32], no stack bit at or above the depth, eos in [0, vocab), 0 <= off[t] <=
//      off[t + 1] <= bytes_len for every token looked at, every entry of the table's first n_states rows either -1
//      or below 1 << 10 with its state field (+ 2 for a pop) below n_states (the whole table is validated while it
//      is copied to LDS, at every launch, so that the walk's inner loop decodes entries without checking them; the
//      advance, which reads the table before the copy, checks the entries it reads), and no pop at depth 0. A
//      violation: err |= GUIDE_ERR_TABLE, and the row, the candidates, cur and jstk stay untouched — which is why
//      the bitmap is complete before anything is written. No table content leads to an out-of-range access.
// Plain C++ and vector stores only.
#include "guide_common.h"

namespace die {

constexpr int JG_TRANS_BYTES = GUIDE_JSON_MAX_STATES * 512;

// One byte from configuration (s, d, k) over table entry v, by selects. s becomes -1 when the walk dies (no
// transition, or a push at the cap); returns true when the entry or the pop is out of bounds (s is -1 then too).
__device__ __forceinline__ bool jg_step(int v, int n_states, int& s, int& d, uint32_t& k) {
  const int nxt = v & 0xff, act = (v >> 8) & 3;
  const bool none = v == -1;
  const bool push = act == 1 || act == 2, pop = act == 3;
  const bool oob = !none && (v < 0 || v >= (1 << 10) || nxt + (pop ? 2 : 0) >= n_states || (pop && d < 1));
  const bool dead = none || oob || (push && d >= GUIDE_JSON_MAX_DEPTH);
  // push: the new container's kind goes to bit d. pop: bit d - 1 is cleared, the new top is bit d - 2
  const int dp = d - 1;
  const uint32_t k_push = k | ((act == 2 ? 1u : 0u) << (d & 31));
  const uint32_t k_pop = k & ~(1u << (dp & 31));
  const int top = dp <= 0 ? 2 : (int)((k_pop >> ((dp - 1) & 31)) & 1u);
  const int s_new = pop ? nxt + top : nxt;
  k = dead ? k : (push ? k_push : (pop ? k_pop : k));
  d = dead ? d : (push ? d + 1 : (pop ? dp : d));
  s = dead ? -1 : s_new;
  return oob;
}

// The same step for the token walk, over an entry of the VALIDATED LDS copy: no bounds checks but the pop at depth 0
// (returned), and the stack word is not cleared on a pop — a push overwrites its bit instead, so the bits at and above
// the depth may be stale inside a walk, which nothing reads (a pop reads bit d - 2, written by the push that made
// depth d - 1 or valid in the start configuration). d and k of a dead chain are never read again.
__device__ __forceinline__ bool jg_step_lean(int v, int& s, int& d, uint32_t& k) {
  const int nxt = v & 0xff, act = v >> 8;
  const bool push = (unsigned)(act - 1) < 2u, pop = act == 3;
  const bool bad_pop = pop && d < 1;
  const bool dead = v < 0 || (push && d >= GUIDE_JSON_MAX_DEPTH) || bad_pop;
  const uint32_t bit = 1u << (d & 31);
  const int top = d <= 1 ? 2 : (int)((k >> ((d - 2) & 31)) & 1u);
  k = push ? ((k & ~bit) | (act == 2 ? bit : 0u)) : k;
  s = dead ? -1 : nxt + (pop ? top : 0);
  d += (push ? 1 : 0) - (pop ? 1 : 0);
  return bad_pop;
}

// The allowed bits of tokens [0, lim) from configuration (c, d0, k0) into s_map; returns true when a table value was
// out of bounds. tr: the table's LDS copy. Uniform trip counts: every lane reaches the ballots.
__device__ __forceinline__ bool jg_walk_tokens(const int16_t* __restrict__ tr, int c, int d0, uint32_t k0, int lim,
                                               const int* __restrict__ tok_off, const uint8_t* __restrict__ tok_bytes,
                                               int bytes_len, uint32_t* s_map, int map_words) {
  bool bad = false;
  for (int t0 = 0; t0 < lim; t0 += GUIDE_T * GUIDE_TU) {
    int s[GUIDE_TU], p[GUIDE_TU], e[GUIDE_TU], d[GUIDE_TU];
    uint32_t k[GUIDE_TU];
    unsigned long long w[GUIDE_TU];  // the chain's next bytes, lowest first
#pragma unroll
    for (int u = 0; u < GUIDE_TU; ++u) {
      const int t = t0 + u * GUIDE_T + (int)threadIdx.x;
      w[u] = 0ull;
      s[u] = -1;
      p[u] = e[u] = 0;
      d[u] = d0;
      k[u] = k0;
      if (t < lim) {
        const int lo = tok_off[t], hi = tok_off[t + 1];
        if (lo < 0 || hi < lo || hi > bytes_len) {
          bad = true;
        } else if (hi > lo && hi - lo <= GUIDE_MAX_TOKEN_BYTES) {
          s[u] = c;
          p[u] = lo;
          e[u] = hi;
        }
      }
    }
    for (int step = 0; step < GUIDE_MAX_TOKEN_BYTES; ++step) {
      bool act[GUIDE_TU], any = false;
#pragma unroll
      for (int u = 0; u < GUIDE_TU; ++u) {
        act[u] = s[u] >= 0 && p[u] < e[u];
        any |= act[u];
      }
      if (__ballot(any) == 0ull) break;  // nothing left to read in this wave
      if ((step & 7) == 0) {  // uniform
#pragma unroll
        for (int u = 0; u < GUIDE_TU; ++u) w[u] = guide_next_bytes(tok_bytes, bytes_len, act[u], p[u]);
      }
      int b[GUIDE_TU], v[GUIDE_TU];
#pragma unroll
      for (int u = 0; u < GUIDE_TU; ++u) {
        b[u] = (int)(w[u] & 0xffull);
        w[u] >>= 8;
      }
      // s[u] < n_states here: it starts at c < n_states and the validated table only yields states below it
#pragma unroll
      for (int u = 0; u < GUIDE_TU; ++u) v[u] = (int)tr[(act[u] ? s[u] : 0) * 256 + b[u]];
#pragma unroll
      for (int u = 0; u < GUIDE_TU; ++u) {  // selects, not branches: the chains stay one instruction stream
        int sn = s[u];
        const bool bad_pop = jg_step_lean(v[u], sn, d[u], k[u]);  // d, k of a chain that does not read: never used
        bad |= act[u] & bad_pop;
        s[u] = act[u] ? sn : s[u];
        p[u] += act[u] ? 1 : 0;
      }
    }
#pragma unroll
    for (int u = 0; u < GUIDE_TU; ++u)
      guide_write_verdicts(s_map, map_words, t0 + u * GUIDE_T + (int)threadIdx.x, s[u] >= 0);
  }
  return bad;
}

__global__ void __launch_bounds__(GUIDE_T) json_guide_kernel(bf16_t* __restrict__ logits, int64_t stride, int vocab,
                                                             const int* __restrict__ slot_of_row, int num_slots,
                                                             const int4* __restrict__ desc,
                                                             const int16_t* __restrict__ trans, int table_states,
                                                             const int* __restrict__ tok_off, int n_tok,
                                                             const uint8_t* __restrict__ tok_bytes, int bytes_len,
                                                             int* __restrict__ cur, int* __restrict__ jstk,
                                                             int* __restrict__ err,
                                                             const int64_t* __restrict__ advance_ids,
                                                             uint32_t* __restrict__ lm_part, int lm_parts,
                                                             int map_words, int tr_off_words) {
  extern __shared__ uint32_t s_map[];  // bit t: token t is allowed; behind it (16-B aligned) the table's copy
  __shared__ int s_bad;
  const int r = blockIdx.x;
  const int slot = slot_of_row[r];
  if (slot < 0 || slot >= num_slots) return;  // uniform
  const int4 ds = desc[slot];
  const int n_states = ds.x, done = ds.y, eos = ds.z;
  int c = cur[slot];
  int d = jstk[2 * slot];
  uint32_t k = (uint32_t)jstk[2 * slot + 1];
  // everything below is uniform across the workgroup: all threads read the same words
  const bool bad_desc = n_states < 3 || n_states > table_states || n_states > GUIDE_JSON_MAX_STATES || done < 0 ||
                        done >= n_states || c < 0 || c > n_states || d < 0 || d > GUIDE_JSON_MAX_DEPTH ||
                        (d < 32 && (k >> (d & 31)) != 0u) || eos < 0 || eos >= vocab;
  if (bad_desc) {
    if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
    return;
  }
  const int lim = n_tok < vocab ? n_tok : vocab;
  int flags = 0;
  if (advance_ids != nullptr) {
    const int64_t tok = advance_ids[r];
    if (tok == (int64_t)eos) {
      if (c == n_states || c == done) {
        c = n_states;
      } else {
        flags = GUIDE_ERR_NO_EDGE;
      }
    } else if (c == n_states || tok < 0 || tok >= (int64_t)lim) {
      flags = GUIDE_ERR_NO_EDGE;
    } else {
      const int lo = tok_off[tok], hi = tok_off[tok + 1];
      if (lo < 0 || hi < lo || hi > bytes_len) {
        if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
        return;
      }
      if (hi == lo || hi - lo > GUIDE_MAX_TOKEN_BYTES) {
        flags = GUIDE_ERR_NO_EDGE;
      } else {
        int s = c, sd = d;
        uint32_t sk = k;
        for (int p = lo; p < hi; ++p) {
          const int v = (int)trans[s * 256 + (int)tok_bytes[p]];
          if (jg_step(v, n_states, s, sd, sk)) {
            if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
            return;
          }
          if (s < 0) break;
        }
        if (s < 0) {
          flags = GUIDE_ERR_NO_EDGE;
        } else {
          c = s;
          d = sd;
          k = sk;
        }
      }
    }
  }
  for (int w = threadIdx.x; w < map_words; w += GUIDE_T) s_map[w] = 0u;
  if (threadIdx.x == 0) s_bad = 0;
  int16_t* s_tr = reinterpret_cast<int16_t*>(s_map + tr_off_words);
  bool bad_entry = false;
  {  // n_states * 512 bytes, 16 B per lane and trip; both sides are 16-B aligned. Every entry is validated on the way
    const uint4* src = reinterpret_cast<const uint4*>(trans);
    uint4* dst = reinterpret_cast<uint4*>(s_tr);
    for (int q = threadIdx.x; q < n_states * 32; q += GUIDE_T) {
      const uint4 x = src[q];
      dst[q] = x;
      const uint32_t w4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = (int)(int16_t)(w4[j >> 1] >> (16 * (j & 1)));
        bad_entry |= v != -1 && (v < 0 || v >= (1 << 10) || (v & 0xff) + ((v >> 8) == 3 ? 2 : 0) >= n_states);
      }
    }
  }
  __syncthreads();
  if (bad_entry) s_bad = 1;  // behind the barrier: thread 0's reset above cannot overwrite it
  if (c == n_states) {
    if (threadIdx.x == 0) s_map[eos >> 5] = 1u << (eos & 31);
  } else {
    const bool bad = jg_walk_tokens(s_tr, c, d, k, lim, tok_off, tok_bytes, bytes_len, s_map, map_words);
    if (bad) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) {  // EOS by the state alone, whatever bytes the table gives it
      const uint32_t bit = 1u << (eos & 31);
      if (c == done) {
        s_map[eos >> 5] |= bit;
      } else {
        s_map[eos >> 5] &= ~bit;
      }
    }
  }
  __syncthreads();
  if (s_bad) {
    if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
    return;
  }
  if (threadIdx.x == 0) {
    cur[slot] = c;
    *reinterpret_cast<int2*>(jstk + 2 * slot) = make_int2(d, (int)k);
    if (flags) err[slot] |= flags;
  }
  guide_mask_row<GUIDE_T>(logits + (int64_t)r * stride, vocab, s_map,
                          lm_part != nullptr ? lm_part + (int64_t)r * lm_parts * 2 : nullptr, lm_parts);
}

hipError_t launch_json_guide(bf16_t* logits, int64_t stride, int rows, int vocab, const int* slot, int num_slots,
                             const int* desc, const int16_t* trans, int64_t table_states, const int* tok_off,
                             int64_t n_tok, const uint8_t* tok_bytes, int64_t bytes_len, int* cur, int* jstk, int* err,
                             const int64_t* advance_ids, uint32_t* lm_part, int lm_parts, hipStream_t s) {
  int map_words;
  if (!guide_row_args_ok(vocab, stride, rows, num_slots, lm_part, lm_parts, &map_words)) return hipErrorInvalidValue;
  if (logits == nullptr || slot == nullptr || desc == nullptr || trans == nullptr || tok_off == nullptr ||
      tok_bytes == nullptr || cur == nullptr || jstk == nullptr || err == nullptr)
    return hipErrorInvalidValue;
  if (table_states < 3 || table_states > GUIDE_JSON_MAX_STATES) return hipErrorInvalidValue;
  if (!guide_tok_table_ok(n_tok, bytes_len)) return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(trans) % 16) return hipErrorInvalidValue;  // the table's copy to LDS moves 16 B
  if (reinterpret_cast<uintptr_t>(jstk) % 8) return hipErrorInvalidValue;    // (depth, bits) is stored as one pair
  if (rows == 0) return hipSuccess;
  const int tr_off_words = (map_words + 3) & ~3;
  const int lds = tr_off_words * 4 + JG_TRANS_BYTES;
  static bool asked[64] = {};
  const hipError_t e = guide_ask_dynamic_lds(reinterpret_cast<const void*>(json_guide_kernel),
                                             GUIDE_MAX_MAP_BYTES + JG_TRANS_BYTES, asked);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(json_guide_kernel, dim3(rows), dim3(GUIDE_T), lds, s, logits, stride, vocab, slot, num_slots,
                     reinterpret_cast<const int4*>(desc), trans, (int)table_states, tok_off, (int)n_tok, tok_bytes,
                     (int)bytes_len, cur, jstk, err, advance_ids, lm_part, lm_parts, map_words, tr_off_words);
  return hipGetLastError();
}

}  // namespace die
