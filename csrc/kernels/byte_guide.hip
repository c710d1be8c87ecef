// Constrained decoding over multi-byte (BPE) vocabularies for gfx950: a step's bf16 logits rows are masked IN PLACE
// to the tokens whose BYTES a per-sequence byte DFA can still read (src/guided.py compiles a guided_regex to a
// ByteGuide when the vocabulary holds tokens longer than one byte). Nothing is lifted to tokens on the host: every
// token's bytes are walked through the DFA here, inside the step. token_guide.hip's idiom: one 1024-thread workgroup
// per batch row; row r maps through slot_of_row[r] (< 0, or beyond the table: the workgroup exits at once and the
// row's bytes stay as they are).
// Device tables:
//   * the vocabulary's bytes, one table per runner: tok_off int32 [n_tok + 1], tok_bytes uint8 [bytes_len]; a token
//     without bytes has length 0. A token longer than GUIDE_MAX_TOKEN_BYTES is never allowed: that only narrows the
//     set, and its bytes can still be spelled by shorter tokens;
//   * trans int16 [arena_states, 256] (-1: no transition) and accept uint8 [arena_states], arenas shared by all slots;
//   * desc[slot] = (state_base, n_states, eos, 0);  cur[slot] / err[slot]: the arrays token_guide uses (a slot
//     belongs to one sequence, so each entry keeps one writer). State n_states is a virtual SINK: entered by EOS
//     from an accepting state, only EOS is legal in it and keeps it (windows run past a finished sequence).
// Contract (tests/byte_guide_reference.py is the oracle; tests/test_byte_guide_kernel_gpu.py compares bit for bit):
//   1. advance_ids != nullptr: the state first advances over advance_ids[r], this step's INPUT token. EOS: to the
//      sink from an accepting state or the sink, else err |= GUIDE_ERR_NO_EDGE. Any other token walks its bytes
//      from cur; a dead transition, a token with no bytes, beyond the table or the vocabulary, or over the length
//      cap, and any non-EOS token in the sink: err |= GUIDE_ERR_NO_EDGE. The state is kept in every such case.
//   2. Token t is allowed next: in the sink only EOS; else EOS iff accept[c]; else iff t < min(vocab, n_tok), it
//      has 1..GUIDE_MAX_TOKEN_BYTES bytes and its walk from c never dies. One lane per token, GUIDE_TU independent
//      chains per lane in flight, level by level, a chain's bytes fetched eight at a time and its state updated by
//      selects (written with branches the compiler serialised the chains: 269 us per launch at 32 x 128,256 against
//      217); a wave's 64 verdicts become two bitmap words by ballot (guide_common.h has the fetch and the ballot
//      write-out). A guide of up to BG_LDS_STATES states has its trans rows copied to LDS first (the walk's lookups
//      then never leave the CU), a larger one is read through L2.
//   3. One dense pass (guide_common.h's guide_mask_row): a barred entry becomes bf16 -inf (0xFF80), an allowed entry
//      keeps its exact bits; a 16-B group with no allowed entry is stored without being loaded, one with all eight
//      is not stored.
//   4. lm_part != nullptr: the row's LM-head candidates are rewritten by the same pass (candidate 0 = the best
//      ALLOWED entry in sampling.hip's better() order, the others (-inf, 0x7fffffff)).
//   5. Everything is checked BEFORE it is used as an index: state_base + n_states within the arenas, cur in
//      [0, n_states], eos in [0, vocab), 0 <= off[t] <= off[t + 1] <= bytes_len for every token looked at, every
//      trans value read in [-1, n_states). A violation: err |= GUIDE_ERR_TABLE, and the row, the candidates and
//      cur stay untouched — which is why the bitmap is complete before the row is written. No table content leads
//      to an out-of-range access.
#include "guide_common.h"

namespace die {

constexpr int BG_LDS_STATES = GUIDE_BYTE_LDS_STATES;
constexpr int BG_LDS_TRANS_BYTES = BG_LDS_STATES * 512;

// The allowed bits of tokens [0, lim) from state c into s_map; returns true when a table value was out of bounds.
// tr: the guide's trans rows, their LDS copy or the arena itself (inlined once for each). Uniform trip counts: every
// lane reaches the ballots.
__device__ __forceinline__ bool bg_walk_tokens(const int16_t* __restrict__ tr, int c, int n_states, int lim,
                                               const int* __restrict__ tok_off, const uint8_t* __restrict__ tok_bytes,
                                               int bytes_len, uint32_t* s_map, int map_words) {
  bool bad = false;
  for (int t0 = 0; t0 < lim; t0 += GUIDE_T * GUIDE_TU) {
    int s[GUIDE_TU], p[GUIDE_TU], e[GUIDE_TU];
    unsigned long long w[GUIDE_TU];  // the chain's next bytes, lowest first
#pragma unroll
    for (int u = 0; u < GUIDE_TU; ++u) {
      const int t = t0 + u * GUIDE_T + (int)threadIdx.x;
      w[u] = 0ull;
      s[u] = -1;
      p[u] = e[u] = 0;
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
      // a lane with nothing to read loads the head of each table (both exist): the loads stay unconditional, so the
      // GUIDE_TU chains' loads issue together
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
#pragma unroll
      for (int u = 0; u < GUIDE_TU; ++u) v[u] = (int)tr[(act[u] ? s[u] : 0) * 256 + b[u]];
#pragma unroll
      for (int u = 0; u < GUIDE_TU; ++u) {  // selects, not branches: the four chains stay one instruction stream
        const bool oob = v[u] < -1 || v[u] >= n_states;
        bad |= act[u] & oob;
        s[u] = act[u] ? (oob ? -1 : v[u]) : s[u];  // -1: the walk died, or read a value out of bounds
        p[u] += act[u] ? 1 : 0;
      }
    }
#pragma unroll
    for (int u = 0; u < GUIDE_TU; ++u)
      guide_write_verdicts(s_map, map_words, t0 + u * GUIDE_T + (int)threadIdx.x, s[u] >= 0);
  }
  return bad;
}

__global__ void __launch_bounds__(GUIDE_T) byte_guide_kernel(bf16_t* __restrict__ logits, int64_t stride, int vocab,
                                                             const int* __restrict__ slot_of_row, int num_slots,
                                                             const int4* __restrict__ desc,
                                                             const int16_t* __restrict__ trans,
                                                             const uint8_t* __restrict__ accept, int arena_states,
                                                             const int* __restrict__ tok_off, int n_tok,
                                                             const uint8_t* __restrict__ tok_bytes, int bytes_len,
                                                             int* __restrict__ cur, int* __restrict__ err,
                                                             const int64_t* __restrict__ advance_ids,
                                                             uint32_t* __restrict__ lm_part, int lm_parts,
                                                             int map_words, int tr_off_words) {
  extern __shared__ uint32_t s_map[];  // bit t: token t is allowed; behind it (16-B aligned) the trans rows' copy
  __shared__ int s_bad;
  const int r = blockIdx.x;
  const int slot = slot_of_row[r];
  if (slot < 0 || slot >= num_slots) return;  // uniform
  const int4 d = desc[slot];
  const int state_base = d.x, n_states = d.y, eos = d.z;
  int c = cur[slot];
  // everything below is uniform across the workgroup: all threads read the same words
  const bool bad_desc = state_base < 0 || n_states < 1 || (int64_t)state_base + n_states > (int64_t)arena_states ||
                        c < 0 || c > n_states || eos < 0 || eos >= vocab;
  if (bad_desc) {
    if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
    return;
  }
  const int16_t* tr = trans + (int64_t)state_base * 256;
  const uint8_t* ac = accept + state_base;
  const int lim = n_tok < vocab ? n_tok : vocab;
  int flags = 0;
  if (advance_ids != nullptr) {
    const int64_t tok = advance_ids[r];
    if (tok == (int64_t)eos) {
      if (c == n_states || ac[c] != 0) {
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
        int s = c;
        for (int p = lo; p < hi; ++p) {
          const int v = (int)tr[s * 256 + (int)tok_bytes[p]];
          if (v < -1 || v >= n_states) {
            if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
            return;
          }
          s = v;
          if (v < 0) break;
        }
        if (s < 0) {
          flags = GUIDE_ERR_NO_EDGE;
        } else {
          c = s;
        }
      }
    }
  }
  for (int w = threadIdx.x; w < map_words; w += GUIDE_T) s_map[w] = 0u;
  if (threadIdx.x == 0) s_bad = 0;
  const bool in_lds = c < n_states && n_states <= BG_LDS_STATES;
  int16_t* s_tr = reinterpret_cast<int16_t*>(s_map + tr_off_words);
  if (in_lds) {  // n_states * 512 bytes, 16 B per lane and trip; both sides are 16-B aligned
    const uint4* src = reinterpret_cast<const uint4*>(tr);
    uint4* dst = reinterpret_cast<uint4*>(s_tr);
    for (int q = threadIdx.x; q < n_states * 32; q += GUIDE_T) dst[q] = src[q];
  }
  __syncthreads();
  if (c == n_states) {
    if (threadIdx.x == 0) s_map[eos >> 5] = 1u << (eos & 31);
  } else {
    const bool bad = in_lds ? bg_walk_tokens(s_tr, c, n_states, lim, tok_off, tok_bytes, bytes_len, s_map, map_words)
                            : bg_walk_tokens(tr, c, n_states, lim, tok_off, tok_bytes, bytes_len, s_map, map_words);
    if (bad) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) {  // EOS by the state alone, whatever bytes the table gives it
      const uint32_t bit = 1u << (eos & 31);
      if (ac[c] != 0) {
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
    if (flags) err[slot] |= flags;
  }
  guide_mask_row<GUIDE_T>(logits + (int64_t)r * stride, vocab, s_map,
                          lm_part != nullptr ? lm_part + (int64_t)r * lm_parts * 2 : nullptr, lm_parts);
}

hipError_t launch_byte_guide(bf16_t* logits, int64_t stride, int rows, int vocab, const int* slot, int num_slots,
                             const int* desc, const int16_t* trans, int64_t trans_states, const uint8_t* accept,
                             int64_t accept_len, const int* tok_off, int64_t n_tok, const uint8_t* tok_bytes,
                             int64_t bytes_len, int* cur, int* err, const int64_t* advance_ids, uint32_t* lm_part,
                             int lm_parts, hipStream_t s) {
  int map_words;
  if (!guide_row_args_ok(vocab, stride, rows, num_slots, lm_part, lm_parts, &map_words)) return hipErrorInvalidValue;
  if (logits == nullptr || slot == nullptr || desc == nullptr || trans == nullptr || accept == nullptr ||
      tok_off == nullptr || tok_bytes == nullptr || cur == nullptr || err == nullptr)
    return hipErrorInvalidValue;
  if (trans_states < 1 || trans_states > GUIDE_BYTE_STATE_ARENA || accept_len < 1 ||
      accept_len > GUIDE_BYTE_STATE_ARENA)
    return hipErrorInvalidValue;
  if (!guide_tok_table_ok(n_tok, bytes_len)) return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(trans) % 16) return hipErrorInvalidValue;  // the rows' copy to LDS moves 16 B
  if (rows == 0) return hipSuccess;
  const int tr_off_words = (map_words + 3) & ~3;
  const int lds = tr_off_words * 4 + BG_LDS_TRANS_BYTES;
  static bool asked[64] = {};
  const hipError_t e = guide_ask_dynamic_lds(reinterpret_cast<const void*>(byte_guide_kernel),
                                             GUIDE_MAX_MAP_BYTES + BG_LDS_TRANS_BYTES, asked);
  if (e != hipSuccess) return e;
  const int arena_states = (int)(trans_states < accept_len ? trans_states : accept_len);
  hipLaunchKernelGGL(byte_guide_kernel, dim3(rows), dim3(GUIDE_T), lds, s, logits, stride, vocab, slot, num_slots,
                     reinterpret_cast<const int4*>(desc), trans, accept, arena_states, tok_off, (int)n_tok, tok_bytes,
                     (int)bytes_len, cur, err, advance_ids, lm_part, lm_parts, map_words, tr_off_words);
  return hipGetLastError();
}

}  // namespace die
