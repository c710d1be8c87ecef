// Structured outputs for gfx950: a step's bf16 logits rows are masked IN PLACE to the tokens whose BYTES a byte
// PUSHDOWN automaton with a stack of RETURN STATES can still read (src/guided_schema.py compiles a JSON Schema,
// guided_json, to a SchemaGuide). json_guide.hip's fixed table keeps one bit per level; a schema has to remember
// which schema position to return to, so this walker keeps states on its stack and reads its tables from an arena.
// json_guide.hip's idiom: one 1024-thread workgroup per batch row; row r maps through slot_of_row[r] (< 0, or beyond
// the table: the workgroup exits at once and the row's bytes stay as they are).
// Device tables:
//   * the vocabulary's bytes, byte_guide's own tensors: tok_off int32 [n_tok + 1], tok_bytes uint8 [bytes_len];
//   * trans int32 [arena_states, 256] and accept uint8 [arena_states], arenas shared by all slots, one region per
//     distinct guide. An entry is -1 (no transition) or
//       bits 0..13 the next state    bits 14..27 the return state (push only)    bits 28..29 the action: 0 none,
//       1 push, 2 pop
//     and nothing above bit 29. A push stores its return state and goes to its next state; at depth
//     GUIDE_SCHEMA_MAX_DEPTH it is no transition. A pop goes to the popped return state;
//   * desc[slot] = (state_base, n_states, eos, 0); state n_states is a virtual SINK, entered by EOS from an accepting
//     state at depth 0, only EOS is legal in it and keeps it (windows run past a finished sequence);
//   * cur[slot] / err[slot]: the arrays token_guide, byte_guide and json_guide use; sdep int32 [slots] the depth and
//     sstk int16 [slots, 32] the return states, entry 0 the oldest. Entries at or above the depth are never read. A
//     slot belongs to one sequence, so every entry keeps one writer.
// Contract (tests/schema_guide_reference.py is the oracle; tests/test_schema_guide_kernel_gpu.py compares bit for bit):
//   1. A token never holds more than GUIDE_SCHEMA_TOKEN_PUSHES of its own not-yet-popped pushes at once: a push
//      beyond that is no transition. This only narrows the set (the bytes can be spelled by shorter tokens, a
//      single-byte token pushes at most once) and lets a chain keep its pushes in one 64-bit register, four 16-bit
//      fields used as a shift register, instead of a private array. A pop takes from that register when it holds
//      something, otherwise it reads the sequence's stack (copied to LDS once per workgroup) at depth - 1: that
//      entry is still the original, because everything the token pushed above it has been popped again.
//   2. advance_ids != nullptr: the configuration first advances over advance_ids[r], this step's INPUT token, by the
//      same rules (so it never accepts a token the mask would not have allowed). EOS: an accepting state at depth 0
//      or the sink go to the sink, anything else err |= GUIDE_ERR_NO_EDGE. A dead walk, a token with no bytes,
//      beyond the table or the vocabulary, or over GUIDE_MAX_TOKEN_BYTES, and any non-EOS token in the sink:
//      err |= GUIDE_ERR_NO_EDGE. The configuration is kept in every such case.
//   3. Token t is allowed next: in the sink only EOS; else EOS iff the state accepts and the depth is 0; else iff
//      t < min(vocab, n_tok), it has 1..GUIDE_MAX_TOKEN_BYTES bytes and its walk from the current configuration
//      never dies. One lane per token, GUIDE_TU independent chains per lane in flight, level by level, a chain's bytes
//      fetched eight at a time; state, depth, the push register and its count are updated by selects, not branches
//      (byte_guide.hip's header has the measurement behind that); a wave's 64 verdicts become two bitmap words by
//      ballot (guide_common.h has the fetch and the ballot write-out). The table is read from the arena through L2:
//      a guide may hold 16 MiB. Copying a small guide's rows to LDS behind the bitmap first was built and measured,
//      and did not pay: 856.1 us against 856.8 us per launch at 32 x 128,256 for the 88 states of {"type": "object"}
//      (docs/performance.md), so no copy is made.
//   4. The dense pass over the row and the rewrite of the LM-head candidates are guide_common.h's guide_mask_row: a
//      barred entry becomes bf16 -inf (0xFF80), an allowed entry keeps its exact bits; a 16-B group with no allowed
//      entry is stored without being loaded, one with all eight is not stored; lm_part != nullptr: candidate 0 = the
//      best ALLOWED entry in sampling.hip's better() order, the others (-inf, 0x7fffffff).
//   5. Everything is checked BEFORE it is used as an index: the region within the arena, n_states in
//      [1, GUIDE_MAX_STATES], state in [0, n_states], depth in [0, 32], every live stack entry in [0, n_states), eos
//      in [0, vocab), 0 <= off[t] <= off[t + 1] <= bytes_len for every token looked at, and every entry READ (the
//      table is too large to validate per launch): -1, or nothing above bit 29, action <= 2, next and return state
//      below n_states, and no pop at depth 0. A violation: err |= GUIDE_ERR_TABLE, and the row, the candidates, cur,
//      sdep and sstk stay untouched — which is why the bitmap is complete before anything is written. No table
//      content leads to an out-of-range access.
// Plain C++ and vector stores only.
#include "guide_common.h"

namespace die {

constexpr int SG_STATE_MASK = 0x3fff;
static_assert(GUIDE_SCHEMA_MAX_DEPTH == 32, "the stack index is masked with 31");
static_assert(GUIDE_SCHEMA_TOKEN_PUSHES == 4, "a chain's pushes are four 16-bit fields of one 64-bit register");
static_assert(GUIDE_MAX_STATES <= SG_STATE_MASK + 1, "a state is a 14-bit field");

// One byte from configuration (s, d) with the chain's own pushes (ov, cnt) over table entry v, by selects. stk: the
// sequence's stack in LDS, 32 entries, every live one below n_states. s becomes -1 when the walk dies (no
// transition, a push at the depth cap or beyond the token's push cap); returns true when the entry or the pop is out
// of bounds (s is -1 then too). s stays below n_states: a next state and a return state are checked here before they
// are kept, and stk was checked when it was loaded.
__device__ __forceinline__ bool sg_step(int v, int n_states, const int* stk, int& s, int& d, unsigned long long& ov,
                                        int& cnt) {
  const int nxt = v & SG_STATE_MASK, ret = (v >> 14) & SG_STATE_MASK, act = (v >> 28) & 3;
  const bool none = v == -1;
  const bool push = act == 1, pop = act == 2;
  const bool oob = !none && (((uint32_t)v >> 30) != 0u || act == 3 || nxt >= n_states || ret >= n_states ||
                             (pop && d < 1));
  const bool dead = none || oob || (push && (d >= GUIDE_SCHEMA_MAX_DEPTH || cnt >= GUIDE_SCHEMA_TOKEN_PUSHES));
  const bool own = cnt > 0;
  const int below = stk[(d - 1) & 31];  // always inside the LDS copy; read only when the pop is legal and not own
  const int landed = own ? (int)(ov & 0xffffull) : below;
  const bool do_push = push && !dead, do_pop = pop && !dead;
  const bool pop_own = do_pop && own;
  ov = do_push ? ((ov << 16) | (unsigned long long)ret) : (pop_own ? (ov >> 16) : ov);
  cnt += (do_push ? 1 : 0) - (pop_own ? 1 : 0);
  d += (do_push ? 1 : 0) - (do_pop ? 1 : 0);
  s = dead ? -1 : (pop ? landed : nxt);
  return oob;
}

// The allowed bits of tokens [0, lim) from configuration (c, d0) into s_map; returns true when a table value was out
// of bounds. tr: the guide's rows in the arena. Uniform trip counts: every lane reaches the ballots.
__device__ __forceinline__ bool sg_walk_tokens(const int* __restrict__ tr, int n_states, const int* stk, int c, int d0,
                                               int lim, const int* __restrict__ tok_off,
                                               const uint8_t* __restrict__ tok_bytes, int bytes_len, uint32_t* s_map,
                                               int map_words) {
  bool bad = false;
  for (int t0 = 0; t0 < lim; t0 += GUIDE_T * GUIDE_TU) {
    int s[GUIDE_TU], p[GUIDE_TU], e[GUIDE_TU], d[GUIDE_TU], cnt[GUIDE_TU];
    unsigned long long ov[GUIDE_TU];  // the chain's own pushes, the latest in the low 16 bits
    unsigned long long w[GUIDE_TU];   // the chain's next bytes, lowest first
#pragma unroll
    for (int u = 0; u < GUIDE_TU; ++u) {
      const int t = t0 + u * GUIDE_T + (int)threadIdx.x;
      w[u] = ov[u] = 0ull;
      s[u] = -1;
      p[u] = e[u] = cnt[u] = 0;
      d[u] = d0;
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
      // an active chain's s is in [0, n_states): it starts at c < n_states and sg_step keeps it there
#pragma unroll
      for (int u = 0; u < GUIDE_TU; ++u) v[u] = tr[(act[u] ? s[u] : 0) * 256 + b[u]];
#pragma unroll
      for (int u = 0; u < GUIDE_TU; ++u) {  // selects, not branches: the chains stay one instruction stream
        int sn = s[u], dn = d[u], cn = cnt[u];
        unsigned long long on = ov[u];
        const bool oob = sg_step(v[u], n_states, stk, sn, dn, on, cn);
        bad |= act[u] & oob;
        s[u] = act[u] ? sn : s[u];
        d[u] = act[u] ? dn : d[u];
        cnt[u] = act[u] ? cn : cnt[u];
        ov[u] = act[u] ? on : ov[u];
        p[u] += act[u] ? 1 : 0;
      }
    }
#pragma unroll
    for (int u = 0; u < GUIDE_TU; ++u)
      guide_write_verdicts(s_map, map_words, t0 + u * GUIDE_T + (int)threadIdx.x, s[u] >= 0);
  }
  return bad;
}

__global__ void __launch_bounds__(GUIDE_T) schema_guide_kernel(bf16_t* __restrict__ logits, int64_t stride, int vocab,
                                                               const int* __restrict__ slot_of_row, int num_slots,
                                                               const int4* __restrict__ desc,
                                                               const int* __restrict__ trans,
                                                               const uint8_t* __restrict__ accept, int arena_states,
                                                               const int* __restrict__ tok_off, int n_tok,
                                                               const uint8_t* __restrict__ tok_bytes, int bytes_len,
                                                               int* __restrict__ cur, int* __restrict__ sdep,
                                                               int16_t* __restrict__ sstk, int* __restrict__ err,
                                                               const int64_t* __restrict__ advance_ids,
                                                               uint32_t* __restrict__ lm_part, int lm_parts,
                                                               int map_words) {
  extern __shared__ uint32_t s_map[];  // bit t: token t is allowed
  __shared__ int s_stk[GUIDE_SCHEMA_MAX_DEPTH];
  __shared__ int s_bad;
  const int r = blockIdx.x;
  const int slot = slot_of_row[r];
  if (slot < 0 || slot >= num_slots) return;  // uniform
  const int4 ds = desc[slot];
  const int base = ds.x, n_states = ds.y, eos = ds.z;
  int c = cur[slot];
  int d = sdep[slot];
  // everything below is uniform across the workgroup: all threads read the same words
  const bool bad_desc = base < 0 || n_states < 1 || n_states > GUIDE_MAX_STATES || base > arena_states - n_states ||
                        c < 0 || c > n_states || d < 0 || d > GUIDE_SCHEMA_MAX_DEPTH || eos < 0 || eos >= vocab;
  if (bad_desc) {
    if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
    return;
  }
  // the sequence's stack, once per workgroup; every live entry is checked on the way, the rest are zero
  bool bad_stk = false;
  if (threadIdx.x < GUIDE_SCHEMA_MAX_DEPTH) {
    int ent = 0;
    if ((int)threadIdx.x < d) {
      ent = (int)sstk[slot * GUIDE_SCHEMA_MAX_DEPTH + (int)threadIdx.x];
      bad_stk = ent < 0 || ent >= n_states;
    }
    s_stk[threadIdx.x] = bad_stk ? 0 : ent;
  }
  if (__syncthreads_or(bad_stk ? 1 : 0)) {
    if (threadIdx.x == 0) err[slot] |= GUIDE_ERR_TABLE;
    return;
  }
  const int* tr = trans + (int64_t)base * 256;
  const int lim = n_tok < vocab ? n_tok : vocab;
  int flags = 0;
  unsigned long long aov = 0ull;  // the advance token's pushes that are still held
  int acnt = 0;
  if (advance_ids != nullptr) {
    const int64_t tok = advance_ids[r];
    if (tok == (int64_t)eos) {
      if (c == n_states || (accept[base + c] != 0 && d == 0)) {
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
        int s = c, sd = d, sc = 0;
        unsigned long long so = 0ull;
        for (int p = lo; p < hi; ++p) {
          const int v = tr[s * 256 + (int)tok_bytes[p]];
          if (sg_step(v, n_states, s_stk, s, sd, so, sc)) {
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
          aov = so;
          acnt = sc;
        }
      }
    }
  }
  __syncthreads();  // every thread has walked the advance over the old stack
  // the held pushes go on top of what the token left of the old stack: entries [d - acnt, d), the oldest first.
  // d - acnt >= 0 (each held push raised d by one) and d <= 32
  if ((int)threadIdx.x < acnt)
    s_stk[d - acnt + (int)threadIdx.x] = (int)((aov >> (16 * (acnt - 1 - (int)threadIdx.x))) & 0xffffull);
  for (int w = threadIdx.x; w < map_words; w += GUIDE_T) s_map[w] = 0u;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  if (c == n_states) {
    if (threadIdx.x == 0) s_map[eos >> 5] = 1u << (eos & 31);
  } else {
    const bool bad = sg_walk_tokens(tr, n_states, s_stk, c, d, lim, tok_off, tok_bytes, bytes_len, s_map, map_words);
    if (bad) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) {  // EOS by the configuration alone, whatever bytes the table gives it
      const uint32_t bit = 1u << (eos & 31);
      if (accept[base + c] != 0 && d == 0) {
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
    sdep[slot] = d;
    if (flags) err[slot] |= flags;
  }
  if ((int)threadIdx.x < acnt) {
    const int at = d - acnt + (int)threadIdx.x;
    sstk[slot * GUIDE_SCHEMA_MAX_DEPTH + at] = (int16_t)s_stk[at];
  }
  guide_mask_row<GUIDE_T>(logits + (int64_t)r * stride, vocab, s_map,
                          lm_part != nullptr ? lm_part + (int64_t)r * lm_parts * 2 : nullptr, lm_parts);
}

hipError_t launch_schema_guide(bf16_t* logits, int64_t stride, int rows, int vocab, const int* slot, int num_slots,
                               const int* desc, const int* trans, int64_t trans_states, const uint8_t* accept,
                               int64_t accept_len, const int* tok_off, int64_t n_tok, const uint8_t* tok_bytes,
                               int64_t bytes_len, int* cur, int* sdep, int16_t* sstk, int* err,
                               const int64_t* advance_ids, uint32_t* lm_part, int lm_parts, hipStream_t s) {
  int map_words;
  if (!guide_row_args_ok(vocab, stride, rows, num_slots, lm_part, lm_parts, &map_words)) return hipErrorInvalidValue;
  if (logits == nullptr || slot == nullptr || desc == nullptr || trans == nullptr || accept == nullptr ||
      tok_off == nullptr || tok_bytes == nullptr || cur == nullptr || sdep == nullptr || sstk == nullptr ||
      err == nullptr)
    return hipErrorInvalidValue;
  const int64_t arena = trans_states < accept_len ? trans_states : accept_len;
  if (arena < 1 || arena > GUIDE_SCHEMA_STATE_ARENA) return hipErrorInvalidValue;
  if (!guide_tok_table_ok(n_tok, bytes_len)) return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(schema_guide_kernel, dim3(rows), dim3(GUIDE_T), map_words * 4, s, logits, stride, vocab, slot,
                     num_slots, reinterpret_cast<const int4*>(desc), trans, accept, (int)arena, tok_off, (int)n_tok,
                     tok_bytes, (int)bytes_len, cur, sdep, sstk, err, advance_ids, lm_part, lm_parts, map_words);
  return hipGetLastError();
}

}  // namespace die
