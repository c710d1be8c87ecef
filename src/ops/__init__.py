"""
Custom ops. GPU tensors always go to the hand-written gfx950 HIP kernels in
``src/_C*.so`` (built by :mod:`src._build`); if that extension is missing a
GPU call raises — there is no silent eager fallback on the GPU. CPU tensors use
:mod:`src.ops.reference` (the fp32 semantics the kernels are tested against),
which lets the engine's control flow run in CPU-only tests.
"""

from __future__ import annotations

from typing import Optional

import torch

from . import reference as ref
# the decode GEMM's mode word, tiles, measured table and lookup: one module, re-exported for the callers of ops
from .decode_tiles import (DECODE_GEMM_MAX_M, DECODE_TILE_CFG, HALF_RING, MODE_BF16, MODE_MASK, MODE_RESID, MODE_SILU,
                           MODE_SILU_NORM, MODE_SILU_NORM_SK, MODE_SLAB, P13, P13_BASE_SHIFT, SSP_LD, SSP_MAX_TILES,
                           SSP_MAX_TILES_WIDE, TILED, _tile_overrides, decode_bucket, decode_tile, decode_tile_silu,
                           gd_tile, gd_tile_valid, moe_decode_tiles)
# the lossless 13-bit weight layout of the (128, 128) tile: packer and exact inverse (pure torch)
from .p13 import P13_DEN, P13_NUM, P13_TILE, gd_pack_weights_p13, gd_unpack_weights_p13, p13_base7

_C = None
_C_ERR: Optional[BaseException] = None
try:
    from src import _C  # type: ignore  # noqa: F811
except Exception as e:  # pragma: no cover - depends on build state
    _C_ERR = e


def native_available() -> bool:
    return _C is not None


def _kern():
    if _C is None:
        raise RuntimeError(
            "HIP kernel extension src/_C is not built or failed to load "
            f"({_C_ERR!r}); run `python -m src._build` (hipcc --offload-arch=gfx950)")
    return _C


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    if not x.is_cuda:
        r = ref.rms_norm(x, w, eps)
        if out is not None:
            out.copy_(r)
            return out
        return r
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _kern().rms_norm(out, x, w, eps)
    return out


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """residual += x (in place, bf16); returns rms_norm(residual) * w."""
    if not x.is_cuda:
        y, r = ref.fused_add_rms_norm(x, residual, w, eps)
        residual.copy_(r)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _kern().fused_add_rms_norm(out, x, residual, w, eps)
    return out


def silu_and_mul(x: torch.Tensor, out: Optional[torch.Tensor] = None,
                 row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """silu(gate) * up for x = [gate | up]; row_scale (fp32 [T]): silu(r gate) * (r up) — the prefill RMSNorm
    applied after a projection of the raw residual (:func:`rms_row_scale`)."""
    if not x.is_cuda:
        if row_scale is not None:
            x = (x.float() * row_scale[:, None]).to(x.dtype)
        return ref.silu_and_mul(x)
    if out is None:
        out = torch.empty(x.shape[0], x.shape[1] // 2, dtype=x.dtype, device=x.device)
    _kern().silu_and_mul(out, x, row_scale if row_scale is not None else _empty(x.device))
    return out


def silu_and_mul_views(gate: torch.Tensor, up: torch.Tensor, out: torch.Tensor,
                       row_scale: Optional[torch.Tensor] = None, per: int = 0) -> torch.Tensor:
    """out = silu(r gate) * (r up) on [T, I] row views (unit column stride, e.g. column blocks of a wider
    buffer): the SiLU * up of one FFN column chunk, written into its columns of the [T, inter] activation.
    per: 16-byte chunks per lane (0: the launcher's choice; micro-benchmarks only)."""
    if not gate.is_cuda:
        g, u = gate.float(), up.float()
        if row_scale is not None:
            g, u = g * row_scale[:, None], u * row_scale[:, None]
        out.copy_((torch.nn.functional.silu(g) * u).to(out.dtype))
        return out
    _kern().silu_and_mul_views(out, gate, up, row_scale if row_scale is not None else _empty(gate.device), per)
    return out


def set_attn_few_pair_parts(on: bool) -> None:
    """Decode attention launch policy for few (sequence, kv head) pairs (tensor-parallel shards) at a short static
    context bound: one chunk per part, one workgroup per task (default on; off = the static split, for A/Bs)."""
    if native_available():
        _kern().attn_set_few_pair_parts(bool(on))


def rms_row_scale(resid: torch.Tensor, x: Optional[torch.Tensor], eps: float,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Prefill RMSNorm as a row scale (norm weight folded into the consuming projection): resid += x (bf16,
    in place; x None: no add) and returns rs [T] fp32 = rsqrt(mean(resid^2) + eps). The projections then run
    on the raw residual and their consumers scale the output rows (rope_and_cache / attn_prefill /
    silu_and_mul ``row_scale``): no normalised copy of the residual is written."""
    t = resid.shape[0]
    if out is None:
        out = torch.empty(t, dtype=torch.float32, device=resid.device)
    if not resid.is_cuda:
        if x is not None:
            resid.copy_((resid.float() + x.float()).to(resid.dtype))
        out.copy_(torch.rsqrt(resid.float().pow(2).mean(-1) + eps))
        return out
    _kern().rms_row_scale(out, resid, x if x is not None else _empty(resid.device), float(eps))
    return out


def rope_and_cache(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, hq: int, hkv: int, head_dim: int,
                   rot_q: bool = True, row_scale: Optional[torch.Tensor] = None) -> None:
    """Rotate k (and q unless rot_q=False: prefill attention then rotates its Q rows on load, see
    attn_prefill's cos_sin) and write k / v into the paged cache. row_scale (fp32 [T], with rot_q=False):
    k and v rows are scaled by the token's RMSNorm scale (:func:`rms_row_scale`); q is left to the attention."""
    if not qkv.is_cuda:
        assert rot_q and row_scale is None, "the CPU reference path rotates q here"
        ref.rope_and_cache(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, hq, hkv, head_dim)
        return
    assert row_scale is None or not rot_q, "a row scale is applied with the attention's Q rotation"
    _kern().rope_and_cache(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, hq, hkv, head_dim, rot_q,
                           row_scale if row_scale is not None else _empty(qkv.device))


def attn_prefill(q, k_cache, v_cache, block_tables, cu_q, ctx_lens, max_q_len: int, hq: int, hkv: int,
                 scale: float, out: Optional[torch.Tensor] = None, cos_sin: Optional[torch.Tensor] = None,
                 q_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal paged prefill attention. cos_sin ([max_pos, 128] fp32): q is NOT yet rotated, the kernel
    applies RoPE to each Q row as it loads it (token positions ctx - q_len + i). q_scale (fp32 [T], with
    cos_sin): each Q row is also scaled by its token's RMSNorm scale (:func:`rms_row_scale`)."""
    if not q.is_cuda:
        assert cos_sin is None and q_scale is None, "the CPU reference path takes a rotated q"
        return ref.attention(q, k_cache, v_cache, block_tables, cu_q, ctx_lens, hq, hkv, scale).reshape(q.shape[0], -1)
    if out is None:
        out = torch.empty(q.shape[0], hq * 128, dtype=q.dtype, device=q.device)
    assert q_scale is None or cos_sin is not None, "the Q row scale is applied with the rotation"
    e = _empty(q.device)
    _kern().attn_prefill(out, q, k_cache, v_cache, block_tables, cu_q, ctx_lens, max_q_len, hq, hkv, scale,
                         cos_sin if cos_sin is not None else e, q_scale if q_scale is not None else e)
    return out


def decode_partials(max_ctx: int) -> int:
    return int(_kern().decode_partials(max_ctx))


def attn_decode(q, k_cache, v_cache, block_tables, ctx_lens, max_ctx: int, hq: int, hkv: int, scale: float,
                part_o: Optional[torch.Tensor] = None, part_ml: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, counters: Optional[torch.Tensor] = None,
                merge_kernel: bool = False, kv_once: bool = True) -> torch.Tensor:
    """Paged decode attention. `counters` (int32, >= num_seqs * hkv, zeroed once) are the
    per-(sequence, kv head) tickets of the self-merging kernel; they are re-armed by the kernel,
    so a runner allocates them once. merge_kernel=True forces the two-launch path. kv_once: the
    self-merging kernel streams K/V with the once-read (nt) cache policy (False: the default policy,
    for A/B; the result is the same bit for bit either way)."""
    if not q.is_cuda:
        n = ctx_lens.numel()
        cu = torch.arange(n + 1, dtype=torch.int32)
        return ref.attention(q[:n], k_cache, v_cache, block_tables, cu, ctx_lens, hq, hkv, scale).reshape(n, -1)
    n = ctx_lens.numel()
    if out is None:
        out = torch.empty(n, hq * 128, dtype=q.dtype, device=q.device)
    if part_o is None or part_ml is None:
        maxp = decode_partials(max_ctx)
        part_o = torch.empty(n * hq * maxp * 128, dtype=torch.float32, device=q.device)
        part_ml = torch.empty(n * hq * maxp * 2, dtype=torch.float32, device=q.device)
    if merge_kernel:
        counters = torch.empty(0, dtype=torch.int32, device=q.device)
    elif counters is None:
        counters = torch.zeros(n * hkv, dtype=torch.int32, device=q.device)
    _kern().attn_decode(out, part_o, part_ml, counters, q, k_cache, v_cache, block_tables, ctx_lens, max_ctx, hq,
                        hkv, scale, kv_once)
    return out


def attn_decode_fused(qkv_slab: torch.Tensor, ssp: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor,
                      slot_mapping: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                      block_tables: torch.Tensor, ctx_lens: torch.Tensor, max_ctx: int, hq: int, hkv: int,
                      scale: float, eps: float, hidden: int, part_o: torch.Tensor, part_ml: torch.Tensor,
                      counters: torch.Tensor, out: Optional[torch.Tensor] = None,
                      kv_once: bool = True) -> torch.Tensor:
    """Decode attention whose prologue does the input RMSNorm row scale (statistics ssp [T, 32],
    weight folded into Wqkv), the split-K reduction of the qkv slabs [sk, M, width], RoPE at
    position ctx-1 and the paged KV write of the new token (attention.hip, FUSED). kv_once as in
    attn_decode."""
    n = ctx_lens.numel()
    if out is None:
        out = torch.empty(n, hq * 128, dtype=torch.bfloat16, device=qkv_slab.device)
    _kern().attn_decode_fused(out, part_o, part_ml, counters, qkv_slab, ssp, positions, cos_sin, slot_mapping,
                              k_cache, v_cache, block_tables, ctx_lens, max_ctx, hq, hkv, scale, eps, hidden,
                              kv_once)
    return out


def decode_advance(out, ids, pos, ctx, slots, bt, step, tokens, cnt, n_real, rows: int, block_size: int) -> None:
    """Device-side advance of the decode inputs (decode_step.hip); see ModelRunner.decode_multi."""
    _kern().decode_advance(out, ids, pos, ctx, slots, bt, step, tokens, cnt, n_real, rows, block_size)


def sample(logits, temperature=None, top_k=None, top_p=None, seeds=None, steps=None,
           out: Optional[torch.Tensor] = None, scratch=None, lm_part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``scratch`` = (part int32 [>= rows * 32], cnt int32 [>= rows], zero): greedy rows are split over several
    workgroups each (a decode step's argmax on ~256 CUs instead of one per row); keep it for the engine's life
    (the tickets are re-armed by the kernel, so it is graph-capturable). ``lm_part`` [rows, parts, 2] int32: the
    LM head's per-column-tile candidates (:func:`linear_tiled_argmax`) — greedy rows reduce those instead."""
    if not logits.is_cuda:
        return ref.sample(logits, temperature, top_k, top_p, seeds, steps)
    if out is None:
        out = torch.empty(logits.shape[0], dtype=torch.long, device=logits.device)
    part, cnt = scratch if scratch is not None else (None, None)
    _kern().sample(out, logits, temperature, top_k, top_p, seeds, steps, part, cnt, lm_part)
    return out


LOGPROBS_MAX_TOP = 20  # the OpenAI chat API's cap (launchers.h)


def token_logprobs(logits: torch.Tensor, targets: torch.Tensor, top_n: int, out=None):
    """Log-probabilities of the model's RAW distribution (``log_softmax`` of the bf16 row in fp32, before
    temperature and filters) -> ``(lp fp32 [R], rank int32 [R], top_lp fp32 [R, top_n], top_id int32 [R, top_n])``.
    Tokens are ordered by larger logit, then lower id: ``rank`` counts the tokens strictly before ``targets[r]``
    (the argmax has rank 0) and the top lists are the first ``top_n`` (0..20) tokens in that order. A target
    outside ``[0, vocab)`` gives ``-inf`` and ``vocab``. ``out`` = the four tensors to write into (the top lists
    may be wider than ``top_n``: the columns beyond it are left alone and the returned lists are views)."""
    top_n = int(top_n)
    if not logits.is_cuda:
        res = ref.token_logprobs(logits, targets, top_n)
        if out is None:
            return res
        r = logits.shape[0]
        out[0][:r].copy_(res[0])
        out[1][:r].copy_(res[1])
        out[2][:r, :top_n].copy_(res[2])
        out[3][:r, :top_n].copy_(res[3])
        return out[0][:r], out[1][:r], out[2][:r, :top_n], out[3][:r, :top_n]
    r = logits.shape[0]
    if out is None:
        dev = logits.device
        w = max(top_n, 0)
        out = (torch.empty(r, dtype=torch.float32, device=dev), torch.empty(r, dtype=torch.int32, device=dev),
               torch.empty(r, w, dtype=torch.float32, device=dev), torch.empty(r, w, dtype=torch.int32, device=dev))
    lp, rank, top_lp, top_id = out
    _kern().token_logprobs(lp, rank, top_lp, top_id, logits, targets, top_n)
    return lp[:r], rank[:r], top_lp[:r, :top_n], top_id[:r, :top_n]


LOGIT_BIAS_MAX = 300  # logit_bias entries per request (launchers.h; the OpenAI API's cap)
LOGIT_COUNT_MAX = ref.LOGIT_COUNT_MAX


def logit_process(logits: torch.Tensor, slot: torch.Tensor, state: torch.Tensor, params: torch.Tensor,
                  bias_cnt: torch.Tensor, bias_ids: torch.Tensor, bias_vals: torch.Tensor,
                  count_ids: Optional[torch.Tensor] = None, lm_part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Repetition / frequency / presence penalties and logit_bias on ``logits`` [rows, vocab] bf16 IN PLACE, before
    the sampler reads them (:func:`reference.logit_process` is the per-entry contract). Row r uses the state of
    ``slot[r]`` (int32; < 0: the row is left untouched): ``state`` int16 [slots, vocab] (as uint16: bit 15 = the
    token occurs in the prompt, bits 0-14 = how often it was generated, saturating at 32767), ``params`` fp32
    [slots, 4] = (rp, fp32(1 / rp), freq, pres), ``bias_cnt`` int32 [slots] and ``bias_ids`` int32 / ``bias_vals``
    fp32 [slots, <= 300] with unique ids. ``count_ids`` int64 [rows]: the step's input tokens (the previous
    samples), added to the counts first. ``lm_part`` [rows, parts, 2] int32: the LM head's greedy candidates of
    these rows, overwritten with the processed row's (max, lowest index) so that :func:`sample` /
    :func:`sample_advance` with ``lm_part`` return the processed argmax."""
    if not logits.is_cuda:
        return ref.logit_process_rows(logits, slot, state, params, bias_cnt, bias_ids, bias_vals, count_ids, lm_part)
    _kern().logit_process(logits, slot, state, params, bias_cnt, bias_ids, bias_vals, count_ids, lm_part)
    return logits


# constrained decoding (launchers.h): the per-request caps the host compiler enforces (src/guided.py) and the arenas
GUIDE_MAX_STATES = 16384      # states of one request's automaton
GUIDE_MAX_EDGES = 262144      # edges of one request's automaton: twice the largest vocabulary
GUIDE_ROWPTR_ARENA = 262144   # int32 row pointers shared by all slots
GUIDE_EDGE_ARENA = 4194304    # (tok, next) int32 pairs shared by all slots: 32 MiB
GUIDE_ERR_NO_EDGE = ref.GUIDE_ERR_NO_EDGE
GUIDE_ERR_TABLE = ref.GUIDE_ERR_TABLE


def token_guide(logits: torch.Tensor, slot: torch.Tensor, desc: torch.Tensor, rowptr: torch.Tensor,
                edges: torch.Tensor, cur: torch.Tensor, err: torch.Tensor,
                advance_ids: Optional[torch.Tensor] = None, lm_part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Constrained decoding on ``logits`` [rows, vocab] bf16 IN PLACE, before the sampler reads them: every entry
    the row's token automaton does not allow next becomes ``-inf``, an allowed entry keeps its exact bits
    (:func:`reference.token_guide_rows` is the contract). Row r uses the tables of ``slot[r]`` (int32; < 0: the row
    is left untouched): ``desc`` int32 [slots, 4] = (state_base, n_states, edge_base, n_edges) into the arenas
    ``rowptr`` int32 [R] (CSR row pointers, relative to edge_base) and ``edges`` int32 [E, 2] = (tok, next);
    ``cur`` int32 [slots] the current state and ``err`` int32 [slots] sticky error bits (GUIDE_ERR_*).
    ``advance_ids`` int64 [rows]: the step's input tokens (the previous samples), which the state advances over
    first. ``lm_part`` [rows, parts, 2] int32: the LM head's greedy candidates of these rows, overwritten with the
    best allowed entry so that :func:`sample` / :func:`sample_advance` with ``lm_part`` return it."""
    if not logits.is_cuda:
        return ref.token_guide_rows(logits, slot, desc, rowptr, edges, cur, err, advance_ids, lm_part)
    _kern().token_guide(logits, slot, desc, rowptr, edges, cur, err, advance_ids, lm_part)
    return logits


# constrained decoding over a multi-byte vocabulary (launchers.h)
GUIDE_MAX_TOKEN_BYTES = ref.GUIDE_MAX_TOKEN_BYTES  # a longer token is never allowed: its bytes can still be spelled
GUIDE_BYTE_STATE_ARENA = 65536   # states shared by all slots: trans int16 [., 256] 32 MiB, accept uint8 64 KiB
GUIDE_BYTE_LDS_STATES = 208      # a guide of up to this many states is walked from LDS, a larger one through L2
GUIDE_TOK_TABLE_MAX = 1 << 20    # tokens in the vocabulary's byte table
GUIDE_TOK_BYTES_MAX = 1 << 25    # bytes in it


def byte_guide(logits: torch.Tensor, slot: torch.Tensor, desc: torch.Tensor, trans: torch.Tensor,
               accept: torch.Tensor, tok_off: torch.Tensor, tok_bytes: torch.Tensor, cur: torch.Tensor,
               err: torch.Tensor, advance_ids: Optional[torch.Tensor] = None,
               lm_part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Constrained decoding on ``logits`` [rows, vocab] bf16 IN PLACE for vocabularies with multi-byte tokens: every
    token whose BYTES the row's byte DFA cannot read from its current state becomes ``-inf``, an allowed entry keeps
    its exact bits (:func:`reference.byte_guide_rows` is the contract). Row r uses the tables of ``slot[r]`` (int32;
    < 0: the row is left untouched): ``desc`` int32 [slots, 4] = (state_base, n_states, eos, 0) into the arenas
    ``trans`` int16 [A, 256] (-1: no transition) and ``accept`` uint8 [A]; state ``n_states`` is the sink, entered
    by EOS from an accepting state, where only EOS is allowed. ``tok_off`` int32 [n_tok + 1] / ``tok_bytes`` uint8
    [B]: the vocabulary's bytes (length 0: never allowed; longer than GUIDE_MAX_TOKEN_BYTES: never allowed either;
    the kernel fetches eight bytes at a time and refuses a table with B < 8).
    ``cur`` / ``err`` int32 [slots], ``advance_ids`` and ``lm_part`` as in :func:`token_guide` (the same arrays: a
    slot belongs to one of the two ops)."""
    if not logits.is_cuda:
        return ref.byte_guide_rows(logits, slot, desc, trans, accept, tok_off, tok_bytes, cur, err, advance_ids,
                                   lm_part)
    _kern().byte_guide(logits, slot, desc, trans, accept, tok_off, tok_bytes, cur, err, advance_ids, lm_part)
    return logits


# JSON mode (launchers.h)
GUIDE_JSON_MAX_DEPTH = ref.GUIDE_JSON_MAX_DEPTH    # containers open at once: the stack is one 32-bit word
GUIDE_JSON_MAX_STATES = ref.GUIDE_JSON_MAX_STATES  # the pushdown table is always walked from LDS


def json_guide(logits: torch.Tensor, slot: torch.Tensor, desc: torch.Tensor, trans: torch.Tensor,
               tok_off: torch.Tensor, tok_bytes: torch.Tensor, cur: torch.Tensor, jstk: torch.Tensor,
               err: torch.Tensor, advance_ids: Optional[torch.Tensor] = None,
               lm_part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """JSON mode on ``logits`` [rows, vocab] bf16 IN PLACE: every token whose BYTES the byte pushdown automaton
    ``trans`` int16 [S, 256] cannot read from the row's configuration becomes ``-inf``, an allowed entry keeps its
    exact bits (:func:`reference.json_guide_rows` is the contract). An entry of ``trans`` is -1 or next state |
    action << 8 (0 none, 1 push-object, 2 push-array, 3 pop; a pop lands on its state field + 0 / 1 / 2 for an
    object on top / an array / depth 0). Row r uses ``slot[r]`` (int32; < 0: the row is left untouched): ``desc``
    int32 [slots, 4] = (n_states, done, eos, 0), the configuration is ``cur[slot]`` (``n_states``: the sink, entered
    by EOS from ``done``) with ``jstk`` int32 [slots, 2] = (depth, stack bits). ``tok_off`` / ``tok_bytes``,
    ``cur`` / ``err``, ``advance_ids`` and ``lm_part`` as in :func:`byte_guide` (the same arrays: a slot belongs to
    one of the three ops)."""
    if not logits.is_cuda:
        return ref.json_guide_rows(logits, slot, desc, trans, tok_off, tok_bytes, cur, jstk, err, advance_ids,
                                   lm_part)
    _kern().json_guide(logits, slot, desc, trans, tok_off, tok_bytes, cur, jstk, err, advance_ids, lm_part)
    return logits


# structured outputs (launchers.h)
GUIDE_SCHEMA_MAX_DEPTH = ref.GUIDE_SCHEMA_MAX_DEPTH        # return states live at once
GUIDE_SCHEMA_TOKEN_PUSHES = ref.GUIDE_SCHEMA_TOKEN_PUSHES  # a token's own pushes held at once
GUIDE_SCHEMA_STATE_ARENA = ref.GUIDE_SCHEMA_STATE_ARENA    # states shared by all slots: trans int32 [., 256] 16 MiB


def schema_guide(logits: torch.Tensor, slot: torch.Tensor, desc: torch.Tensor, trans: torch.Tensor,
                 accept: torch.Tensor, tok_off: torch.Tensor, tok_bytes: torch.Tensor, cur: torch.Tensor,
                 sdep: torch.Tensor, sstk: torch.Tensor, err: torch.Tensor,
                 advance_ids: Optional[torch.Tensor] = None, lm_part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Structured outputs on ``logits`` [rows, vocab] bf16 IN PLACE: every token whose BYTES the row's byte pushdown
    automaton cannot read from its configuration becomes ``-inf``, an allowed entry keeps its exact bits
    (:func:`reference.schema_guide_rows` is the contract). Row r uses ``slot[r]`` (int32; < 0: the row is left
    untouched): ``desc`` int32 [slots, 4] = (state_base, n_states, eos, 0) into the arenas ``trans`` int32 [A, 256]
    (-1, or next state | return state << 14 | action << 28: 0 none, 1 push, 2 pop) and ``accept`` uint8 [A]. The
    configuration is ``cur[slot]`` (``n_states``: the sink, entered by EOS from an accepting state at depth 0) with
    ``sdep`` int32 [slots], the depth, and ``sstk`` int16 [slots, 32], the return states (the oldest first; entries
    at or above the depth are never read). A push at depth 32, and a token's fifth own push that is still held, are
    no transition. ``tok_off`` / ``tok_bytes``, ``cur`` / ``err``, ``advance_ids`` and ``lm_part`` as in
    :func:`byte_guide` (the same arrays: a slot belongs to one of the four ops)."""
    if not logits.is_cuda:
        return ref.schema_guide_rows(logits, slot, desc, trans, accept, tok_off, tok_bytes, cur, sdep, sstk, err,
                                     advance_ids, lm_part)
    _kern().schema_guide(logits, slot, desc, trans, accept, tok_off, tok_bytes, cur, sdep, sstk, err, advance_ids,
                         lm_part)
    return logits


# embedding pooling (launchers.h): a segment descriptor's flag bits, and the row split of long mean segments
POOL_MEAN, POOL_FIRST, POOL_FINAL = 1, 2, 4
POOL_MAX_PARTS = 64    # workgroups per segment
POOL_PART_ROWS = 256   # rows per part (bench/micro_pool_embed.py: one workgroup alone reads ~90 GB/s)


def pool_parts(rows: int) -> int:
    """Into how many parts (workgroups) a mean segment of ``rows`` rows is split: POOL_PART_ROWS rows each, at most
    POOL_MAX_PARTS. 1: one workgroup, no scratch needed."""
    return max(1, min(POOL_MAX_PARTS, -(-int(rows) // POOL_PART_ROWS)))


def pool_segment(first: int, rows: int, slot: int = 0, total: int = 0, mean: bool = False, first_chunk: bool = True,
                 final: bool = True, part_base: int = 0, parts: int = 0) -> tuple:
    """One row of :func:`pool_embed`'s ``segs``. ``parts`` > 1 (mean only): the segment's rows are split over that
    many workgroups whose partial sums lie at rows [part_base, part_base + parts) of ``part``."""
    flags = (POOL_MEAN if mean else 0) | (POOL_FIRST if first_chunk else 0) | (POOL_FINAL if final else 0)
    return (int(first), int(rows), int(slot), int(total), flags, int(part_base), int(parts), 0)


def pool_embed(hidden: torch.Tensor, segs: torch.Tensor, acc: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, dims: int = 0, normalize: bool = True, scratch=None,
               max_parts: int = 1) -> torch.Tensor:
    """Pool the final-norm rows ``hidden`` bf16 [T, H] (row stride allowed) of a prefill step into one fp32 vector
    per segment, all segments in one launch -> ``out`` fp32 [S, H]. ``segs`` int32 [S, 8] on ``hidden``'s device,
    rows as :func:`pool_segment` builds them: (first row, rows, acc slot, total prompt length, flags, part base,
    parts). Without ``POOL_MEAN`` the vector is the segment's last row. With it, it is (``POOL_FIRST`` ? 0 :
    ``acc[slot]``) + the fp32 sum of the rows; a segment without ``POOL_FINAL`` stores that to ``acc[slot]`` (fp32
    [slots, H]) and leaves its row of ``out`` alone, one with it divides by ``total``. The vector is cut to its
    first ``dims`` components (0: all H; else a multiple of 8; the columns of ``out`` beyond stay as they are) and,
    with ``normalize``, divided by max(its L2 norm, 1e-12) as ``torch.nn.functional.normalize`` does. Rows outside
    every segment are never read. A descriptor that does not fit the tensors writes nothing.
    ``scratch`` = (part fp32 [P, H], tickets int32 [>= S], zero, re-armed by the kernel) and ``max_parts`` (>= the
    largest ``parts`` of a segment, <= POOL_MAX_PARTS) are needed when a segment has ``parts`` > 1; the result does
    not depend on which workgroup finishes last (the partials are combined in part order)."""
    dims = int(dims)
    s, (t, h) = segs.shape[0], hidden.shape
    if out is None:
        out = torch.zeros(s, h, dtype=torch.float32, device=hidden.device)
    if not hidden.is_cuda:
        if h % 8 or dims % 8 or not 0 <= dims <= h:
            raise RuntimeError("pool_embed: H and dims must be multiples of 8, dims <= H")
        return ref.pool_embed_rows(hidden, segs, acc, out, dims, normalize)
    part, tickets = scratch if scratch is not None else (None, None)
    _kern().pool_embed(out, acc, hidden, segs, dims, bool(normalize), part, tickets, int(max_parts))
    return out


def sample_advance(logits, temperature, top_k, top_p, seeds, steps, out, lm_part, ids, pos, ctx, slots, bt, tokens,
                   cnt, n_real, block_size: int, ticket, embed=None) -> torch.Tensor:
    """:func:`sample` from the LM head's candidates (``lm_part``) fused with :func:`decode_advance`: every row's
    workgroup also writes its token into the window's token row ``cnt[0]`` and advances the row's id / position /
    context / slot / step (``steps`` is read for the draw, then incremented); the last row bumps ``cnt[0]``.
    ``ticket``: int32 [1], zero, re-armed by the kernel (graph-capturable). ``embed`` = (table [V, H], h_out
    [>= rows, H], ssp_out [>= rows] fp32): also writes the next step's embedding rows of the advanced ids and their
    sums of squares, bit-identical to :func:`embed_sumsq`."""
    e = _empty(logits.device)
    table, h_out, ssp_out = embed if embed is not None else (e, e, e)
    _kern().sample_advance(out, logits, temperature, top_k, top_p, seeds, lm_part, ids, pos, ctx, slots, bt, steps,
                           tokens, cnt, n_real, block_size, ticket, table, h_out, ssp_out)
    return out


def copy_blocks(pool: torch.Tensor, pairs: torch.Tensor) -> None:
    """pool viewed [planes, num_blocks, ...]; pairs [n, 2] int64 (src, dst)."""
    if not pool.is_cuda:
        for s, d in pairs.tolist():
            pool[:, d] = pool[:, s]
        return
    _kern().copy_blocks(pool, pairs)


def gather_blocks(pool: torch.Tensor, ids: torch.Tensor, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pack blocks `ids` of every plane into [n, planes, slab] (KV transfer staging)."""
    planes, nb = pool.shape[0], pool.shape[1]
    slab = pool.numel() // (planes * nb)
    if buf is None:
        buf = torch.empty(ids.numel(), planes, slab, dtype=pool.dtype, device=pool.device)
    if not pool.is_cuda:
        buf.copy_(pool.reshape(planes, nb, slab)[:, ids.long()].transpose(0, 1))
        return buf
    _kern().move_blocks(pool, buf, ids, True)
    return buf


def gather_blocks_rows(pool: torch.Tensor, ids: torch.Tensor, dst: torch.Tensor, plane0: int, nplanes: int) -> None:
    """Planes [plane0, plane0 + nplanes) of pool blocks ``ids`` into the packet rows at device addresses ``dst``
    (int64, one per block; each row [planes, slab]) — the overlapped disaggregated export (LayerGroupExporter)."""
    _kern().gather_blocks_rows(pool, ids, dst, plane0, nplanes)


def scatter_blocks(pool: torch.Tensor, ids: torch.Tensor, buf: torch.Tensor) -> None:
    planes, nb = pool.shape[0], pool.shape[1]
    slab = pool.numel() // (planes * nb)
    if not pool.is_cuda:
        pool.view(planes, nb, slab)[:, ids.long()] = buf.view(ids.numel(), planes, slab).transpose(0, 1)
        return
    _kern().move_blocks(pool, buf, ids, False)


# expert-streaming grouped decode GEMM up to this many tokens (<= 128 rows per expert: 16/32/64/128-row
# images; above it: <= 128-row segments). 32 (round 1's limit) measured 14.9 vs 18.1 req/s at batch 64
MOE_DECODE_MAX_T = 128


def _decode_gemm_ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    return (x.is_cuda and 1 <= x.shape[0] <= DECODE_GEMM_MAX_M and x.shape[1] % 256 == 0
            and w.shape[0] % 16 == 0 and x.stride(1) == 1 and x.stride(0) % 8 == 0)


DECODE_GEMM_NT = True


def gemm_decode(x: torch.Tensor, w: torch.Tensor, mode: int = 0, wr: int = 64, sk: int = 1,
                out: Optional[torch.Tensor] = None, nt: Optional[bool] = None, kc: Optional[int] = None) -> torch.Tensor:
    """Raw access to the decode GEMM kernel (see csrc/kernels/gemm_decode.hip).
    ``mode``: a decode_tiles.MODE_* epilogue (MODE_BF16: bf16 x@w^T; MODE_SILU: bf16 silu(gate)*up, w = [gate; up];
    MODE_SLAB: fp32 split-K slabs [sk, M, N]), | TILED for a w packed by gd_pack_weights, or :func:`p13_mode`'s
    flags for one packed by gd_pack_weights_p13. ``(wr, kc)``: the workgroup tile (:func:`gd_tile`)."""
    m = x.shape[0]
    wr, kc = gd_tile(wr, kc)
    base = mode & MODE_MASK
    rows = w.shape[0] * P13_DEN // P13_NUM if mode & P13 else w.shape[0]
    n = rows // 2 if base == MODE_SILU else rows
    if out is None:
        if base == MODE_SLAB:
            out = torch.empty(sk, m, n, dtype=torch.float32, device=x.device)
        else:
            out = torch.empty(m, n, dtype=x.dtype, device=x.device)
    e = _empty(x.device)
    _kern().gemm_decode(out, x, w, mode, wr, kc, sk, DECODE_GEMM_NT if nt is None else nt, e, e, e, e, 0.0)
    return out


def p13_mode(base7: int) -> int:
    """The mode-word flags of a weight packed by gd_pack_weights_p13 with this base7."""
    return P13 | (int(base7) << P13_BASE_SHIFT)


def gd_swizzle(r: torch.Tensor, kc: int) -> torch.Tensor:
    """16-byte chunk swizzle of LDS-image row r for a K slot of kc elements (gemm_decode.hip swz())."""
    rowb = 2 * kc
    if rowb >= 256:
        return r & 15
    if rowb == 128:
        return (r >> 1) & 7
    return (r ^ (r >> 1)) & 3


def gd_pack_weights(w: torch.Tensor, wr: int, silu: bool = False, kc: Optional[int] = None) -> torch.Tensor:
    """Re-lay a [rows, K] projection weight in the decode GEMM's tile order: for column tile t and
    K-chunk c, the tile's (wr x KC) block is contiguous and already in the kernel's LDS-image order
    (rows of the tile, 16-byte chunks XOR-swizzled by row), so every 1-KiB LDS-DMA piece is one
    linear read. silu: w = [gate; up] and a tile holds wr/2 gate rows then the matching wr/2 up
    rows. The result has w's shape (pass mode | TILED to gemm_decode)."""
    rows, k = w.shape
    wrr, kc = gd_tile(wr, kc)
    cpr = kc // 8
    no = wrr // 2 if silu else wrr
    n_out = rows // 2 if silu else rows
    assert n_out % no == 0 and k % kc == 0
    nt, nch = n_out // no, k // kc
    t = torch.arange(nt, device=w.device).view(nt, 1) * no
    j = torch.arange(no, device=w.device).view(1, no)
    idx = torch.cat([t + j, n_out + t + j], 1) if silu else (t + torch.arange(wrr, device=w.device).view(1, wrr))
    wt = w[idx.reshape(-1)].view(nt, wrr, nch, cpr, 8)
    r = torch.arange(wrr, device=w.device).view(1, wrr, 1, 1, 1)
    q = torch.arange(cpr, device=w.device).view(1, 1, 1, cpr, 1)
    sw = (q ^ gd_swizzle(r, kc)).expand(nt, wrr, nch, cpr, 8)
    wt = torch.gather(wt, 3, sw)
    return wt.permute(0, 2, 1, 3, 4).contiguous().view(rows, k)


def gd_unpack_weights(wt: torch.Tensor, wr: int, kc: Optional[int] = None) -> torch.Tensor:
    """Inverse of :func:`gd_pack_weights` (plain projections, not the SiLU pairing): the row-major weight."""
    rows, k = wt.shape
    wrr, kc = gd_tile(wr, kc)
    cpr = kc // 8
    assert rows % wrr == 0 and k % kc == 0
    nt, nch = rows // wrr, k // kc
    w = wt.view(nt, nch, wrr, cpr, 8).permute(0, 2, 1, 3, 4)
    r = torch.arange(wrr, device=wt.device).view(1, wrr, 1, 1, 1)
    q = torch.arange(cpr, device=wt.device).view(1, 1, 1, cpr, 1)
    sw = (q ^ gd_swizzle(r, kc)).expand(nt, wrr, nch, cpr, 8)  # the XOR swizzle is its own inverse
    return torch.gather(w, 3, sw).contiguous().view(rows, k)


_EMPTY: dict = {}


def _empty(dev) -> torch.Tensor:
    t = _EMPTY.get(dev)
    if t is None:
        t = _EMPTY[dev] = torch.empty(0, device=dev)
    return t


def linear_slab_residual(x: torch.Tensor, w: torch.Tensor, resid: torch.Tensor, ssp_out: torch.Tensor,
                         counters: torch.Tensor, wr: int = 64, sk: int = 4, tiled: bool = False,
                         kc: Optional[int] = None, half_ring: bool = False) -> torch.Tensor:
    """resid += x @ w^T (bf16, in place) with split-K reduced by the last-arriving workgroup of
    each column tile, which also writes the tile's row sums of squares of the new residual to
    ssp_out [N/wr, SSP_LD] — the statistics of the next RMSNorm (whose weight is folded into the
    consuming projection). counters [N/wr] int32, zeroed once. Returns the slab scratch."""
    m, n = x.shape[0], w.shape[0]
    wr, kc = gd_tile(wr, kc)
    slab = torch.empty(sk, m, n, dtype=torch.float32, device=x.device)
    e = _empty(x.device)
    _kern().gemm_decode(slab, x, w, MODE_RESID | (TILED if tiled else 0) | (HALF_RING if half_ring else 0), wr, kc, sk,
                        DECODE_GEMM_NT, resid, ssp_out, counters, e, 0.0)
    return slab


_OCC: dict = {}


def gd_occupancy(mode: int, wr: int, kc: int, sk: int, rows: int, half_ring: bool = False) -> int:
    """Resident workgroups per CU of the decode-GEMM launch these parameters select
    (hipOccupancyMaxActiveBlocksPerMultiprocessor on that instantiation; 0 off the GPU or if none exists)."""
    if not native_available() or not torch.cuda.is_available():
        return 0
    key = (mode, wr, kc, sk, rows, half_ring)
    v = _OCC.get(key)
    if v is None:
        v = max(0, int(_kern().gd_occupancy(mode | (HALF_RING if half_ring else 0), wr, kc, sk, rows, DECODE_GEMM_NT)))
        _OCC[key] = v
    return v


def linear_silu_mul_rownorm(x: torch.Tensor, w_gate_up: torch.Tensor, ssp_in: torch.Tensor, eps: float,
                            wr: Optional[int] = None, tiled: bool = False, kc: Optional[int] = None, sk: int = 1,
                            slab: Optional[torch.Tensor] = None, counters: Optional[torch.Tensor] = None,
                            p13_base7: Optional[int] = None) -> torch.Tensor:
    """silu(r * x @ gate^T) * (r * x @ up^T) with r = rsqrt(sum_t ssp_in[t] / K + eps) per row:
    RMSNorm (weight folded into w_gate_up) + gate/up + SiLU*mul in one weight stream. sk > 1 (MODE_SILU_NORM_SK): K
    split over sk workgroups per tile with fp32 partials in ``slab`` (>= sk * rows * 2N floats) and the tile's
    last arriver finishing (``counters``: >= N / (wr / 2) int32, zero; re-armed by the kernel). ``p13_base7``:
    w_gate_up is the P13 form (gd_pack_weights_p13) with this base — tile (128, 128), <= 32 rows, sk = 1."""
    if p13_base7 is not None:
        n = w_gate_up.shape[0] * P13_DEN // P13_NUM // 2
        out = torch.empty(x.shape[0], n, dtype=x.dtype, device=x.device)
        e = _empty(x.device)
        _kern().gemm_decode(out, x, w_gate_up, MODE_SILU_NORM | p13_mode(p13_base7), *P13_TILE, 1, True, e, e, e,
                            ssp_in, float(eps))
        return out
    n = w_gate_up.shape[0] // 2
    if wr is None:
        wr, kc, _ = decode_tile(n, x.shape[1], MODE_SILU_NORM, decode_bucket(x.shape[0]))
    wr, kc = gd_tile(wr, kc)
    out = torch.empty(x.shape[0], n, dtype=x.dtype, device=x.device)
    e = _empty(x.device)
    if sk > 1:
        if slab is None or counters is None:
            raise ValueError("split-K gate/up (sk > 1) needs its slab and counters")
        _kern().gemm_decode(out, x, w_gate_up, MODE_SILU_NORM_SK | (TILED if tiled else 0), wr, kc, sk,
                            DECODE_GEMM_NT, e, slab, counters, ssp_in, float(eps))
        return out
    _kern().gemm_decode(out, x, w_gate_up, MODE_SILU_NORM | (TILED if tiled else 0), wr, kc, 1, DECODE_GEMM_NT, e, e, e,
                        ssp_in, float(eps))
    return out


def residual_add_sumsq(resid: torch.Tensor, x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """resid += x (bf16, in place); out [1, SSP_LD] = per-row sums of squares of the new residual."""
    if not x.is_cuda:
        resid.copy_((resid.float() + x.float()).to(resid.dtype))
        out.zero_()
        out[0, : x.shape[0]] = resid.float().pow(2).sum(-1)
        return out
    _kern().residual_add_sumsq(out, resid, x)
    return out


def embed_sumsq(ids: torch.Tensor, table: torch.Tensor, ssp: torch.Tensor, out: Optional[torch.Tensor] = None):
    """(table[ids] [M, H], ssp): the decode step's embedding gather and its per-row sums of squares (the first
    layer's RMSNorm statistics, ssp [1, SSP_LD]) in one launch."""
    if not table.is_cuda:
        h = torch.nn.functional.embedding(ids, table)
        if out is not None:
            h = out.copy_(h)
        return h, row_sumsq(h, out=ssp)
    h = out if out is not None else torch.empty(ids.shape[0], table.shape[1], dtype=table.dtype, device=table.device)
    _kern().embed_sumsq(h, ssp, table, ids)
    return h, ssp


def row_sumsq(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[1, SSP_LD] fp32 per-row sums of squares of x [M <= SSP_LD, H] (RMSNorm statistics)."""
    if out is None:
        out = torch.zeros(1, SSP_LD, dtype=torch.float32, device=x.device)
    if not x.is_cuda:
        out.zero_()
        out[0, : x.shape[0]] = x.float().pow(2).sum(-1)
        return out
    _kern().row_sumsq(out, x)
    return out


DECODE_GEMM_MAX_N = 262144


def linear(x: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x @ w^T. Decode-sized M (<= 128 rows) runs on the weight-streaming
    gfx950 kernel (gemm_decode.hip); larger M goes to hipBLASLt."""
    if _decode_gemm_ok(x, w) and w.shape[0] % 32 == 0 and w.shape[0] <= DECODE_GEMM_MAX_N:
        wr, kc, _ = decode_tile(w.shape[0], x.shape[1], MODE_BF16, decode_bucket(x.shape[0]))
        return gemm_decode(x, w, MODE_BF16, wr, 1, out, kc=kc)
    return torch.nn.functional.linear(x, w, out=out) if out is not None else torch.nn.functional.linear(x, w)


def linear_residual(resid: torch.Tensor, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """resid += x @ w^T in place through the library GEMM's C input (beta = 1): the prefill o / down projections
    add into the residual stream in their epilogue (fp32 accumulator + bf16 C, one rounding) instead of writing
    a [T, hidden] output that a separate pass reads back with the residual. Same TN signature as
    :func:`linear`, so the prefill GEMM table's solution applies. Prefill sizes only (the decode GEMM has its
    own residual epilogue, :func:`linear_slab_residual`)."""
    return resid.addmm_(x, w.t())


def linear_tiled(x: torch.Tensor, w: torch.Tensor, wr: int, kc: int) -> torch.Tensor:
    """y = x @ w^T (bf16, decode sizes) with w packed by gd_pack_weights for the (wr, kc) tile."""
    return gemm_decode(x, w, MODE_BF16 | TILED, wr, 1, kc=kc)


def linear_tiled_argmax(x: torch.Tensor, w: torch.Tensor, wr: int, kc: int, amax: torch.Tensor) -> torch.Tensor:
    """linear_tiled that also writes every wr-column tile's per-row greedy candidate (max of the bf16 outputs,
    lowest column on ties) into amax [M, N / wr, 2] int32 — the LM head's share of a decode step's argmax."""
    out = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
    _kern().gemm_decode_argmax(out, x, w, wr, kc, 1, amax)
    return out


def linear_p13_argmax(x: torch.Tensor, w: torch.Tensor, base7: int, amax: torch.Tensor) -> torch.Tensor:
    """:func:`linear_tiled_argmax` on a weight packed by gd_pack_weights_p13 (tile (128, 128), <= 32 rows)."""
    out = torch.empty(x.shape[0], w.shape[0] * P13_DEN // P13_NUM, dtype=x.dtype, device=x.device)
    _kern().gemm_decode_argmax(out, x, w, *P13_TILE, p13_mode(base7), amax)
    return out


def linear_slab(x: torch.Tensor, w: torch.Tensor, sk: Optional[int] = None, wr: Optional[int] = None,
                tiled: bool = False, kc: Optional[int] = None) -> torch.Tensor:
    """fp32 split-K slabs [sk, M, N] of x @ w^T (decode sizes only); the
    consumer (fused_add_rms_norm_slab / rope_and_cache_slab) reduces them.
    tiled: w was packed by gd_pack_weights for this (wr, kc)."""
    if sk is None or wr is None:
        assert not tiled, "a tiled weight needs its packing wr"
        wr0, kc0, sk0 = decode_tile(w.shape[0], x.shape[1], MODE_SLAB, decode_bucket(x.shape[0]))
        wr, sk, kc = wr or wr0, sk or sk0, kc or kc0
    return gemm_decode(x, w, MODE_SLAB | (TILED if tiled else 0), wr, sk, kc=kc)


def linear_silu_mul(x: torch.Tensor, w_gate_up: torch.Tensor) -> torch.Tensor:
    """silu(x @ gate^T) * (x @ up^T) with w_gate_up = [gate; up] (fused epilogue
    in the decode kernel; GEMM + silu_and_mul kernel otherwise)."""
    if _decode_gemm_ok(x, w_gate_up) and (w_gate_up.shape[0] // 2) % 32 == 0:
        wr, kc, _ = decode_tile(w_gate_up.shape[0] // 2, x.shape[1], MODE_SILU, decode_bucket(x.shape[0]))
        return gemm_decode(x, w_gate_up, MODE_SILU, wr, 1, kc=kc)
    return silu_and_mul(torch.nn.functional.linear(x, w_gate_up))


def fused_add_rms_norm_slab(slab: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """residual += slab.sum(0) (bf16, in place); returns rms_norm(residual) * w."""
    if not slab.is_cuda:
        return fused_add_rms_norm(slab.sum(0).to(residual.dtype), residual, w, eps, out)
    if out is None:
        out = torch.empty(residual.shape, dtype=residual.dtype, device=residual.device)
    _kern().fused_add_rms_norm_slab(out, slab, residual, w, eps)
    return out


def rope_and_cache_slab(slab, positions, cos_sin, slot_mapping, k_cache, v_cache, hq: int, hkv: int,
                        head_dim: int, q_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sum the QKV split-K slabs, rotate q/k, write k/v into the paged cache;
    returns q [T, hq*D] (bf16)."""
    t = slab.shape[1]
    if q_out is None:
        q_out = torch.empty(t, hq * head_dim, dtype=torch.bfloat16, device=slab.device)
    _kern().rope_and_cache_slab(q_out, slab, positions, cos_sin, slot_mapping, k_cache, v_cache, hq, hkv, head_dim)
    return q_out


def topk_softmax(gating: torch.Tensor, k: int, renorm: bool = True):
    if not gating.is_cuda:
        return ref.topk_softmax(gating, k, renorm)
    t = gating.shape[0]
    w = torch.empty(t, k, dtype=torch.float32, device=gating.device)
    ids = torch.empty(t, k, dtype=torch.int32, device=gating.device)
    _kern().topk_softmax(w, ids, gating, renorm)
    return w, ids


def moe_align(ids: torch.Tensor, num_experts: int):
    """Expert-sorted order of the flattened (token, slot) assignments."""
    n = ids.numel()
    dev = ids.device
    offsets = torch.empty(num_experts + 1, dtype=torch.int32, device=dev)
    sorted_idx = torch.empty(n, dtype=torch.int32, device=dev)
    pos = torch.empty(n, dtype=torch.int32, device=dev)
    _kern().moe_align(offsets, sorted_idx, pos, ids.reshape(-1).contiguous(), num_experts)
    return offsets, sorted_idx, pos


def expert_parallel_local(w: torch.Tensor, ids: torch.Tensor, expert0: int, n_local: int):
    """Expert parallelism over replicated tokens: keep the (token, slot) assignments routed to the
    local experts [expert0, expert0 + n_local) (ids rebased to 0..n_local-1) and send every other
    one to a null group ``n_local`` with weight 0 — no rows are computed for it, and the TP
    all-reduce after the MoE sums the experts' contributions across ranks. Plain tensor ops: no
    host sync, hipGraph-capturable."""
    local = (ids >= expert0) & (ids < expert0 + n_local)
    ids_l = torch.where(local, ids - expert0, torch.full_like(ids, n_local))
    return torch.where(local, w, torch.zeros_like(w)), ids_l.to(ids.dtype)


MOE_ROUTE_MAX_T = 256  # fused routing for decode-sized batches; larger ones: hipBLASLt gating GEMM


def moe_route(x: torch.Tensor, router: torch.Tensor, k: int, renorm: bool = True):
    """Routing weights and expert ids [T, k] from the activations and the router weights [E, H]: one
    fused launch (logits rounded to bf16, softmax, top-k) for decode-sized GPU batches; otherwise
    the router GEMM + :func:`topk_softmax`."""
    t, e = x.shape[0], router.shape[0]
    if x.is_cuda and t <= MOE_ROUTE_MAX_T and e <= 16 and x.shape[1] % 8 == 0 and x.stride(1) == 1 \
            and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0 and router.is_contiguous() \
            and router.data_ptr() % 16 == 0:
        w = torch.empty(t, k, dtype=torch.float32, device=x.device)
        ids = torch.empty(t, k, dtype=torch.int32, device=x.device)
        _kern().moe_route(w, ids, x, router, renorm)
        return w, ids
    return topk_softmax(torch.nn.functional.linear(x, router), k, renorm)


def moe_forward_routed(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor, w: torch.Tensor, ids: torch.Tensor,
                       expert0: Optional[int] = None, residual: Optional[torch.Tensor] = None,
                       ssp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`moe_forward` after routing (``w``, ``ids`` [T, k] over ALL routed experts). With
    ``residual``/``ssp``: residual += output and ssp[0, :T] = its row sums of squares (returns residual)."""
    e = w13.shape[0]
    if expert0 is not None:
        w, ids = expert_parallel_local(w, ids, expert0, e)
        return moe_apply(x, w13, w2, w, ids, e + 1, residual, ssp)
    return moe_apply(x, w13, w2, w, ids, e, residual, ssp)


def moe_forward(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor, gating: torch.Tensor, k: int,
                renorm: bool = True, expert0: Optional[int] = None) -> torch.Tensor:
    """Fused-routing MoE FFN on the HIP kernels: route → align → gather →
    grouped GEMM (gate/up) → SiLU·mul → grouped GEMM (down) → weighted combine.
    No host synchronisation (hipGraph-capturable). ``expert0``: expert parallelism — ``w13``/``w2``
    hold experts [expert0, expert0 + E_local) of the ``gating.shape[1]`` routed experts, and the
    output is this rank's partial sum (see :func:`expert_parallel_local`)."""
    w, ids = topk_softmax(gating, k, renorm)
    return moe_forward_routed(x, w13, w2, w, ids, expert0)  # EP: + the null group of remote assignments


def moe_apply(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor, w: torch.Tensor, ids: torch.Tensor,
              groups: int, residual: Optional[torch.Tensor] = None, ssp: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[t] = sum_j w[t, j] * expert_{ids[t, j]}(x[t]) for given routing (w [T, k] fp32, ids [T, k]
    int32). ``groups`` may exceed the number of local experts ``w13.shape[0]``: assignments to those
    extra groups are not computed (their weight must be 0)."""
    e = w13.shape[0]
    if residual is not None and not (x.is_cuda and x.shape[0] <= MOE_DECODE_MAX_T):
        return residual_add_sumsq(residual, moe_apply(x, w13, w2, w, ids, groups), ssp)
    if not x.is_cuda:
        return ref.moe_experts(x, w13, w2, w, ids)
    kern = _kern()
    t, hdim = x.shape
    k = ids.shape[1]
    inter = w13.shape[1] // 2
    ids = ids.to(torch.int32).contiguous()
    w = w.float().contiguous()
    offsets, sorted_idx, pos = moe_align(ids, groups)
    # rows of the extra groups are never computed: zero them so that weight 0 x row stays 0
    ys = (torch.zeros if groups > e else torch.empty)(t * k, hdim, dtype=x.dtype, device=x.device)
    x = x.contiguous()
    tiles = moe_decode_tiles(hdim, inter, t)
    if tiles is not None and t <= MOE_DECODE_MAX_T:
        # decode: every expert's weights streamed once by the weight-streaming kernel, its routed
        # tokens (<= t, so the activation image of the step's row bucket holds any expert's group)
        # riding along, gathered from x by the kernel itself through the sorted order; SiLU*mul
        # fused; idle experts read nothing
        (wr1, kc1), (wr2, kc2) = tiles
        a = torch.empty(t * k, inter, dtype=x.dtype, device=x.device)
        kern.gemm_decode_grouped(a, x, w13, offsets, MODE_SILU, wr1, kc1, sorted_idx, k, t, 1)
        kern.gemm_decode_grouped(ys, a, w2, offsets, MODE_BF16, wr2, kc2, _NO_ROWS(x.device), 1, t, 1)
        if residual is not None:  # combine + residual add + next-norm statistics in one launch
            kern.moe_combine_residual(ssp, residual, ys, pos, w)
            return residual
        out = torch.empty_like(x)
        kern.moe_combine(out, ys, pos, w)
        return out
    seg_tiles = moe_decode_tiles(hdim, inter, MOE_DECODE_MAX_T)
    capturing = torch.cuda.is_current_stream_capturing()
    if (t >= MOE_LIBRARY_MIN_TOKENS or seg_tiles is None) and not capturing:
        # prefill: the per-expert groups are thousands of rows — hipBLASLt GEMMs per expert at
        # ~1.5 PF/s; costs one host read of the offsets per layer
        xs = torch.empty(t * k, hdim, dtype=x.dtype, device=x.device)
        kern.moe_gather(xs, x, sorted_idx, k)
        off = offsets.tolist()
        for ei in range(e):
            a0, a1 = off[ei], off[ei + 1]
            if a1 > a0:
                act = silu_and_mul(torch.nn.functional.linear(xs[a0:a1], w13[ei]))
                torch.nn.functional.linear(act, w2[ei], out=ys[a0:a1])
    else:
        # between the decode path and the library path (and under graph capture): the expert-streaming
        # grouped GEMM with each expert's rows cut into segments of <= 128 (offsets built on the device,
        # no host read); an expert with r rows streams its weights ceil(r / 128) times
        if seg_tiles is None:
            raise ValueError(f"MoE shapes hidden={hdim} inter={inter} do not tile the grouped decode GEMM "
                             "(needed under graph capture)")
        (wr1, kc1), (wr2, kc2) = seg_tiles
        segs = (t + MOE_DECODE_MAX_T - 1) // MOE_DECODE_MAX_T
        j = torch.arange(segs, device=x.device, dtype=torch.int32) * MOE_DECODE_MAX_T
        off_v = torch.minimum(offsets[:-1, None] + j[None, :], offsets[1:, None]).reshape(-1)
        off_v = torch.cat([off_v, offsets[-1:]]).to(torch.int32).contiguous()
        a = torch.empty(t * k, inter, dtype=x.dtype, device=x.device)
        kern.gemm_decode_grouped(a, x, w13, off_v, MODE_SILU, wr1, kc1, sorted_idx, k, MOE_DECODE_MAX_T, segs)
        kern.gemm_decode_grouped(ys, a, w2, off_v, MODE_BF16, wr2, kc2, _NO_ROWS(x.device), 1, MOE_DECODE_MAX_T, segs)
    out = torch.empty_like(x)
    kern.moe_combine(out, ys, pos, w)
    if residual is not None:
        return residual_add_sumsq(residual, out, ssp)
    return out


MOE_LIBRARY_MIN_TOKENS = 256
_NO_ROWS_CACHE: dict = {}


def _NO_ROWS(device) -> torch.Tensor:
    """Empty int32 tensor: 'no gather' for gemm_decode_grouped (cached per device, graph-safe)."""
    t = _NO_ROWS_CACHE.get(device)
    if t is None:
        t = _NO_ROWS_CACHE[device] = torch.empty(0, dtype=torch.int32, device=device)
    return t
