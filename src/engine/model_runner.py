"""
Model runner: turns a scheduled step into GPU work on one HIP stream.

* Step inputs are assembled by the native step builder
  (``csrc/runtime/step_builder.h``) straight into pinned host buffers and
  shipped with one async H2D copy per buffer.
* Prefill steps run eagerly (ragged shapes; their GEMMs dominate anyway).
* Decode steps replay a **hipGraph** captured per padded batch size
  (``EngineConfig.graph_batch_sizes``): embedding → 32 layers of
  norm/GEMM/RoPE+KV-write/paged-attention → LM head → sampling is one graph
  launch, so host launch overhead (≈10 launches × 32 layers) disappears.
  The graph reads everything from static buffers; the decode attention grid
  is sized for ``max_model_len`` and idle workgroups exit immediately.
* Only the token ids (8 B per sequence) come back to the host each step.
"""

from __future__ import annotations

import bisect
import collections
import logging
import os
from typing import Dict, List, Optional, Sequence as Seq

import numpy as np
import torch

from src import ops
from src.config import EngineConfig
from src.engine.block_manager import native_runtime
from src.engine.scheduler import PrefillChunk
from src.engine.sequence import Sequence
from src.guided import (GUIDE_MAX_TOKEN_BYTES, Automaton, ByteGuide, FirstFit, JsonGuide, SchemaGuide, table_of,
                        walk)
from src.models.llama import AttnMetadata, CausalLM

logger = logging.getLogger(__name__)


class KVPool:
    """One HBM tensor for the whole KV cache:
    [layers, 2 (K,V), num_blocks, kv_heads, block_size, head_dim] (bf16)."""

    def __init__(self, num_layers: int, num_blocks: int, kv_heads: int, block_size: int, head_dim: int, device,
                 dtype=torch.bfloat16):
        self.shape = (num_layers, 2, num_blocks, kv_heads, block_size, head_dim)
        # zeroed once: a padded graph row reads block 0 before anything was written there, and
        # uninitialised bf16 can hold NaN bit patterns
        self.tensor = torch.zeros(self.shape, dtype=dtype, device=device)
        self.num_blocks = num_blocks
        self.block_size = block_size

    @property
    def nbytes(self) -> int:
        return self.tensor.numel() * self.tensor.element_size()

    def planes(self) -> torch.Tensor:
        """[layers*2, num_blocks, ...] view used by the block movers."""
        s = self.shape
        return self.tensor.view(s[0] * s[1], s[2], s[3], s[4], s[5])

    @staticmethod
    def bytes_per_block(num_layers: int, kv_heads: int, block_size: int, head_dim: int, dtype_bytes: int = 2) -> int:
        return num_layers * 2 * kv_heads * block_size * head_dim * dtype_bytes


class ModelRunner:
    mirrors_windows = False  # see supports_multistep
    # penalties / logit_bias (SamplingParams.processes_logits): per-sequence state on this runner's device; a
    # runner whose steps other ranks mirror would need mirrored state (TPModelRunner: False, the engine refuses)
    supports_logit_processing = True
    # constrained decoding (SamplingParams.guided): the automaton's state lives on this runner's device too
    supports_token_guide = True

    def __init__(self, model: CausalLM, pool: KVPool, cfg: EngineConfig, max_model_len: int):
        self.model = model
        self.pool = pool
        self.cfg = cfg
        self.device = model.device
        # prefill's last layer only for the sampled rows (CausalLM._last_layer_kept_rows)
        self.prune_last = True
        self.is_cuda = self.device.type == "cuda"
        self.bs = pool.block_size
        self.max_model_len = max_model_len
        self.bt_width = (max_model_len + self.bs - 1) // self.bs
        self.rt = native_runtime()
        self.max_seqs = cfg.max_num_seqs
        self.max_tokens = max(cfg.max_num_batched_tokens, self.max_seqs)
        pin = self.is_cuda
        i64, i32 = torch.int64, torch.int32
        # pinned host staging
        self.h_ids = torch.zeros(self.max_tokens, dtype=i64, pin_memory=pin)
        self.h_pos = torch.zeros(self.max_tokens, dtype=i64, pin_memory=pin)
        self.h_slots = torch.zeros(self.max_tokens, dtype=i64, pin_memory=pin)
        self.h_cu = torch.zeros(self.max_seqs + 1, dtype=i32, pin_memory=pin)
        self.h_ctx = torch.zeros(self.max_seqs, dtype=i32, pin_memory=pin)
        self.h_bt = torch.zeros(self.max_seqs, self.bt_width, dtype=i32, pin_memory=pin)
        self.h_last = torch.zeros(self.max_seqs, dtype=i64, pin_memory=pin)
        self.h_temp = torch.zeros(self.max_seqs, dtype=torch.float32, pin_memory=pin)
        self.h_topk = torch.zeros(self.max_seqs, dtype=i32, pin_memory=pin)
        self.h_topp = torch.ones(self.max_seqs, dtype=torch.float32, pin_memory=pin)
        self.h_seed = torch.zeros(self.max_seqs, dtype=i64, pin_memory=pin)
        self.h_step = torch.zeros(self.max_seqs, dtype=i64, pin_memory=pin)
        self.h_out = torch.zeros(self.max_seqs, dtype=i64, pin_memory=pin)
        self.k_max = max(1, int(getattr(cfg, "decode_window", 1)))
        # two halves of k_max rows: a window's tokens land in one half while the next (continuation)
        # window, already queued behind it, writes the other
        self.h_tokens = torch.zeros(2 * self.k_max, self.max_seqs, dtype=i64, pin_memory=pin)
        # continuation-window staging (block tables + first-step slots), double-buffered by parity: a
        # set is rewritten only after the window that read it has been waited for
        self.h_cbt = [torch.zeros(self.max_seqs, self.bt_width, dtype=i32, pin_memory=pin) for _ in range(2)]
        self.h_cslots = [torch.zeros(self.max_seqs, dtype=i64, pin_memory=pin) for _ in range(2)]
        self.h_cscratch = (torch.zeros(self.max_seqs, dtype=i64), torch.zeros(self.max_seqs, dtype=i32))
        self._cpar = 0
        self.inflight: Optional[Dict[str, object]] = None  # a queued window whose tokens are not yet read
        self.h_ctl = torch.zeros(2, dtype=i32, pin_memory=pin)   # [window step counter, real rows]
        # numpy views over the pinned buffers (zero-copy) for cheap bulk writes
        self.n_ids, self.n_temp, self.n_topk = self.h_ids.numpy(), self.h_temp.numpy(), self.h_topk.numpy()
        self.n_topp, self.n_seed, self.n_step = self.h_topp.numpy(), self.h_seed.numpy(), self.h_step.numpy()
        self._samp_key = None
        self._samp_dirty = False
        dev = self.device
        # device-side static buffers (graph inputs)
        self.d_ids = torch.zeros(self.max_tokens, dtype=i64, device=dev)
        self.d_pos = torch.zeros(self.max_tokens, dtype=i64, device=dev)
        self.d_slots = torch.zeros(self.max_tokens, dtype=i64, device=dev)
        self.d_cu = torch.zeros(self.max_seqs + 1, dtype=i32, device=dev)
        self.d_ctx = torch.ones(self.max_seqs, dtype=i32, device=dev)
        self.d_bt = torch.zeros(self.max_seqs, self.bt_width, dtype=i32, device=dev)
        self.d_last = torch.zeros(self.max_seqs, dtype=i64, device=dev)
        self.d_temp = torch.zeros(self.max_seqs, dtype=torch.float32, device=dev)
        self.d_topk = torch.zeros(self.max_seqs, dtype=i32, device=dev)
        self.d_topp = torch.ones(self.max_seqs, dtype=torch.float32, device=dev)
        self.d_seed = torch.zeros(self.max_seqs, dtype=i64, device=dev)
        self.d_step = torch.zeros(self.max_seqs, dtype=i64, device=dev)
        self.d_out = torch.zeros(self.max_seqs, dtype=i64, device=dev)
        # split greedy argmax scratch (ops.sample): per-slice (max, index) and per-row tickets, re-armed in-kernel
        self.d_samp = (torch.zeros(self.max_seqs * 32, dtype=torch.int32, device=dev),
                       torch.zeros(self.max_seqs, dtype=torch.int32, device=dev))
        self.d_tokens = torch.zeros(2 * self.k_max, self.max_seqs, dtype=i64, device=dev)
        self.d_ctl = torch.zeros(2, dtype=i32, device=dev)
        # per-token log-probabilities (ops.token_logprobs: logprob, rank, top logprobs, top ids), shaped like
        # d_tokens and written by a launch queued behind a step's graph replay — only for batches with a row
        # that asked (SamplingParams.logprobs); the pinned twins come back with h_tokens, only then
        top = ops.LOGPROBS_MAX_TOP
        lp_shapes = (((2 * self.k_max, self.max_seqs), torch.float32), ((2 * self.k_max, self.max_seqs), i32),
                     ((2 * self.k_max, self.max_seqs, top), torch.float32), ((2 * self.k_max, self.max_seqs, top), i32))
        self.d_lp = tuple(torch.zeros(s, dtype=t, device=dev) for s, t in lp_shapes)
        self.h_lp = tuple(torch.zeros(s, dtype=t, pin_memory=pin) for s, t in lp_shapes)
        self.graph_logits: Dict[int, torch.Tensor] = {}   # each captured graph's logits [pad, vocab] (kept alive)
        self._last_logits: Optional[torch.Tensor] = None  # of the latest _decode_forward
        self.logprob_launches = 0
        self.last_logprobs = None         # the latest call's logprobs (take_logprobs), None when no row asked
        self.last_prompt_logprobs = None  # the latest prefill's prompt logprobs: {chunk index: (positions, ...)}
        self.d_adv_ticket = torch.zeros(1, dtype=i32, device=dev)  # sample_advance's row ticket (re-armed in-kernel)
        # logit processing (ops.logit_process): row r of a step -> d_pen_slot[r] -> that sequence's state (-1: the
        # row did not ask, or is padding). The tables themselves are allocated by _pen_alloc when first needed.
        self.h_pen_slot = torch.full((self.max_seqs,), -1, dtype=i32, pin_memory=pin)
        self.d_pen_slot = torch.full((self.max_seqs,), -1, dtype=i32, device=dev)
        self.d_pen = None                       # (state, params, bias_cnt, bias_ids, bias_vals)
        self._pen_slots: Dict[int, int] = {}    # seq_id -> slot
        self._pen_free: List[int] = []
        self._pen_ev = None                     # the latest upload from the pinned staging buffers
        self.graphs_proc: Dict[int, torch.cuda.CUDAGraph] = {}  # the decode graphs with the ops.logit_process launch
        self.graph_logits_proc: Dict[int, torch.Tensor] = {}
        self.logit_process_launches = 0  # eager launches and processed graph replays
        self._proc = False                      # the step being assembled has a row that asks (_fill_sampling)
        # constrained decoding (ops.token_guide): row r -> d_guide_slot[r] -> that sequence's descriptor, current
        # state and error word; the automata themselves lie in two arenas shared by all slots, one region per
        # distinct spec (ref-counted; unreferenced regions stay until their room is needed). _guide_alloc
        # allocates the tables when first needed.
        self.h_guide_slot = torch.full((self.max_seqs,), -1, dtype=i32, pin_memory=pin)
        self.d_guide_slot = torch.full((self.max_seqs,), -1, dtype=i32, device=dev)
        self.d_guide = None                     # (desc, rowptr, edges, cur, err)
        # guided_regex over a multi-byte vocabulary (ops.byte_guide, launched directly behind ops.token_guide): the
        # byte DFA's rows live in a second pair of arenas, the vocabulary's bytes in one table per runner; slots,
        # descriptors, cur and err are the ones above. A row is in at most one of the two slot vectors.
        self.h_bguide_slot = torch.full((self.max_seqs,), -1, dtype=i32, pin_memory=pin)
        self.d_bguide_slot = torch.full((self.max_seqs,), -1, dtype=i32, device=dev)
        self.d_bguide = None                    # (trans, accept, tok_off, tok_bytes)
        self._bguide_st: Optional[FirstFit] = None
        self._bguide_table: Optional[int] = None  # guided.id_of the byte table that is on the device
        self.byte_guide_launches = 0            # eager launches and guided graph replays
        # JSON mode (ops.json_guide, launched directly behind ops.byte_guide): one pushdown table for all slots,
        # uploaded at the first such request, and a (depth, stack bits) pair per slot next to cur. The byte table,
        # slots, descriptors, cur and err are the ones above. A row is in at most one of the three slot vectors.
        self.h_jguide_slot = torch.full((self.max_seqs,), -1, dtype=i32, pin_memory=pin)
        self.d_jguide_slot = torch.full((self.max_seqs,), -1, dtype=i32, device=dev)
        self.d_jguide = None                    # (trans, jstk)
        self._jguide_up = False                 # the table is on the device
        self.json_guide_launches = 0            # eager launches and replays of the JSON graph set
        # structured outputs (ops.schema_guide, launched directly behind ops.json_guide): a schema's pushdown table
        # lives in a third pair of arenas (first fit, one region per distinct spec), a slot's depth and stack of
        # return states next to cur. The byte table, slots, descriptors, cur and err are the ones above. A row is in
        # at most one of the four slot vectors.
        self.h_sguide_slot = torch.full((self.max_seqs,), -1, dtype=i32, pin_memory=pin)
        self.d_sguide_slot = torch.full((self.max_seqs,), -1, dtype=i32, device=dev)
        self.d_sguide = None                    # (trans, accept, sdep, sstk)
        self._sguide_st: Optional[FirstFit] = None
        self.schema_guide_launches = 0          # eager launches and replays of the schema graph set
        self._guide_slots: Dict[int, int] = {}  # seq_id -> slot
        self._guide_free: List[int] = []
        self._guide_refs: Dict[int, tuple] = {}  # seq_id -> the spec key of the region it references
        self._guide_regions: Dict[tuple, dict] = {}  # spec key -> {"auto", "rp", "ed", "refs"}
        self._guide_lru: "collections.OrderedDict[tuple, None]" = collections.OrderedDict()  # unreferenced regions
        self._guide_rp: Optional[FirstFit] = None
        self._guide_ed: Optional[FirstFit] = None
        self._guide_ev = None
        self.graphs_guided: Dict[int, torch.cuda.CUDAGraph] = {}  # LM head -> logit_process -> token_guide -> byte_guide -> tail
        self.graph_logits_guided: Dict[int, torch.Tensor] = {}
        # a fourth set for batches with a JSON row: ... -> byte_guide -> json_guide -> tail (the guided set above stays
        # launch for launch what it was before JSON mode)
        self.graphs_json: Dict[int, torch.cuda.CUDAGraph] = {}
        self.graph_logits_json: Dict[int, torch.Tensor] = {}
        self._json = False                      # the step being assembled has a JSON row (_fill_guide)
        # a fifth set for batches with a schema row: ... -> byte_guide -> json_guide -> schema_guide -> tail (the four
        # sets above stay launch for launch what they were)
        self.graphs_schema: Dict[int, torch.cuda.CUDAGraph] = {}
        self.graph_logits_schema: Dict[int, torch.Tensor] = {}
        self._schema = False                    # the step being assembled has a schema row (_fill_guide)
        self.token_guide_launches = 0           # eager launches and guided graph replays
        self._guided = False                    # the step being assembled has a guided row (_fill_sampling)
        # embeddings (ops.pool_embed): requests with SamplingParams.pooling end with their prompt and return its
        # pooled final-norm hidden state. Mean pooling keeps its partial sums across chunks in an fp32 slot arena
        # [max_seqs, H]; arena, segment descriptors and output rows are allocated by _pool_alloc at the first such
        # request, so an engine nobody asks keeps its memory plan.
        self.d_pool = None                      # (acc, segs, out)
        self.h_pool = None                      # pinned (segs, out)
        self._pool_slots: Dict[int, int] = {}   # seq_id -> arena slot (mean pooling, while its prompt is in flight)
        self._pool_free: List[int] = []
        self.pool_embed_launches = 0
        # decode attention streams K/V as once-read data (DIE_ATTN_KV_ONCE=0: the default cache policy, for A/B)
        self.kv_once = os.environ.get("DIE_ATTN_KV_ONCE", "1") != "0"
        if self.is_cuda:
            maxp = ops.decode_partials(max_model_len)
            hq = model.hq
            self.part_o = torch.empty(self.max_seqs * hq * maxp * 128, dtype=torch.float32, device=dev)
            self.part_ml = torch.empty(self.max_seqs * hq * maxp * 2, dtype=torch.float32, device=dev)
            self.attn_cnt = torch.zeros(self.max_seqs * model.hkv, dtype=i32, device=dev)
            self.dec_scratch = (model.alloc_decode_scratch(self.max_seqs) if hasattr(model, "alloc_decode_scratch")
                                else None)
            # the LM head's per-column-tile greedy candidates (CausalLM.compute_logits(argmax_parts=...)): a greedy
            # row's argmax reduces those instead of re-reading its 128K logits (decode steps of <= 128 rows)
            parts = model.lm_head_argmax_parts() if hasattr(model, "lm_head_argmax_parts") else 0
            self.d_lmpart = torch.zeros(self.max_seqs, parts, 2, dtype=i32, device=dev) if parts else None
        else:
            self.part_o = self.part_ml = self.attn_cnt = self.dec_scratch = self.d_lmpart = None
        self.supports_swap = type(self)._sync_step is ModelRunner._sync_step
        # a runner whose steps are mirrored by other ranks (tensor parallelism) must mirror whole windows too:
        # it declares that with mirrors_windows (TPModelRunner sends one message per window, not per step)
        self.supports_multistep = self.is_cuda and self.k_max > 1 and (
            type(self)._sync_step is ModelRunner._sync_step or self.mirrors_windows)
        self.graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.graph_sizes: List[int] = []
        self._graph_pool = None
        self.stream = torch.cuda.current_stream(dev) if self.is_cuda else None

    # ------------------------------------------------------------ helpers
    def _h2d(self, n_tok: int, n_seq: int, with_cu: bool) -> None:
        nb = self.is_cuda
        self.d_ids[:n_tok].copy_(self.h_ids[:n_tok], non_blocking=nb)
        self.d_pos[:n_tok].copy_(self.h_pos[:n_tok], non_blocking=nb)
        self.d_slots[:n_tok].copy_(self.h_slots[:n_tok], non_blocking=nb)
        self.d_ctx[:n_seq].copy_(self.h_ctx[:n_seq], non_blocking=nb)
        self.d_bt[:n_seq].copy_(self.h_bt[:n_seq], non_blocking=nb)
        if with_cu:
            self.d_cu[: n_seq + 1].copy_(self.h_cu[: n_seq + 1], non_blocking=nb)
            self.d_last[:n_seq].copy_(self.h_last[:n_seq], non_blocking=nb)

    # --------------------------------------------------- logit processing
    def _pen_alloc(self) -> None:
        """The per-sequence tables of ops.logit_process (max_seqs x vocab uint16 counts, parameters, bias lists)
        and their pinned staging twins: at the first request that needs them — or at capture_graphs, whose
        processed graphs bake the tables' addresses in."""
        if self.d_pen is not None:
            return
        dev, pin, m = self.device, self.is_cuda, self.max_seqs
        v, nb = self.model.arch.vocab_size, ops.LOGIT_BIAS_MAX
        shapes = (((v,), torch.int16), ((4,), torch.float32), ((), torch.int32), ((nb,), torch.int32),
                  ((nb,), torch.float32))
        self.d_pen = tuple(torch.zeros((m,) + s, dtype=t, device=dev) for s, t in shapes)
        self.h_pen = tuple(torch.zeros(s, dtype=t, pin_memory=pin) for s, t in shapes)
        self._pen_free = list(range(m - 1, -1, -1))

    @staticmethod
    def _asks(seqs) -> bool:
        """THE predicate of the processed decode path: one of the rows set a penalty or a bias."""
        return any(s.sampling.processes_logits for s in seqs)

    def _pen_build(self, seq: Sequence, all_outputs: bool) -> int:
        """The sequence's slot. A sequence without one gets one and its state is built here from its token
        lists, whatever brought it (a fresh prompt, a recompute, a swap-in, a disaggregated import): prompt bits
        from the original prompt, counts from every output except the next decode step's input (the step counts
        that one itself) — all_outputs (a prefill step's sampled rows, where no such input exists): every output,
        and an existing slot is rebuilt (a decode row of a mixed step). The upload rides the compute stream, so
        a slot reused after a queued window is rewritten behind that window."""
        slot = self._pen_slots.get(seq.seq_id)
        if slot is not None and not all_outputs:
            return slot
        self._pen_alloc()
        if slot is None:
            slot = self._pen_free.pop()
            self._pen_slots[seq.seq_id] = slot
        if self._pen_ev is not None:  # the staging buffers' previous upload
            self._pen_ev.synchronize()
        sp = seq.sampling
        pre = list(getattr(seq, "_preempted_outputs", None) or ())
        prompt = seq.prompt_ids[: len(seq.prompt_ids) - len(pre)]
        outs = pre + (seq.output_ids if all_outputs else seq.output_ids[:-1])
        h_row, h_par, h_cnt, h_bid, h_bval = self.h_pen
        row = h_row.numpy().view(np.uint16)
        row.fill(0)
        if prompt:
            row[np.asarray(prompt, dtype=np.int64)] = 0x8000
        if outs:
            ids, cnt = np.unique(np.asarray(outs, dtype=np.int64), return_counts=True)
            row[ids] |= np.minimum(cnt, ops.LOGIT_COUNT_MAX).astype(np.uint16)
        rp = np.float32(sp.repetition_penalty)
        h_par.numpy()[:] = (rp, np.float32(1.0) / rp, sp.frequency_penalty, sp.presence_penalty)
        bias = sp.logit_bias or {}
        h_cnt.fill_(len(bias))
        if bias:
            h_bid.numpy()[:len(bias)] = list(bias.keys())
            h_bval.numpy()[:len(bias)] = list(bias.values())
        for h, d in zip(self.h_pen, self.d_pen):
            d[slot].copy_(h, non_blocking=self.is_cuda)
        if self.is_cuda:
            self._pen_ev = torch.cuda.Event()
            self._pen_ev.record(torch.cuda.current_stream(self.device))
        return slot

    def release_logit_state(self, seq: Sequence) -> None:
        """Give the sequence's slot back (finish, abort, preemption, swap-out). A window still queued may go on
        counting into it; whoever takes it next rewrites it behind that window (stream order)."""
        slot = self._pen_slots.pop(seq.seq_id, None)
        if slot is not None:
            self._pen_free.append(slot)

    def _fill_pen(self, seqs: Seq[Sequence], n_pad: int, all_outputs: bool, force: bool = False) -> bool:
        """d_pen_slot[:n_pad] for the step (-1: padding, and rows that did not ask); False and nothing written
        when no row asks — the raw graphs never read it. force (a guided step, whose graphs hold the
        ops.logit_process launch too): written even then, all -1."""
        asks = self._asks(seqs)
        if not asks and not force:
            return False
        if force:
            self._pen_alloc()
        n = len(seqs)
        ns = self.h_pen_slot.numpy()
        ns[:n] = [self._pen_build(s, all_outputs) if s.sampling.processes_logits else -1 for s in seqs]
        ns[n:n_pad] = -1
        self.d_pen_slot[:n_pad].copy_(self.h_pen_slot[:n_pad], non_blocking=self.is_cuda)
        return asks

    def _launch_logit_process(self, logits: torch.Tensor, n: int, count_ids=None, lm_part=None) -> None:
        ops.logit_process(logits, self.d_pen_slot[:n], *self.d_pen, count_ids=count_ids, lm_part=lm_part)
        self.logit_process_launches += 1

    # ------------------------------------------------ constrained decoding
    def _guide_alloc(self) -> None:
        """The tables of ops.token_guide (per-slot descriptor, current state, error word; the two arenas) and the
        arenas' host bookkeeping: at the first request that needs them — or at capture_graphs, whose guided
        graphs bake the tables' addresses in."""
        if self.d_guide is not None:
            return
        dev, m, i32 = self.device, self.max_seqs, torch.int32
        self.d_guide = (torch.zeros(m, 4, dtype=i32, device=dev),
                        torch.zeros(ops.GUIDE_ROWPTR_ARENA, dtype=i32, device=dev),
                        torch.zeros(ops.GUIDE_EDGE_ARENA, 2, dtype=i32, device=dev),
                        torch.zeros(m, dtype=i32, device=dev), torch.zeros(m, dtype=i32, device=dev))
        self.h_guide = torch.zeros(6, dtype=i32, pin_memory=self.is_cuda)      # one slot's desc, cur, err
        self.h_guide_err = torch.zeros(m, dtype=i32, pin_memory=self.is_cuda)  # err, read back with the tokens
        self._guide_free = list(range(m - 1, -1, -1))
        self._guide_rp, self._guide_ed = FirstFit(ops.GUIDE_ROWPTR_ARENA), FirstFit(ops.GUIDE_EDGE_ARENA)
        # ops.byte_guide: the state arenas, and room for the vocabulary's bytes (a token over the cap is stored cut
        # to one byte more than the cap, which bars it just the same)
        v = self.model.arch.vocab_size
        self.d_bguide = (torch.full((ops.GUIDE_BYTE_STATE_ARENA, 256), -1, dtype=torch.int16, device=dev),
                         torch.zeros(ops.GUIDE_BYTE_STATE_ARENA, dtype=torch.uint8, device=dev),
                         torch.zeros(v + 1, dtype=i32, device=dev),
                         torch.zeros(v * (GUIDE_MAX_TOKEN_BYTES + 1), dtype=torch.uint8, device=dev))
        self._bguide_st = FirstFit(ops.GUIDE_BYTE_STATE_ARENA)
        # ops.json_guide: the table, a slot's (depth, stack bits), and the pinned staging row of one slot's pair
        self.d_jguide = (torch.full((ops.GUIDE_JSON_MAX_STATES, 256), -1, dtype=torch.int16, device=dev),
                         torch.zeros(m, 2, dtype=i32, device=dev))
        self.h_jguide = torch.zeros(2, dtype=i32, pin_memory=self.is_cuda)
        # ops.schema_guide: the arenas, a slot's depth and return states, and the pinned staging of one slot's
        self.d_sguide = (torch.full((ops.GUIDE_SCHEMA_STATE_ARENA, 256), -1, dtype=i32, device=dev),
                         torch.zeros(ops.GUIDE_SCHEMA_STATE_ARENA, dtype=torch.uint8, device=dev),
                         torch.zeros(m, dtype=i32, device=dev),
                         torch.zeros(m, ops.GUIDE_SCHEMA_MAX_DEPTH, dtype=torch.int16, device=dev))
        self._sguide_st = FirstFit(ops.GUIDE_SCHEMA_STATE_ARENA)
        self.h_sguide = (torch.zeros(1, dtype=i32, pin_memory=self.is_cuda),
                         torch.zeros(ops.GUIDE_SCHEMA_MAX_DEPTH, dtype=torch.int16, pin_memory=self.is_cuda))

    @staticmethod
    def _guides(seqs) -> bool:
        """THE predicate of the guided decode path: one of the rows asked for constrained decoding."""
        return any(s.sampling.guided for s in seqs)

    def _mode(self, seqs) -> int:
        """Which graph set a decode batch replays: 4 guided with a schema row, 3 guided with a row in JSON mode, 2
        guided (a row is guided), 1 processed (a row set a penalty or a bias), 0 raw."""
        if any(s.sampling.guided_json is not None for s in seqs):
            return 4
        if any(s.sampling.guided_json_object for s in seqs):
            return 3
        return 2 if self._guides(seqs) else 1 if self._asks(seqs) else 0

    @torch.inference_mode()
    def guide_admit(self, seq: Sequence, auto) -> None:
        """Reference the arena region of the sequence's automaton, an Automaton, a ByteGuide, a JsonGuide or a SchemaGuide
        (LLMEngine.add_request: a ValueError here refuses the request). Sequences with the same spec share one
        region; a new one is uploaded first-fit, evicting unreferenced regions, least recently used first, until
        it fits."""
        self._guide_alloc()
        reg = self._guide_regions.get(auto.key)
        if isinstance(auto, (ByteGuide, JsonGuide, SchemaGuide)):
            self._bguide_vocab(auto)
        if reg is None and isinstance(auto, JsonGuide):
            # one table for every JSON request, uploaded once; the region entry takes no room in any arena (its key
            # "js" is neither "st" nor "rp": the eviction loops below never pick it)
            if not self._jguide_up:
                self.d_jguide[0][:auto.n_states].copy_(torch.from_numpy(auto.trans))
                self._jguide_up = True
            reg = self._guide_regions[auto.key] = {"auto": auto, "js": 0, "refs": 0}
        elif reg is None and isinstance(auto, SchemaGuide):
            n = auto.n_states
            while True:
                st = self._sguide_st.alloc(n)
                if st is not None:
                    break
                old = next((k for k in self._guide_lru if "sg" in self._guide_regions[k]), None)
                if old is None:
                    raise ValueError("no room for the request's guide: the constrained-decoding arena is full")
                del self._guide_lru[old]
                self._guide_drop(old)
            d_tr, d_ac, _, _ = self.d_sguide
            # on the compute stream: behind every queued window that may still read what lay here
            d_tr[st:st + n].copy_(torch.from_numpy(auto.trans))
            d_ac[st:st + n].copy_(torch.from_numpy(auto.accept))
            reg = self._guide_regions[auto.key] = {"auto": auto, "sg": st, "refs": 0}
        elif reg is None and isinstance(auto, ByteGuide):
            n = auto.n_states
            while True:
                st = self._bguide_st.alloc(n)
                if st is not None:
                    break
                old = next((k for k in self._guide_lru if "st" in self._guide_regions[k]), None)
                if old is None:
                    raise ValueError("no room for the request's guide: the constrained-decoding arena is full")
                del self._guide_lru[old]
                self._guide_drop(old)
            d_tr, d_ac, _, _ = self.d_bguide
            d_tr[st:st + n].copy_(torch.from_numpy(auto.trans))
            d_ac[st:st + n].copy_(torch.from_numpy(auto.accept))
            reg = self._guide_regions[auto.key] = {"auto": auto, "st": st, "refs": 0}
        elif reg is None:
            n_rp, n_ed = auto.n_states + 1, auto.n_edges
            while True:
                rp = self._guide_rp.alloc(n_rp)
                ed = self._guide_ed.alloc(n_ed) if rp is not None else None
                if ed is not None:
                    break
                if rp is not None:
                    self._guide_rp.release(rp, n_rp)
                old = next((k for k in self._guide_lru if "rp" in self._guide_regions[k]), None)
                if old is None:
                    raise ValueError("no room for the request's guide: the constrained-decoding arena is full")
                del self._guide_lru[old]
                self._guide_drop(old)
            _, d_rp, d_ed, _, _ = self.d_guide
            # on the compute stream: behind every queued window that may still read what lay here
            d_rp[rp:rp + n_rp].copy_(torch.from_numpy(auto.row_ptr))
            d_ed[ed:ed + n_ed].copy_(torch.from_numpy(np.stack([auto.edge_tok, auto.edge_next], axis=1)))
            reg = self._guide_regions[auto.key] = {"auto": auto, "rp": rp, "ed": ed, "refs": 0}
        self._guide_lru.pop(auto.key, None)
        reg["refs"] += 1
        self._guide_refs[seq.seq_id] = auto.key

    def _bguide_vocab(self, guide) -> None:
        """The vocabulary's bytes on the device: uploaded (on the compute stream, behind every queued window) when
        the first ByteGuide, JsonGuide or SchemaGuide arrives, and again only if the engine was paired with another byte table since — which
        is refused while a sequence still walks the old one."""
        tid = guide.key[-1]
        if tid == self._bguide_table:
            return
        if any("st" in self._guide_regions[k] or "js" in self._guide_regions[k] or "sg" in self._guide_regions[k]
               for k in self._guide_refs.values()):
            raise ValueError("guided_regex / guided_json_object / guided_json: the tokenizer's byte table changed "
                             "while guided requests are running")
        _, _, d_off, d_by = self.d_bguide
        v = d_off.shape[0] - 1
        table = table_of(tid)
        cut = [(table[t] or b"")[:GUIDE_MAX_TOKEN_BYTES + 1] if t < len(table) else b"" for t in range(v)]
        off = np.zeros(v + 1, dtype=np.int32)
        np.cumsum([len(b) for b in cut], out=off[1:])
        data = np.frombuffer(b"".join(cut), dtype=np.uint8)
        d_off.copy_(torch.from_numpy(off))
        if len(data):
            d_by[:len(data)].copy_(torch.from_numpy(data.copy()))
        self._bguide_table = tid

    def _guide_drop(self, key: tuple) -> None:
        reg = self._guide_regions.pop(key)
        if "js" in reg:  # the JSON table stays where it is
            return
        if "st" in reg:
            self._bguide_st.release(reg["st"], reg["auto"].n_states)
            return
        if "sg" in reg:
            self._sguide_st.release(reg["sg"], reg["auto"].n_states)
            return
        self._guide_rp.release(reg["rp"], reg["auto"].n_states + 1)
        self._guide_ed.release(reg["ed"], reg["auto"].n_edges)

    def _guide_build(self, seq: Sequence, all_outputs: bool) -> int:
        """The sequence's slot. A sequence without one gets one, and its state is rebuilt on the host, whatever
        brought it (a fresh prompt, a recompute, a swap-in, a disaggregated import): the automaton walked over
        every output except the next decode step's input (the step advances over that one itself) —
        all_outputs (a prefill step's sampled rows, which do not advance): over every output, and an existing
        slot is rebuilt (a decode row of a mixed step). The upload rides the compute stream."""
        slot = self._guide_slots.get(seq.seq_id)
        if slot is not None and not all_outputs:
            return slot
        reg = self._guide_regions[self._guide_refs[seq.seq_id]]
        if slot is None:
            slot = self._guide_free.pop()
            self._guide_slots[seq.seq_id] = slot
        if self._guide_ev is not None:  # the staging buffer's previous upload
            self._guide_ev.synchronize()
        auto = reg["auto"]
        pre = list(getattr(seq, "_preempted_outputs", None) or ())
        state = walk(auto, 0, pre + (seq.output_ids if all_outputs else seq.output_ids[:-1]))
        if "js" in reg:  # the configuration (state, depth, stack bits), by the device's rules (guided.walk_json)
            state, depth, bits = state
            self.h_guide.numpy()[:] = (auto.n_states, auto.done, auto.eos, 0, state, 0)
            self.h_jguide.numpy()[:] = (depth, bits - (1 << 32) if bits >= 1 << 31 else bits)
            self.d_jguide[1][slot].copy_(self.h_jguide, non_blocking=self.is_cuda)
        elif "sg" in reg:  # (state, depth, return states), by the device's rules (guided.walk_schema)
            state, depth, stack = state
            self.h_guide.numpy()[:] = (reg["sg"], auto.n_states, auto.eos, 0, state, 0)
            h_dep, h_stk = self.h_sguide
            h_dep[0] = depth
            h_stk.numpy()[:depth] = stack
            self.d_sguide[2][slot:slot + 1].copy_(h_dep, non_blocking=self.is_cuda)
            self.d_sguide[3][slot].copy_(h_stk, non_blocking=self.is_cuda)
        elif "st" in reg:
            self.h_guide.numpy()[:] = (reg["st"], auto.n_states, auto.eos, 0, state, 0)
        else:
            self.h_guide.numpy()[:] = (reg["rp"], auto.n_states, reg["ed"], auto.n_edges, state, 0)
        d_desc, _, _, d_cur, d_err = self.d_guide
        nb = self.is_cuda
        d_desc[slot].copy_(self.h_guide[0:4], non_blocking=nb)
        d_cur[slot:slot + 1].copy_(self.h_guide[4:5], non_blocking=nb)
        d_err[slot:slot + 1].copy_(self.h_guide[5:6], non_blocking=nb)
        if self.is_cuda:
            self._guide_ev = torch.cuda.Event()
            self._guide_ev.record(torch.cuda.current_stream(self.device))
        return slot

    def release_guide_state(self, seq: Sequence, keep_region: bool = False) -> None:
        """Give the sequence's slot back (finish, abort, preemption, swap-out) and, unless keep_region (a
        preempted sequence returns: its place in the arena was granted at add_request), its reference to the
        arena region; a region nobody references stays until its room is needed. A window still queued may go on
        advancing the slot; whoever takes it next rewrites it behind that window (stream order)."""
        slot = self._guide_slots.pop(seq.seq_id, None)
        if slot is not None:
            self._guide_free.append(slot)
        if keep_region:
            return
        key = self._guide_refs.pop(seq.seq_id, None)
        if key is not None:
            reg = self._guide_regions[key]
            reg["refs"] -= 1
            if reg["refs"] == 0:
                self._guide_lru[key] = None

    def guide_arena_edges_used(self) -> int:
        return self._guide_ed.used if self._guide_ed is not None else 0

    def guide_arena_states_used(self) -> int:
        """States of the byte guides held on the device (ops.byte_guide's arenas)."""
        return self._bguide_st.used if self._bguide_st is not None else 0

    def _fill_guide(self, seqs: Seq[Sequence], n_pad: int, all_outputs: bool) -> bool:
        """d_guide_slot[:n_pad], d_bguide_slot[:n_pad], d_jguide_slot[:n_pad] and d_sguide_slot[:n_pad] for the step (-1: padding, rows that
        are not guided, and in each vector the rows another kernel guides); False and nothing written when no row is guided — only
        the guided graphs read them."""
        self._json = self._schema = False
        if not self._guides(seqs):
            return False
        n = len(seqs)
        ns, nb, nj = self.h_guide_slot.numpy(), self.h_bguide_slot.numpy(), self.h_jguide_slot.numpy()
        nsg = self.h_sguide_slot.numpy()
        for i, s in enumerate(seqs):
            slot = self._guide_build(s, all_outputs) if s.sampling.guided else -1
            reg = self._guide_regions[self._guide_refs[s.seq_id]] if slot >= 0 else ()
            ns[i], nb[i], nj[i] = (-1, -1, slot) if "js" in reg else (-1, slot, -1) if "st" in reg else (slot, -1, -1)
            if "sg" in reg:
                ns[i], nsg[i] = -1, slot
            else:
                nsg[i] = -1
        ns[n:n_pad] = -1
        nb[n:n_pad] = -1
        nj[n:n_pad] = -1
        nsg[n:n_pad] = -1
        self._json = bool((nj[:n] >= 0).any())
        self._schema = bool((nsg[:n] >= 0).any())
        if self._schema:  # only the schema graphs read it: a batch without a schema row copies nothing more
            self.d_sguide_slot[:n_pad].copy_(self.h_sguide_slot[:n_pad], non_blocking=self.is_cuda)
        self.d_guide_slot[:n_pad].copy_(self.h_guide_slot[:n_pad], non_blocking=self.is_cuda)
        self.d_bguide_slot[:n_pad].copy_(self.h_bguide_slot[:n_pad], non_blocking=self.is_cuda)
        self.d_jguide_slot[:n_pad].copy_(self.h_jguide_slot[:n_pad], non_blocking=self.is_cuda)
        return True

    def _launch_token_guide(self, logits: torch.Tensor, n: int, advance_ids=None, lm_part=None,
                            json: Optional[bool] = None, schema: Optional[bool] = None) -> None:
        """ops.token_guide for the rows a CSR automaton guides and, directly behind it, ops.byte_guide for the rows
        a ByteGuide does and — json (default: the step has a JSON row, _fill_guide) — ops.json_guide for those in
        JSON mode and — schema (default: the step has a schema row) — ops.schema_guide for those a SchemaGuide
        guides; the workgroups of every other row exit at once in each."""
        desc, _, _, cur, err = self.d_guide
        ops.token_guide(logits, self.d_guide_slot[:n], *self.d_guide, advance_ids=advance_ids, lm_part=lm_part)
        self.token_guide_launches += 1
        ops.byte_guide(logits, self.d_bguide_slot[:n], desc, *self.d_bguide, cur, err, advance_ids=advance_ids,
                       lm_part=lm_part)
        self.byte_guide_launches += 1
        schema = self._schema if schema is None else schema
        _, _, tok_off, tok_bytes = self.d_bguide
        if self._json if json is None else json:  # (the schema graph set holds the JSON launch too: json = True)
            d_jtr, d_jstk = self.d_jguide
            ops.json_guide(logits, self.d_jguide_slot[:n], desc, d_jtr, tok_off, tok_bytes, cur, d_jstk, err,
                           advance_ids=advance_ids, lm_part=lm_part)
            self.json_guide_launches += 1
        if not schema:
            return
        d_str, d_sac, d_sdep, d_sstk = self.d_sguide
        ops.schema_guide(logits, self.d_sguide_slot[:n], desc, d_str, d_sac, tok_off, tok_bytes, cur, d_sdep, d_sstk,
                         err, advance_ids=advance_ids, lm_part=lm_part)
        self.schema_guide_launches += 1

    def _step_mode(self) -> int:
        """_mode of the step being assembled, from the flags _fill_sampling / _fill_guide left."""
        if not self._guided:
            return int(self._proc)
        return 4 if self._schema else 3 if self._json else 2

    def _guide_err_to_host(self) -> None:
        """Queue the sticky error words behind a guided step: they come back with its tokens."""
        if self.is_cuda:
            self.h_guide_err.copy_(self.d_guide[4], non_blocking=True)

    def guide_errors(self, seqs: Seq[Sequence]) -> List[tuple]:
        """(sequence, error bits) of the guided sequences whose slot reported an error in a step already read
        back (ops.GUIDE_ERR_*): the engine fails those requests."""
        if not self._guide_slots:
            return []
        err = self.h_guide_err if self.is_cuda else self.d_guide[4]
        out = []
        for s in seqs:
            slot = self._guide_slots.get(s.seq_id)
            if slot is not None and int(err[slot]):
                out.append((s, int(err[slot])))
        return out

    def _fill_sampling(self, seqs: Seq[Sequence], n_pad: int, prefill: bool = False) -> bool:
        """Write per-row sampling params; returns True when every row is greedy.
        Skips the H2D copies when the rows are all greedy (the kernel's greedy
        path ignores them) — the common decode case costs nothing here.
        Also maps the rows that ask for logit processing or constrained decoding to their slots (self._proc /
        self._guided: one of them does)."""
        self._guided = self._fill_guide(seqs, n_pad, all_outputs=prefill)
        # a guided decode step replays graphs that hold the ops.logit_process launch too: its slots must be current
        self._proc = self._fill_pen(seqs, n_pad, all_outputs=prefill, force=self._guided and not prefill)
        greedy = all(s.sampling.greedy for s in seqs)
        if greedy:
            key = ("greedy", n_pad)
            if self._samp_key == key:
                return True
            self.n_temp[:n_pad] = 0.0
            self.n_topk[:n_pad] = 0
            self.n_topp[:n_pad] = 1.0
            self._samp_key = key
        else:
            n = len(seqs)
            self.n_temp[:n] = [s.sampling.temperature for s in seqs]
            self.n_topk[:n] = [s.sampling.top_k for s in seqs]
            self.n_topp[:n] = [s.sampling.top_p for s in seqs]
            self.n_seed[:n] = [s.sampling.seed if s.sampling.seed is not None else s.seq_id for s in seqs]
            self.n_step[:n] = [len(s.output_ids) + len(getattr(s, "_preempted_outputs", ())) for s in seqs]
            self.n_temp[n:n_pad] = 0.0
            self.n_topk[n:n_pad] = 0
            self.n_topp[n:n_pad] = 1.0
            self._samp_key = None
        nb = self.is_cuda
        for h, d in ((self.h_temp, self.d_temp), (self.h_topk, self.d_topk), (self.h_topp, self.d_topp),
                     (self.h_seed, self.d_seed), (self.h_step, self.d_step)):
            d[:n_pad].copy_(h[:n_pad], non_blocking=nb)
        self._samp_dirty = True  # the device-side parameters changed since a TP leader last mirrored them
        return greedy

    def _sample(self, logits: torch.Tensor, n: int, greedy: bool, out: torch.Tensor) -> torch.Tensor:
        if greedy:
            return ops.sample(logits, out=out[:n], scratch=self.d_samp) if self.is_cuda else ops.sample(logits)
        args = (self.d_temp[:n], self.d_topk[:n], self.d_topp[:n], self.d_seed[:n], self.d_step[:n])
        return ops.sample(logits, *args, out=out[:n], scratch=self.d_samp) if self.is_cuda else ops.sample(logits, *args)

    def _to_host(self, ids: torch.Tensor, n: int) -> List[int]:
        if self.is_cuda:
            self.h_out[:n].copy_(ids[:n], non_blocking=True)
            self._queue_fault_readback()
            torch.cuda.current_stream(self.device).synchronize()
            self._raise_on_fault()
            return self.h_out[:n].tolist()
        return ids[:n].tolist()

    # ----------------------------------------------------------- logprobs
    @staticmethod
    def _lp_top(seqs) -> int:
        """-1 when no sequence asked for logprobs, else the largest number of top tokens any of them asked for."""
        top = -1
        for s in seqs:
            v = s.sampling.logprobs
            if v is not None and v > top:
                top = v
        return top

    def _launch_logprobs(self, logits: torch.Tensor, targets: torch.Tensor, n: int, row: int, top: int) -> None:
        """Queue ops.token_logprobs for the step's first n rows (targets: the ids just sampled) into row `row`
        of the logprob buffers."""
        ops.token_logprobs(logits[:n], targets[:n], top, out=tuple(d[row] for d in self.d_lp))
        self.logprob_launches += 1

    def _lp_to_host(self, lo: int, hi: int) -> None:
        for d, h in zip(self.d_lp, self.h_lp):
            h[lo:hi].copy_(d[lo:hi], non_blocking=self.is_cuda)

    def _lp_read(self, lo: int, hi: int, n: int, top: int) -> List[tuple]:
        """Per step: (logprobs [n], ranks [n], top logprobs [n][top], top ids [n][top]) from the host twins."""
        lp, rk, tl, ti = self.h_lp
        return [(lp[r, :n].tolist(), rk[r, :n].tolist(), tl[r, :n, :top].tolist(), ti[r, :n, :top].tolist())
                for r in range(lo, hi)]

    def take_logprobs(self):
        """The logprobs of the latest prefill / decode / decode_multi / decode_continue call (None when no row
        asked): one tuple per step as :meth:`_lp_read` gives them (prefill: one tuple over the sampled rows)."""
        r, self.last_logprobs = self.last_logprobs, None
        return r

    def _queue_fault_readback(self) -> None:
        """Queue device-side error words behind the step (read with the tokens, same sync). None on one GPU;
        the TP runner reads the one-shot collectives' sticky error word."""

    def _raise_on_fault(self) -> None:
        """Raise if an error word read by :meth:`_queue_fault_readback` is set."""

    # --------------------------------------------------------- embeddings
    def _pool_alloc(self) -> None:
        """The tables of ops.pool_embed (mean pooling's fp32 slot arena, segment descriptors, output rows, the row
        split's scratch) and their pinned twins: at the first request that needs them."""
        if self.d_pool is not None:
            return
        dev, pin, m, h = self.device, self.is_cuda, self.max_seqs, self.model.arch.hidden_size
        f32, i32 = torch.float32, torch.int32
        self.d_pool = (torch.zeros(m, h, dtype=f32, device=dev), torch.zeros(m, 8, dtype=i32, device=dev),
                       torch.zeros(m, h, dtype=f32, device=dev))
        # the row split of long mean segments (ops.pool_parts): at most one part per POOL_PART_ROWS rows of a step
        # and one more per segment; tickets are zero and re-armed by the kernel
        self.d_pool_scratch = (torch.zeros(self.max_tokens // ops.POOL_PART_ROWS + m, h, dtype=f32, device=dev),
                               torch.zeros(m, dtype=i32, device=dev)) if self.is_cuda else None
        self.h_pool = (torch.zeros(m, 8, dtype=i32, pin_memory=pin), torch.zeros(m, h, dtype=f32, pin_memory=pin))
        self._pool_free = list(range(m - 1, -1, -1))

    def release_pool_state(self, seq: Sequence) -> None:
        """Give a mean-pooling sequence's arena slot back (finish, abort, preemption: a recompute starts again at
        position 0 with POOL_FIRST)."""
        slot = self._pool_slots.pop(seq.seq_id, None)
        if slot is not None:
            self._pool_free.append(slot)

    def _pool_plan(self, chunks: List[PrefillChunk], pooled: List[int]):
        """The step's pooling segments, from the host's cu_q: (chunk index, mean, first row, rows) per segment —
        every chunk of a mean request, the completing chunk of a last request — grouped by (dimensions,
        normalize) so that each group is one launch."""
        cu = self.h_cu.numpy()
        plan = []
        for i in pooled:
            c = chunks[i]
            mean = c.seq.sampling.pooling == "mean"
            if mean or c.completes_prompt:
                plan.append((i, mean, int(cu[i]), c.length))
        plan.sort(key=lambda e: (chunks[e[0]].seq.sampling.embed_dimensions or 0,
                                 chunks[e[0]].seq.sampling.embed_normalize))
        return plan

    def _launch_pool_embed(self, hidden: torch.Tensor, chunks: List[PrefillChunk], plan, kept0: Optional[int]) -> None:
        """Queue the step's pooling launches behind its forward and the copy of their vectors to the pinned buffer.
        kept0 (a pruned last layer): hidden holds only the kept rows and the j-th last-pooling segment's row is
        kept0 + j, in plan order of the chunks; None: hidden holds every row of the step."""
        self._pool_alloc()
        d_acc, d_segs, d_out = self.d_pool
        h_segs, h_out = self.h_pool
        ns = h_segs.numpy()
        order = {i: j for j, i in enumerate(sorted(e[0] for e in plan if not e[1]))}
        groups, finals = [], []
        part_base = 0  # rows of the split scratch handed out in this step
        for k, (i, mean, row0, rows) in enumerate(plan):
            c = chunks[i]
            seq, sp = c.seq, c.seq.sampling
            parts = 1
            if mean:
                slot = self._pool_slots.get(seq.seq_id)
                if slot is None:
                    slot = self._pool_slots[seq.seq_id] = self._pool_free.pop()
                parts = ops.pool_parts(rows) if self.is_cuda else 1
                ns[k] = ops.pool_segment(row0, rows, slot, seq.prompt_len, True, c.start == 0, c.completes_prompt,
                                         part_base, parts)
                part_base += parts
                if c.completes_prompt:
                    finals.append(seq)
            elif kept0 is not None:
                ns[k] = ops.pool_segment(kept0 + order[i], 1)
            else:
                ns[k] = ops.pool_segment(row0, rows)
            key = (sp.embed_dimensions or 0, sp.embed_normalize)
            if not groups or groups[-1][0] != key:
                groups.append([key, k, k, 1])  # key, first segment, end, the widest split
            groups[-1][2], groups[-1][3] = k + 1, max(groups[-1][3], parts)
        # only now: a slot given back inside the loop could go to another segment of the same launch, whose
        # workgroup would write it while this one reads it. Whoever takes it later writes it behind this launch
        # (stream order).
        for seq in finals:
            self.release_pool_state(seq)
        n = len(plan)
        d_segs[:n].copy_(h_segs[:n], non_blocking=self.is_cuda)
        for (dims, norm), lo, hi, mp in groups:
            ops.pool_embed(hidden, d_segs[lo:hi], d_acc, d_out[lo:hi], dims=dims, normalize=norm,
                           scratch=self.d_pool_scratch, max_parts=mp)
            self.pool_embed_launches += 1
        h_out[:n].copy_(d_out[:n], non_blocking=self.is_cuda)

    def _pool_read(self, chunks: List[PrefillChunk], plan) -> None:
        """After the step's synchronise: the finished vectors onto their sequences."""
        h_out = self.h_pool[1].numpy()
        for k, (i, _, _, _) in enumerate(plan):
            c = chunks[i]
            if c.completes_prompt:
                d = c.seq.sampling.embed_dimensions or h_out.shape[1]
                c.seq.embedding = h_out[k, :d].copy()

    # ------------------------------------------------------------ prefill
    KIND_STOP, KIND_PREFILL, KIND_DECODE, KIND_HEARTBEAT = 0, 1, 2, 3

    def idle_tick(self) -> None:
        """Called by the engine loop while it has no work (TP runners send heartbeats)."""

    def _sync_step(self, kind: int, a: int = 0, b: int = 0, c: int = 0, d: int = 0) -> None:
        """Hook for tensor parallelism: rank 0 publishes the step to followers
        (see :class:`src.parallel.tp_runner.TPModelRunner`). No-op at TP=1."""

    def _sync_window(self, n: int, pad: int, k: int) -> None:
        """Hook: rank 0 publishes a k-step decode window (its first step's inputs, already in the host staging
        buffers; the graph advances them on every rank). No-op at TP=1."""

    def _sync_continuation(self, par: int, pad: int, k: int, base: int) -> None:
        """Hook: rank 0 publishes a continuation window queued behind the running one (the re-sent block tables
        and first-step slots of staging set ``par``, the token-row base). No-op at TP=1."""

    @torch.inference_mode()
    def prefill(self, chunks: List[PrefillChunk], kv_hook=None) -> List[Optional[int]]:
        """Run one ragged prefill batch — or a mixed step, whose decode rows are 1-token chunks —
        and return the sampled token for every chunk that completes its prompt or decodes
        (None for partial prompt chunks)."""
        toks = [c.tokens() for c in chunks]
        starts = [c.start for c in chunks]
        tables = [c.seq.block_table for c in chunks]
        n = len(chunks)
        t = self.rt.build_prefill_inputs(toks, starts, tables, self.bs, self.h_ids.data_ptr(),
                                         self.h_pos.data_ptr(), self.h_slots.data_ptr(), self.h_cu.data_ptr(),
                                         self.h_ctx.data_ptr(), self.h_bt.data_ptr(), self.bt_width,
                                         self.h_last.data_ptr())
        # chunks of embedding requests (SamplingParams.pooling) sample nothing: they are not in done
        pooled = [i for i, c in enumerate(chunks) if c.seq.sampling.pooling is not None]
        done = [i for i, c in enumerate(chunks)
                if c.completes_prompt and (not pooled or c.seq.sampling.pooling is None)]
        nd = len(done)
        pplan = self._pool_plan(chunks, pooled) if pooled else None
        # last pooling: the completing chunk's last row joins the kept rows of the last-layer pruning, after the
        # sampled rows; a mean chunk needs every row of the step
        kept = done + sorted(e[0] for e in pplan if not e[1]) if pplan else done
        pool_all = bool(pooled) and any(chunks[i].seq.sampling.pooling == "mean" for i in pooled)
        if kept and (len(kept) != n or pooled):
            nl = self.h_last.numpy()
            nl[:len(kept)] = nl[kept]
        greedy = self._fill_sampling([chunks[i].seq for i in done], nd, prefill=True) if nd else True
        proc = bool(nd) and self._proc
        guide = bool(nd) and self._guided
        lp_top = self._lp_top(chunks[i].seq for i in done) if nd else -1
        plan = self._prompt_logprob_plan(chunks)
        self.last_logprobs = self.last_prompt_logprobs = None
        self._h2d(t, n, with_cu=True)
        max_q = max(c.length for c in chunks)
        self._sync_step(self.KIND_PREFILL, t, n, max_q, nd)
        if not pooled:
            ids = self._exec_prefill(t, n, max_q, nd, greedy, kv_hook=kv_hook, lp_top=lp_top, plan=plan, process=proc,
                                     guide=guide)
        else:
            ids = self._exec_prefill(t, n, max_q, nd, greedy, kv_hook=kv_hook, lp_top=lp_top, plan=plan, process=proc,
                                     guide=guide, pool=(chunks, pplan, len(kept), pool_all))
        res: List[Optional[int]] = [None] * n
        if nd:
            if guide:
                self._guide_err_to_host()
            if lp_top >= 0:
                self._lp_to_host(0, 1)
            vals = self._to_host(ids, nd)
            for j, i in enumerate(done):
                res[i] = vals[j]
            if lp_top >= 0:  # row j of the launch belongs to chunk done[j]
                lp, rk, tl, ti = self._lp_read(0, 1, nd, lp_top)[0]
                full = ([None] * n, [None] * n, [None] * n, [None] * n)
                for j, i in enumerate(done):
                    full[0][i], full[1][i], full[2][i], full[3][i] = lp[j], rk[j], tl[j], ti[j]
                self.last_logprobs = [full]
        elif self.is_cuda:
            self._queue_fault_readback()
            torch.cuda.current_stream(self.device).synchronize()
            self._raise_on_fault()
        if pplan:
            self._pool_read(chunks, pplan)
        return res

    PROMPT_LOGPROB_SLAB = 1024  # rows of prompt logits at a time (<= 256 MiB of bf16 logits at a 128K vocabulary)

    @staticmethod
    def _prompt_logprob_plan(chunks: List[PrefillChunk]) -> List[tuple]:
        """For every prompt chunk of a request with prompt_logprobs: (chunk index, first row in the step's flat
        batch, first scored position, target ids, top-N). Row p (absolute position) scores prompt token p + 1 —
        the last row of a chunk that does not complete the prompt scores the first token of the next chunk; the
        row that completes the prompt samples instead. After a recompute preemption the prompt carries the earlier
        outputs at its end: only the original prompt is scored."""
        plan = []
        row0 = 0
        for i, c in enumerate(chunks):
            s = c.seq
            top = None if c.decode else s.sampling.prompt_logprobs
            if top is not None:
                orig = s.prompt_len - len(getattr(s, "_preempted_outputs", ()))
                last = min(c.start + c.length, orig - 1)  # rows [start, last) have a next prompt token
                if last > c.start:
                    plan.append((i, row0, c.start + 1, s.prompt_ids[c.start + 1: last + 1], int(top)))
            row0 += c.length
        return plan

    def _prompt_logprobs(self, hidden: torch.Tensor, plan: List[tuple]) -> dict:
        """{chunk index: (first position, logprobs, ranks, top logprobs, top ids)} from the step's hidden rows,
        PROMPT_LOGPROB_SLAB rows of logits at a time."""
        res = {}
        for i, row0, pos0, targets, top in plan:
            tg = torch.tensor(targets, dtype=torch.int64).to(self.device)
            parts = ([], [], [], [])
            for a in range(0, len(targets), self.PROMPT_LOGPROB_SLAB):
                b = min(len(targets), a + self.PROMPT_LOGPROB_SLAB)
                logits = self.model.compute_logits(hidden[row0 + a: row0 + b])
                out = ops.token_logprobs(logits, tg[a:b], top)
                self.logprob_launches += 1
                for acc, x in zip(parts, out):
                    acc.extend(x.tolist())
            res[i] = (pos0,) + parts
        return res

    def _exec_prefill(self, t: int, n: int, max_q: int, nd: int, greedy: bool, kv_hook=None, lp_top: int = -1,
                      plan: Optional[List[tuple]] = None, process: bool = False,
                      guide: bool = False, pool: Optional[tuple] = None) -> Optional[torch.Tensor]:
        # the last layer runs only for the sampled rows (CausalLM._last_layer_kept_rows; DIE_PRUNE_LAST=0: all);
        # a step that scores prompt tokens (prompt_logprobs) needs every row
        keep = self.d_last[:nd] if self.prune_last and not plan else None
        if pool is not None:
            return self._exec_prefill_pooled(t, n, max_q, nd, greedy, kv_hook, lp_top, plan, process, guide, pool)
        meta = AttnMetadata(is_prefill=True, slot_mapping=self.d_slots[:t], block_tables=self.d_bt[:n],
                            ctx_lens=self.d_ctx[:n], cu_q=self.d_cu[: n + 1], max_q_len=max_q, kv_hook=kv_hook,
                            keep_rows=keep)
        hidden = self.model.forward(self.d_ids[:t], self.d_pos[:t], meta, self.pool.tensor)
        if plan:
            self.last_prompt_logprobs = self._prompt_logprobs(hidden, plan)
        if not nd:
            return None
        if hidden.shape[0] != nd or plan:  # a path that computed every row (e.g. the slab path of small steps)
            hidden = hidden.index_select(0, self.d_last[:nd])
        logits = self.model.compute_logits(hidden)
        if process:  # penalties / bias of the rows that ask (their counts hold every output: nothing to count here)
            self._launch_logit_process(logits, nd)
        if guide:  # constrained rows: masked to their state's tokens (the state holds every output: no advance here)
            self._launch_token_guide(logits, nd)
        ids = self._sample(logits, nd, greedy, self.d_out)
        if lp_top >= 0:  # the first generated token's logprobs (the leader only: followers have nothing to report)
            self._launch_logprobs(logits, ids, nd, 0, lp_top)
        return ids

    def _exec_prefill_pooled(self, t: int, n: int, max_q: int, nd: int, greedy: bool, kv_hook, lp_top: int, plan,
                             process: bool, guide: bool, pool: tuple) -> Optional[torch.Tensor]:
        """_exec_prefill for a step with chunks of embedding requests: the kept rows are the nd sampled rows and,
        behind them, the last-pooling rows (d_last[:kn]); a mean chunk (pool_all) keeps every row, as a
        prompt_logprobs plan does, and so does a step whose rows are all kept. Only the first nd kept rows go to the
        LM head; a step without sampled rows skips it."""
        chunks, pplan, kn, pool_all = pool
        pruned = self.prune_last and not plan and not pool_all and kn != t
        meta = AttnMetadata(is_prefill=True, slot_mapping=self.d_slots[:t], block_tables=self.d_bt[:n],
                            ctx_lens=self.d_ctx[:n], cu_q=self.d_cu[: n + 1], max_q_len=max_q, kv_hook=kv_hook,
                            keep_rows=self.d_last[:kn] if pruned else None)
        hidden = self.model.forward(self.d_ids[:t], self.d_pos[:t], meta, self.pool.tensor)
        pruned = pruned and hidden.shape[0] != t  # a path that computed every row (the slab path of small steps)
        if plan:
            self.last_prompt_logprobs = self._prompt_logprobs(hidden, plan)
        if pplan:
            self._launch_pool_embed(hidden, chunks, pplan, nd if pruned else None)
        if not nd:
            return None
        hidden = hidden[:nd] if pruned else hidden.index_select(0, self.d_last[:nd])
        logits = self.model.compute_logits(hidden)
        if process:
            self._launch_logit_process(logits, nd)
        if guide:
            self._launch_token_guide(logits, nd)
        ids = self._sample(logits, nd, greedy, self.d_out)
        if lp_top >= 0:
            self._launch_logprobs(logits, ids, nd, 0, lp_top)
        return ids

    # ------------------------------------------------------------- decode
    def _fused_tail(self, n: int) -> bool:
        """Steps of n rows end in ONE launch that samples from the LM head's candidates, advances the inputs and
        gathers the next step's embedding rows (ops.sample_advance): then the step itself starts from them
        (AttnMetadata.pre_embedded) and the host writes them before the first step of a window (_pre_embed)."""
        return bool(self.supports_multistep and self.d_lmpart is not None and n <= ops.DECODE_GEMM_MAX_M
                    and self.model.lm_head_argmax_parts() == self.d_lmpart.shape[1]
                    and self.dec_scratch is not None and n <= self.dec_scratch["h_in"].shape[0])

    def _pre_embed(self, pad: int) -> None:
        if self._fused_tail(pad):
            sc = self.dec_scratch
            ops.embed_sumsq(self.d_ids[:pad], self.model.embed, sc["ssp0"], out=sc["h_in"][:pad])

    def _decode_forward(self, n: int, process: bool = False, guide: bool = False, json: bool = False,
                        schema: bool = False) -> torch.Tensor:
        tail = self._fused_tail(n)
        meta = AttnMetadata(is_prefill=False, slot_mapping=self.d_slots[:n], block_tables=self.d_bt[:n],
                            ctx_lens=self.d_ctx[:n], max_ctx=self.max_model_len, part_o=self.part_o,
                            part_ml=self.part_ml, attn_cnt=self.attn_cnt, kv_once=self.kv_once,
                            scratch=self.dec_scratch, pre_embedded=tail)
        hidden = self.model.forward(self.d_ids[:n], self.d_pos[:n], meta, self.pool.tensor)
        amax = (self.d_lmpart if self.d_lmpart is not None and n <= ops.DECODE_GEMM_MAX_M
                and self.model.lm_head_argmax_parts() == self.d_lmpart.shape[1] else None)
        logits = self.model.compute_logits(hidden, argmax_parts=amax) if amax is not None else \
            self.model.compute_logits(hidden)
        self._last_logits = logits  # ops.token_logprobs reads them behind the step (capture_graphs keeps each graph's)
        if process:
            # between the LM head and the sampling tail: counts this step's input ids (the previous samples), rewrites
            # the rows that ask in place and makes their greedy candidates agree with the rewritten rows
            self._launch_logit_process(logits, n, count_ids=self.d_ids[:n], lm_part=amax[:n] if amax is not None else None)
        if guide:
            # after the penalties and biases, so that no bias can lift a barred token: advances the guided rows'
            # automata over this step's input ids, masks the rows and makes their greedy candidates agree
            self._launch_token_guide(logits, n, advance_ids=self.d_ids[:n],
                                     lm_part=amax[:n] if amax is not None else None, json=json, schema=schema)
        if not self.is_cuda:
            return ops.sample(logits, self.d_temp[:n], self.d_topk[:n], self.d_topp[:n], self.d_seed[:n],
                              self.d_step[:n])
        if tail:
            # sampling from the LM head's candidates, the next step's input advance and its embedding rows in one launch
            sc = self.dec_scratch
            return ops.sample_advance(logits, self.d_temp[:n], self.d_topk[:n], self.d_topp[:n], self.d_seed[:n],
                                      self.d_step, self.d_out[:n], amax[:n], self.d_ids, self.d_pos, self.d_ctx,
                                      self.d_slots, self.d_bt, self.d_tokens, self.d_ctl[0:1], self.d_ctl[1:2],
                                      self.bs, self.d_adv_ticket,
                                      embed=(self.model.embed, sc["h_in"], sc["ssp0"].view(-1)))
        out = ops.sample(logits, self.d_temp[:n], self.d_topk[:n], self.d_topp[:n], self.d_seed[:n],
                         self.d_step[:n], out=self.d_out[:n], scratch=self.d_samp,
                         lm_part=amax[:n] if amax is not None else None)
        if self.supports_multistep:
            # next step's inputs from this step's samples, on the device (multi-step windows)
            ops.decode_advance(self.d_out, self.d_ids, self.d_pos, self.d_ctx, self.d_slots, self.d_bt, self.d_step,
                               self.d_tokens, self.d_ctl[0:1], self.d_ctl[1:2], n, self.bs)
        return out

    @torch.inference_mode()
    def capture_graphs(self) -> None:
        if not self.is_cuda or not self.cfg.use_cuda_graph:
            return
        sizes = sorted({min(b, self.max_seqs) for b in self.cfg.graph_batch_sizes} | {self.max_seqs})
        self._graph_pool = torch.cuda.graph_pool_handle()
        # warm up (hipBLASLt heuristics, kernel loads) outside capture
        for b in sizes:
            self.d_slots[:b].fill_(-1)
            self.d_ctx[:b].fill_(1)
            self._decode_forward(b)
        torch.cuda.synchronize(self.device)
        for b in reversed(sizes):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._graph_pool):
                self._decode_forward(b)
            self.graphs[b] = g
            # the graph's logits [b, vocab]: read by the logprob launch behind a replay; the reference also keeps
            # the shared pool from handing this memory to a graph captured later
            self.graph_logits[b] = self._last_logits
        torch.cuda.synchronize(self.device)
        if self.supports_logit_processing:
            # a second set with the ops.logit_process launch, for batches with a row that asks (_asks): the raw
            # set above is captured first and stays what it was
            self._pen_alloc()
            self.d_pen_slot.fill_(-1)
            for b in sizes:
                self._decode_forward(b, process=True)
            torch.cuda.synchronize(self.device)
            for b in reversed(sizes):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=self._graph_pool):
                    self._decode_forward(b, process=True)
                self.graphs_proc[b] = g
                self.graph_logits_proc[b] = self._last_logits
            torch.cuda.synchronize(self.device)
            self.logit_process_launches = 0  # warm-up and capture served no request
        if self.supports_logit_processing and self.supports_token_guide:
            # a third set, LM head -> ops.logit_process -> ops.token_guide -> ops.byte_guide -> the unchanged tail,
            # for batches with a guided row (_guides); rows that did not ask have slot -1 in all three kernels.
            # The two sets above stay exactly what they were. Behind it a fourth set with ops.json_guide behind
            # ops.byte_guide, replayed only by batches with a row in JSON mode: a guided batch without one pays
            # nothing for JSON mode (the idle launch measured +2 to +3 us per step in the third set).
            self._guide_alloc()
            self.d_pen_slot.fill_(-1)
            self.d_guide_slot.fill_(-1)
            self.d_bguide_slot.fill_(-1)
            self.d_jguide_slot.fill_(-1)
            for b in sizes:
                self._decode_forward(b, process=True, guide=True)
            torch.cuda.synchronize(self.device)
            for b in reversed(sizes):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=self._graph_pool):
                    self._decode_forward(b, process=True, guide=True)
                self.graphs_guided[b] = g
                self.graph_logits_guided[b] = self._last_logits
            torch.cuda.synchronize(self.device)
            for b in sizes:
                self._decode_forward(b, process=True, guide=True, json=True)
            torch.cuda.synchronize(self.device)
            for b in reversed(sizes):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=self._graph_pool):
                    self._decode_forward(b, process=True, guide=True, json=True)
                self.graphs_json[b] = g
                self.graph_logits_json[b] = self._last_logits
            torch.cuda.synchronize(self.device)
            # a fifth set with ops.schema_guide behind ops.json_guide, replayed only by batches with a schema row
            self.d_sguide_slot.fill_(-1)
            for b in sizes:
                self._decode_forward(b, process=True, guide=True, json=True, schema=True)
            torch.cuda.synchronize(self.device)
            for b in reversed(sizes):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=self._graph_pool):
                    self._decode_forward(b, process=True, guide=True, json=True, schema=True)
                self.graphs_schema[b] = g
                self.graph_logits_schema[b] = self._last_logits
            torch.cuda.synchronize(self.device)
            self.logit_process_launches = self.token_guide_launches = self.byte_guide_launches = 0
            self.json_guide_launches = self.schema_guide_launches = 0
        self.graph_sizes = sizes
        logger.info("captured decode hipGraphs for batch sizes %s", sizes)

    def _pad_for(self, n: int) -> int:
        if self.graphs:
            k = bisect.bisect_left(self.graph_sizes, n)
            if k < len(self.graph_sizes):
                return self.graph_sizes[k]
        return n

    @torch.inference_mode()
    def decode(self, seqs: List[Sequence]) -> List[int]:
        n = len(seqs)
        pad = self._pad_for(n)
        self.n_ids[:n] = [s.last_token for s in seqs]
        self.n_ids[n:pad] = 0
        self.rt.build_decode_inputs([s.block_table for s in seqs], [len(s) for s in seqs], self.bs,
                                    self.h_pos.data_ptr(), self.h_slots.data_ptr(), self.h_ctx.data_ptr(),
                                    self.h_bt.data_ptr(), self.bt_width, pad)
        self._fill_sampling(seqs, pad)
        self._h2d(pad, pad, with_cu=False)
        self._pre_embed(pad)  # the step starts from these rows when its tail launch writes the next ones
        if self.supports_multistep:  # the graph's input advance must see this step's real rows
            self.h_ctl[0] = 0
            self.h_ctl[1] = n
            self.d_ctl.copy_(self.h_ctl, non_blocking=True)
        self._sync_step(self.KIND_DECODE, n, pad)
        mode = self._step_mode()
        ids = self._exec_decode(n, pad, mode)
        if mode >= 2:
            self._guide_err_to_host()
        top = self._lp_top(seqs)
        self.last_logprobs = None
        if top < 0:
            return self._to_host(ids, n)
        glog = (self.graph_logits, self.graph_logits_proc, self.graph_logits_guided, self.graph_logits_json,
                self.graph_logits_schema)[mode]
        self._launch_logprobs(glog[pad] if pad in self.graphs else self._last_logits, ids, n, 0, top)
        self._lp_to_host(0, 1)
        toks = self._to_host(ids, n)
        self.last_logprobs = self._lp_read(0, 1, n, top)
        return toks

    @torch.inference_mode()
    def decode_multi(self, seqs: List[Sequence], k: int, k_next: int = 0) -> List[List[int]]:
        """k decode steps for the same batch in one host round trip: the step's hipGraph ends
        with a device-side input advance (sampled ids -> next ids, positions/context/step + 1,
        next slot from the block table), so the graph is replayed k times back to back and the
        k x n sampled tokens come back in one copy. The caller has reserved KV slots for the
        k positions. Falls back to single steps where no graph covers the batch.

        k_next > 1 (slots reserved for k + k_next positions): a continuation window of k_next
        steps is queued behind this one before the host waits, so the GPU runs it while the
        caller applies this window's tokens; :meth:`decode_continue` collects it."""
        n = len(seqs)
        pad = self._pad_for(n)
        g = self.graphs.get(pad)
        if k <= 1 or g is None or not self.supports_multistep:
            return [self.decode(seqs)]
        assert self.inflight is None, "a queued decode window must be collected first"
        k = min(k, self.k_max)
        self.n_ids[:n] = [s.last_token for s in seqs]
        self.n_ids[n:pad] = 0
        self.rt.build_decode_inputs([s.block_table for s in seqs], [len(s) for s in seqs], self.bs,
                                    self.h_pos.data_ptr(), self.h_slots.data_ptr(), self.h_ctx.data_ptr(),
                                    self.h_bt.data_ptr(), self.bt_width, pad)
        self._fill_sampling(seqs, pad)
        self._h2d(pad, pad, with_cu=False)
        self._pre_embed(pad)  # the step starts from these rows when its tail launch writes the next ones
        self.h_ctl[0] = 0
        self.h_ctl[1] = n
        self.d_ctl.copy_(self.h_ctl, non_blocking=True)
        self._sync_window(n, pad, k)
        top = self._lp_top(seqs)
        self._replay_window(pad, n, k, 0, top, self._step_mode())
        self._queue_fault_readback()
        if k_next > 1:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._queue_continuation(seqs, k, k_next, base=self.k_max)
            ev.synchronize()
        else:
            torch.cuda.current_stream(self.device).synchronize()
        self._raise_on_fault()
        self.last_logprobs = self._lp_read(0, k, n, top) if top >= 0 else None
        return self.h_tokens[:k, :n].tolist()

    def _replay_window(self, pad: int, n: int, k: int, base: int, top: int, mode: int) -> None:
        """k replays queued back to back, their tokens into rows [base, base + k); top >= 0 (a row asked for
        logprobs): one ops.token_logprobs launch behind each replay — it reads that step's logits and sampled ids
        before the next replay overwrites them (stream order) — and the logprob rows come back with the tokens.
        mode (_mode) 1, a row asks for logit processing: the graphs with the ops.logit_process launch and their
        logits; 2, a row is guided: the graphs with the ops.token_guide launch behind it, and the slots' error
        words come back with the tokens; 3, a row is in JSON mode: the same with the ops.json_guide launch too; 4, a
        row has a schema: the same with the ops.schema_guide launch behind that; 0: the raw graphs, launch for launch
        as without any of the features."""
        g = (self.graphs, self.graphs_proc, self.graphs_guided, self.graphs_json, self.graphs_schema)[mode][pad]
        if mode:
            self.logit_process_launches += k
        if mode >= 2:
            self.token_guide_launches += k
            self.byte_guide_launches += k
        if mode >= 3:
            self.json_guide_launches += k
        if mode == 4:
            self.schema_guide_launches += k
        if top < 0:
            for _ in range(k):
                g.replay()
            self.h_tokens[base:base + k].copy_(self.d_tokens[base:base + k], non_blocking=True)
            if mode >= 2:
                self._guide_err_to_host()
            return
        logits = (self.graph_logits, self.graph_logits_proc, self.graph_logits_guided, self.graph_logits_json,
                  self.graph_logits_schema)[mode][pad]
        for i in range(k):
            g.replay()
            self._launch_logprobs(logits, self.d_out, n, base + i, top)
        self.h_tokens[base:base + k].copy_(self.d_tokens[base:base + k], non_blocking=True)
        self._lp_to_host(base, base + k)
        if mode >= 2:
            self._guide_err_to_host()

    def _queue_continuation(self, seqs: List[Sequence], pending: int, k: int, base: int) -> None:
        """Queue k more decode steps for `seqs` behind a window of `pending` steps whose tokens the
        host has not applied yet (len(s) excludes them). Positions, context lengths and ids are
        already advanced on the device; the block tables (grown for the new positions) and the
        first step's slots (the queued window's last advance read the old tables) are re-sent."""
        n = len(seqs)
        pad = self._pad_for(n)
        k = min(k, self.k_max)
        par = self._cpar
        self._cpar ^= 1
        hbt, hsl = self.h_cbt[par], self.h_cslots[par]
        spos, sctx = self.h_cscratch
        self.rt.build_decode_inputs([s.block_table for s in seqs], [len(s) + pending for s in seqs], self.bs,
                                    spos.data_ptr(), hsl.data_ptr(), sctx.data_ptr(), hbt.data_ptr(),
                                    self.bt_width, pad)
        self.d_bt[:pad].copy_(hbt[:pad], non_blocking=True)
        self.d_slots[:pad].copy_(hsl[:pad], non_blocking=True)
        self.d_ctl[0:1].fill_(base)  # token rows [base, base + k)
        self._sync_continuation(par, pad, k, base)
        top = self._lp_top(seqs)
        self._replay_window(pad, n, k, base, top, self._mode(seqs))
        self._queue_fault_readback()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.inflight = {"seqs": list(seqs), "k": k, "base": base, "event": ev, "lp_top": top}

    def inflight_batch(self):
        """(sequences, steps) of the queued window, or None."""
        w = self.inflight
        return None if w is None else (w["seqs"], w["k"])

    @torch.inference_mode()
    def decode_continue(self, k_next: int = 0) -> List[List[int]]:
        """Collect the queued window's tokens ([k][n]); first, if k_next > 1 (the caller reserved
        the slots and the batch is unchanged), queue the next window behind it."""
        w = self.inflight
        assert w is not None
        self.inflight = None
        if k_next > 1:
            self._queue_continuation(w["seqs"], w["k"], k_next, base=self.k_max - w["base"])
        w["event"].synchronize()
        self._raise_on_fault()
        b, k, n = w["base"], w["k"], len(w["seqs"])
        self.last_logprobs = self._lp_read(b, b + k, n, w["lp_top"]) if w["lp_top"] >= 0 else None
        return self.h_tokens[b:b + k, :n].tolist()

    def _exec_decode(self, n: int, pad: int, mode: int = 0) -> torch.Tensor:
        g = self.graphs.get(pad)
        if g is not None:
            if mode:
                g = (self.graphs_proc, self.graphs_guided, self.graphs_json, self.graphs_schema)[mode - 1][pad]
                self.logit_process_launches += 1
                self.token_guide_launches += mode >= 2
                self.byte_guide_launches += mode >= 2
                self.json_guide_launches += mode >= 3
                self.schema_guide_launches += mode == 4
            g.replay()
            return self.d_out
        # eager: a guided step launches ops.logit_process only when a row asks for it
        return self._decode_forward(n, self._proc if mode >= 2 else bool(mode), mode >= 2, mode >= 3, mode == 4)
