"""Not a test: the float64 oracle of the Llama / Mixtral forward and everything the files that use it share.

* :class:`Oracle` — the model written plainly: RMSNorm with the unfolded gains, q / k / v, RoPE from the model's own
  ``cos_sin`` table taken as data, full causal attention with GQA over keys and values kept per sequence as plain
  lists, o, SiLU(gate) * up, down, the final norm and the LM head. No block tables, no buckets, nothing of
  ``src/ops/reference.py``. Per token it returns the taps ``hidden`` (final norm), ``resid`` (the residual stream
  after the last layer), ``logits`` and, per layer, ``kv<l>`` (K after RoPE and V, one row per kv head). Its
  mutations are switches (``MUTATIONS``): each is one wrong hand-off between two launches of a GPU path.
* the designed weight family (:func:`family_state_dict`) — HF-named tensors, every value a bf16 number: norm gains
  are powers of two per feature (folding them into bf16 weights is exact), every embedding row carries a
  power-of-two magnitude by ``token % 5`` (neighbouring rows of a script differ by >= 2x in their row scale), q / k
  x1.5 (llama-mini at two layers: x1; scores are not flat, x2 already took a 128-row case's bf16 reference past the
  cap), o / down x16 (the block outputs are comparable with the residual), gate / up x2, and an LM head in which
  the loudest tokens' rows point at the embedding of a permuted loud token (greedy steps have a clear winner).
* scripts (:class:`Script`) — named sequences with all tokens drawn in advance (decode steps are teacher-forced) and
  the way they are cut into steps: chunked prefill, the kept rows, which sequences decode together.
* :func:`run_paged` — the same script on a ``CausalLM`` through paged KV: sentinel-filled pool, scattered block
  tables, one ``forward`` per step, the taps read back (K / V through the block tables, the residual from the
  argument of the path's last norm launch), and the count of every ``src.ops`` entry point the step went through.
* the metric — per-row relative L2 error on each tap — and its tolerance: for each case and tap ``MARGIN`` x the
  worst row of the bf16 reference path (``reference_copy("cpu", torch.bfloat16)`` on the plain PyTorch ops) on the
  same case, computed on the CPU when the test runs, never from the code under test.
* ``CASES`` — every GPU case by name with the path it must take, its model variant and the mutations it claims to
  notice; ``COVERAGE`` — the paths and entries that the lists must cover.

Mixtral (arch ``moe``: mixtral-tiny). The oracle's MLP is then a plain MoE block (``Oracle._moe``) with two more taps
per layer and token, the chosen expert set and the K routing weights. Routing is discrete, so an MoE script's tokens
are chosen so that it is decided (``draw_decided``: redrawn until the K-th and (K+1)-th router logit are ROUTE_GAP
apart in every layer); ``moe_conditions`` then measures, on the CPU, that no (token, layer) pair of a case is closer
than GAP_FACTOR x the bf16 reference's largest router-logit deviation and that the bf16 reference chooses the
oracle's set everywhere. A run's sets are therefore compared exactly and its weights within a tolerance
(``routing_errors``). ``run_paged`` also counts the MoE entry points and, on the extension, the launches by which
``ops.moe_apply``'s three regimes differ; ``moe_expected_counts`` states them per step.
"""

from __future__ import annotations

import contextlib
import copy
import functools
import math
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from src import ops
from src.models.llama import AttnMetadata, CausalLM
from src.models.presets import get_preset
from tests import moe_reference as moer

BLOCK = 16
SENTINEL = 60.25  # a bf16 number no tap holds; finite, so a masked read of it is harmless
MAX_POS = 512

# tolerance = MARGIN x the bf16 reference path's worst row. 2 is the starting margin: the GPU chains round at other
# points (fp32 slabs where the reference rounds to bf16) and sum in other orders, both accumulations of the same
# order of bf16 roundings; a composition error moves a row by tens of percent.
MARGIN = 2.0
TOL_CAP = 0.06      # no case may have a larger tolerance on any tap
MUT_FACTOR = 4.0    # a claimed mutation moves rows beyond MUT_FACTOR x tol
MUT_ROWS = 8        # ... this many, or all the rows it affects in a smaller case
GAP_FACTOR = 8.0    # greedy steps are judged where the oracle's top-2 gap exceeds GAP_FACTOR x tol x |row|_inf

# MoE cases: a script's tokens are redrawn until the oracle's gap between the K-th and the (K+1)-th router logit
# exceeds ROUTE_GAP in every layer (the family's parameter, in logit units); test_model_reference_cpu.py then holds
# every (token, layer) of every case over GAP_FACTOR x the bf16 reference's largest router-logit deviation on it
ROUTE_GAP = 0.75

ARCHS = {"tiny": ("llama-tiny", {}), "mini": ("llama-mini", {"num_layers": 2}), "moe": ("mixtral-tiny", {})}

# the family's scales over the model's own init (std 0.02, o / down 0.02 / sqrt(2 L)); retuned per shape on the CPU:
# test_model_reference_cpu.py holds every case's tolerance under TOL_CAP and its mutations over MUT_FACTOR x tol
FAMILY = {"tiny": dict(q=1.5, k=1.5, v=1.0, o=16.0, down=16.0, gate_up=2.0, head_noise=0.1),
          "mini": dict(q=1.0, k=1.0, v=1.0, o=16.0, down=16.0, gate_up=2.0, head_noise=0.1),
          # mixtral-tiny: w1 / w3 / w2 as gate / up / down; router rows x2 (logits of standard deviation about 1.5:
          # the chosen pair changes from token to token and neither routing weight is negligible)
          # w2 x4: at x16 the 257-row case's bf16 reference went past the cap (0.088) and at x8 a 5-row decode
          # script did (0.075); at x4 no case is over 0.033, the router logits of the bf16 reference move by at
          # most 0.042 (ROUTE_GAP / GAP_FACTOR = 0.094) and every claimed mutation still clears MUT_FACTOR x tol
          "moe": dict(q=1.5, k=1.5, v=1.0, o=16.0, down=4.0, gate_up=2.0, router=2.0, head_noise=0.1)}


def arch_of(name: str):
    preset, over = ARCHS[name]
    return get_preset(preset, **over)


# ---------------------------------------------------------------------------------------------- the weight family
def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def family_state_dict(arch_name: str, seed: int = 5) -> Dict[str, torch.Tensor]:
    """The family as HF-named fp32 tensors holding bf16 numbers (so a bf16 model stores them exactly)."""
    a, sc = arch_of(arch_name), FAMILY[arch_name]
    g = torch.Generator().manual_seed(seed)
    h, d, L = a.hidden_size, a.head_dim, a.num_layers
    std, ostd = 0.02, 0.02 / math.sqrt(2 * L)

    def rnd(*shape, s):
        return _bf16(torch.randn(*shape, generator=g) * s)

    def gains():  # 2^[-1..2] per feature, another draw for every norm
        return torch.pow(2.0, torch.randint(-1, 3, (h,), generator=g).float())

    sd: Dict[str, torch.Tensor] = {}
    mag = torch.pow(2.0, (torch.arange(a.vocab_size) % 5 - 2).float())  # 2^[-2..2] by token % 5
    emb = _bf16(torch.randn(a.vocab_size, h, generator=g)) * mag[:, None]
    sd["model.embed_tokens.weight"] = emb
    for li in range(L):
        p = f"model.layers.{li}."
        sd[p + "input_layernorm.weight"] = gains()
        sd[p + "post_attention_layernorm.weight"] = gains()
        sd[p + "self_attn.q_proj.weight"] = rnd(a.num_heads * d, h, s=std * sc["q"])
        sd[p + "self_attn.k_proj.weight"] = rnd(a.num_kv_heads * d, h, s=std * sc["k"])
        sd[p + "self_attn.v_proj.weight"] = rnd(a.num_kv_heads * d, h, s=std * sc["v"])
        sd[p + "self_attn.o_proj.weight"] = rnd(h, a.num_heads * d, s=ostd * sc["o"])
        if a.is_moe:
            sd[p + "block_sparse_moe.gate.weight"] = rnd(a.num_experts, h, s=std * sc["router"])
            for x in range(a.num_experts):
                e = p + f"block_sparse_moe.experts.{x}."
                sd[e + "w1.weight"] = rnd(a.intermediate_size, h, s=std * sc["gate_up"])
                sd[e + "w3.weight"] = rnd(a.intermediate_size, h, s=std * sc["gate_up"])
                sd[e + "w2.weight"] = rnd(h, a.intermediate_size, s=ostd * sc["down"])
            continue
        sd[p + "mlp.gate_proj.weight"] = rnd(a.intermediate_size, h, s=std * sc["gate_up"])
        sd[p + "mlp.up_proj.weight"] = rnd(a.intermediate_size, h, s=std * sc["gate_up"])
        sd[p + "mlp.down_proj.weight"] = rnd(h, a.intermediate_size, s=ostd * sc["down"])
    sd["model.norm.weight"] = gains()
    # the LM head: noise, and among the tokens with the largest magnitude (loud: their embedding stands out in the
    # residual) row perm[t] also points at token t's embedding (unit length) over the final gain. After a loud token
    # t the greedy winner is perm[t], again loud, by a clear margin, and the walk does not repeat itself
    loud = torch.nonzero(torch.arange(a.vocab_size) % 5 == 4)[:, 0]
    perm = loud[torch.randperm(loud.numel(), generator=g)]
    unit = emb / emb.norm(dim=1, keepdim=True)
    head = torch.randn(a.vocab_size, h, generator=g) * (sc["head_noise"] / math.sqrt(h))
    head[perm] += unit[loud] / sd["model.norm.weight"][None, :]
    sd["lm_head.weight"] = _bf16(head * 0.25)
    return sd


def family_model(arch_name: str, device="cpu", dtype=torch.bfloat16, fold: bool = True) -> CausalLM:
    """A ``CausalLM`` holding the family, through the checkpoint path (``load_state_dict``, HF names)."""
    m = CausalLM(arch_of(arch_name), device, dtype=dtype, seed=1, max_position=MAX_POS)
    n = m.load_state_dict(family_state_dict(arch_name), fold=fold)
    assert n == len(family_state_dict(arch_name))
    return m


# ---------------------------------------------------------------------------------------------------------- scripts
@dataclass
class Step:
    prefill: bool
    rows: List[Tuple[str, int]]             # (sequence, tokens of it in this step), in batch order
    keep: Optional[List[str]] = None        # prefill: only the last rows of these sequences' chunks are returned


@dataclass
class Script:
    seqs: Dict[str, List[int]]
    steps: List[Step] = field(default_factory=list)

    def tokens(self) -> int:
        return sum(n for st in self.steps for _, n in st.rows)


def draw_tokens(rng: random.Random, vocab: int, seq_index: int, n: int) -> List[int]:
    """n tokens whose magnitude class differs between neighbouring positions and between neighbouring sequences at
    the same position (class = 2 (sequence + position) mod 5)."""
    out = []
    for p in range(n):
        t = rng.randrange(5, vocab - 5)
        out.append(t - t % 5 + (2 * (seq_index + p)) % 5)
    return out


def prefill_script(arch_name: str, chunks: List[List[Tuple[str, int]]], keeps=None, decode_steps: int = 0,
                   seed: int = 1) -> Script:
    """Sequences named in ``chunks`` (one list of (name, tokens) per prefill step), then ``decode_steps`` steps in
    which every sequence decodes one teacher-forced token."""
    rng = random.Random(seed)
    vocab = arch_of(arch_name).vocab_size
    total: Dict[str, int] = {}
    for st in chunks:
        for name, n in st:
            total[name] = total.get(name, 0) + n
    names = list(total)
    if arch_of(arch_name).is_moe:
        sc = Script(draw_decided(arch_name, rng, {name: total[name] + decode_steps for name in names}))
    else:
        sc = Script({name: draw_tokens(rng, vocab, i, total[name] + decode_steps) for i, name in enumerate(names)})
    for i, st in enumerate(chunks):
        sc.steps.append(Step(True, list(st), keeps[i] if keeps else None))
    for _ in range(decode_steps):
        sc.steps.append(Step(False, [(name, 1) for name in names]))
    return sc


def draw_decided(arch_name: str, rng: random.Random, lengths: Dict[str, int]) -> Dict[str, List[int]]:
    """Tokens of an MoE script, by rejection: the sequences are walked token by token through the float64 oracle
    (one row per unfinished sequence and round), and a token whose gap between the K-th and the (K+1)-th router
    logit is under ROUTE_GAP in some layer is drawn again, from the same stream and in the same magnitude class
    (``draw_tokens``). Routing is discrete: the inputs are chosen so that it is decided."""
    a = arch_of(arch_name)
    oracle = Oracle(family_weights(arch_name))
    names = list(lengths)
    seqs: Dict[str, List[int]] = {s: [] for s in names}
    state = oracle.begin(names)
    draws = 0
    while True:
        active = [s for s in names if len(seqs[s]) < lengths[s]]
        if not active:
            return seqs
        for s in active:
            t = rng.randrange(5, a.vocab_size - 5)
            seqs[s].append(t - t % 5 + (2 * (names.index(s) + len(seqs[s]))) % 5)
        draws += len(active)
        assert draws <= 64 * sum(lengths.values()), "ROUTE_GAP rejects nearly every token: retune the family"
        taps = oracle.run(Script(seqs), state, [Step(True, [(s, 1) for s in active])])
        gap = torch.stack([taps.moe[f"gap{li}"][0] for li in range(a.num_layers)]).min(0).values
        for s, ok in zip(active, (gap > ROUTE_GAP).tolist()):
            if not ok:
                oracle.rewind(state, s)
                seqs[s].pop()


def decode_contexts(n: int) -> List[int]:
    """Prompt lengths of a decode case with n rows, ragged within the step: the first decoded token sits at position
    15 (steps cross the block edge 15 -> 16), at 16 (16 -> 17), behind a context over 200, and at position 1 (a
    context of 2); the others are short."""
    rng = random.Random(100 + n)
    base = [15, 16, 205, 1]
    return base[:n] + [rng.randrange(2, 13) for _ in range(max(0, n - len(base)))]


def all_remote_steps(script: Script, world: int) -> List[Tuple[int, int]]:
    """(step, layer) of the 1-row decode steps whose chosen experts all live on one rank of ``world``: the other
    ranks compute nothing there (every assignment in the null group)."""
    a = arch_of("moe")
    per, want = a.num_experts // world, oracle_taps("moe", script)
    return [(i, li) for i, st in enumerate(script.steps) if not st.prefill and len(st.rows) == 1
            for li in range(a.num_layers) if len(set((want.moe[f"route{li}"][i][0] // per).tolist())) == 1]


def ep_remote_script() -> Script:
    """One sequence of 9 tokens and three 1-row decode steps, the first seed with an all-remote step."""
    for seed in range(300, 332):
        sc = prefill_script("moe", [[("s0", 9)]], decode_steps=3, seed=seed)
        if all_remote_steps(sc, 2):
            return sc
    raise AssertionError("no seed gives a 1-row step whose experts share a rank")


def decode_script(arch_name: str, n: int, steps: int = 3) -> Script:
    """Every caller gets a script of its own (one draw per (arch, rows, steps))."""
    return copy.deepcopy(_decode_script(arch_name, n, steps))


@functools.lru_cache(maxsize=None)
def _decode_script(arch_name: str, n: int, steps: int) -> Script:
    return prefill_script(arch_name, [[(f"s{i}", c) for i, c in enumerate(decode_contexts(n))]], decode_steps=steps,
                          seed=200 + n)


# ----------------------------------------------------------------------------------------------------------- oracle
MUTATIONS = (
    "rs_neighbour_qkv",      # the neighbouring token's row scale on q / k / v (layer 0)
    "rs_neighbour_mlp",      # ... on gate / up (layer 0)
    "fold_twice",            # gains applied twice in layer 0
    "fold_none",             # gains left out in layer 0
    "mlp_stats_pre_o",       # gate / up scaled by the statistics from before the o add (layer 0)
    "ssp0_prev_step",        # first-layer statistics from the previous step's embedding rows
    "pos_q_plus", "pos_q_minus", "pos_k_plus", "pos_k_minus",   # position +- 1 on q only / on k only
    "own_key_absent",        # the new token's own key is not attended to
    "kv_head_mod",           # kv head h % hkv instead of h // g
    "no_softmax_scale",
    "o_dropped", "o_doubled", "down_dropped", "down_doubled",   # in layer 0
    "final_norm_layer_gain",  # the final norm with the last layer's ln2
    "keep_first_row",        # keep_rows takes the first row of a sequence's chunk instead of the last
    "keep_neighbour_table",  # a kept row attends through its neighbour's block table
    "prefix_ignored",        # a chunk's cached prefix is not attended to
    # the MoE block (layer 0 unless said otherwise)
    "moe_router_raw",        # the router fed the un-normalised residual
    "moe_ln2_gain_off",      # ln2's gain left off (router and experts)
    "moe_no_renorm",         # the K weights not renormalised
    "moe_top1",              # only the first expert
    "moe_slots_swapped",     # the two slots' weights exchanged
    "moe_expert_plus1",      # expert id + 1
    "moe_w1_w3_swapped",     # SiLU on w3 x, times w1 x
    "moe_dropped", "moe_doubled",   # the MoE output in the residual
    "moe_stats_pre_add",     # layer 1's first statistics from before layer 0's MoE add
    # a group of W ranks (the oracle's ``world``); the full model stays the yardstick. Layer 0 where per layer
    "tp_o_dropped", "tp_o_doubled", "tp_down_dropped", "tp_down_doubled",   # rank 1's partial sum of o / down
    "tp_heads_next_o",       # rank r's heads against rank r + 1's o columns
    "tp_gate_next_up",       # gate rows of rank r with the up rows of rank r + 1
    "tp_next_kv_head",       # every rank attends to the kv head of rank r + 1
    "tp_vocab_reversed",     # the vocabulary shards gathered in reverse rank order
    "ep_unmasked",           # remote assignments not masked: every expert is counted W times
    "ep_next_expert0",       # the local expert index taken from rank r + 1's first expert
    "sp_rank_minor",         # the final rows gathered rank-minor
    "sp_pad_counted",        # the pad row counted in a real row's place (every row moves up by one)
)


class Weights:
    """float64 weights of one model, unfused: from the family's tensors (gains in the norms) or from a ``CausalLM``
    (whatever it holds: folded weights and unit gains after ``fold_norm_weights``)."""

    def __init__(self, arch, embed, layers, norm, lm_head, cos_sin):
        self.arch, self.embed, self.layers, self.norm, self.lm_head = arch, embed, layers, norm, lm_head
        self.cos_sin = cos_sin

    @classmethod
    def from_state_dict(cls, arch, sd, cos_sin):
        f = lambda t: t.detach().to("cpu", torch.float64)  # noqa: E731
        layers = []
        for li in range(arch.num_layers):
            p = f"model.layers.{li}."
            lw = dict(ln1=f(sd[p + "input_layernorm.weight"]), ln2=f(sd[p + "post_attention_layernorm.weight"]),
                      q=f(sd[p + "self_attn.q_proj.weight"]), k=f(sd[p + "self_attn.k_proj.weight"]),
                      v=f(sd[p + "self_attn.v_proj.weight"]), o=f(sd[p + "self_attn.o_proj.weight"]))
            if arch.is_moe:  # per expert: w1 (gate) / w3 (up) [inter, hidden], w2 (down) [hidden, inter]
                e = [p + f"block_sparse_moe.experts.{x}." for x in range(arch.num_experts)]
                lw.update(router=f(sd[p + "block_sparse_moe.gate.weight"]),
                          w1=torch.stack([f(sd[x + "w1.weight"]) for x in e]),
                          w3=torch.stack([f(sd[x + "w3.weight"]) for x in e]),
                          w2=torch.stack([f(sd[x + "w2.weight"]) for x in e]))
            else:
                lw.update(gate=f(sd[p + "mlp.gate_proj.weight"]), up=f(sd[p + "mlp.up_proj.weight"]),
                          down=f(sd[p + "mlp.down_proj.weight"]))
            layers.append(lw)
        return cls(arch, f(sd["model.embed_tokens.weight"]), layers, f(sd["model.norm.weight"]),
                   f(sd["lm_head.weight"]), f(cos_sin))

    @classmethod
    def from_model(cls, m: CausalLM):
        f = lambda t: t.detach().to("cpu", torch.float64)  # noqa: E731
        nq, nk, i = m.hq * m.head_dim, m.hkv * m.head_dim, m.inter
        layers = []
        for lw in m.layers:
            qkv = f(lw.qkv)
            d = dict(ln1=f(lw.ln1), ln2=f(lw.ln2), q=qkv[:nq], k=qkv[nq:nq + nk], v=qkv[nq + nk:], o=f(lw.o))
            if m.arch.is_moe:
                w13 = f(lw.w13)
                d.update(router=f(lw.router), w1=w13[:, :i], w3=w13[:, i:], w2=f(lw.w2))
            else:
                gu = f(lw.gate_up)
                d.update(gate=gu[:i], up=gu[i:], down=f(lw.down))
            layers.append(d)
        return cls(m.arch, f(m.embed), layers, f(m.norm), f(m.lm_head_rows()), f(m.cos_sin))


@functools.lru_cache(maxsize=None)
def family_weights(arch_name: str) -> Weights:
    a = arch_of(arch_name)
    from src.ops.reference import rope_cos_sin  # the table is data: the model's own, built the model's way

    return Weights.from_state_dict(a, family_state_dict(arch_name),
                                   rope_cos_sin(MAX_POS, a.head_dim, a.rope_theta, None, a.rope_scaling))


@dataclass
class Taps:
    """What a run returns. hidden / resid / logits: one tensor per step, rows in the order ``forward`` returns
    them; kv[sequence]: [layers, 2, tokens, kv heads, head_dim]."""
    hidden: List[torch.Tensor]
    resid: List[torch.Tensor]
    logits: List[torch.Tensor]
    kv: Dict[str, torch.Tensor]
    # MoE models, per layer l and step (rows: the tokens the layer's MoE block ran on, experts in index order):
    # "route<l>" the chosen experts [rows, K] int64, "rw<l>" their weights [rows, K]; from the oracle and from a
    # CPU reference run also "gl<l>", the router logits [rows, E]; from the oracle alone "gap<l>" [rows], the K-th
    # minus the (K+1)-th logit, and "rwtol<l>" [rows, K, 2]: the weight's own tolerance and its sensitivity to a
    # relative error of the router's input (rw_tolerance)
    moe: Dict[str, List[torch.Tensor]] = field(default_factory=dict)
    counts: List[Dict[str, int]] = field(default_factory=list)   # run_paged: launches per step
    pool: Optional[torch.Tensor] = None                          # run_paged: the pool after the run
    owned: Optional[torch.Tensor] = None                         # run_paged: bool [blocks, BLOCK] slots written


def _rope(x: torch.Tensor, pos: torch.Tensor, cos_sin: torch.Tensor) -> torch.Tensor:
    """x [T, heads, d], rotate-half form: (a, b) -> (a cos - b sin, b cos + a sin)."""
    half = x.shape[-1] // 2
    cs = cos_sin[pos]
    c, s = cs[:, None, :half], cs[:, None, half:]
    a, b = x[..., :half], x[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


class Oracle:
    def __init__(self, w: Weights, mutation: Optional[str] = None, world: int = 1):
        """``world``: the ranks of the group whose hand-offs a tp_ / ep_ / sp_ mutation gets wrong (the clean
        oracle does not depend on it)."""
        assert mutation is None or mutation in MUTATIONS, mutation
        assert world > 1 or mutation is None or mutation[:3] not in ("tp_", "ep_", "sp_"), mutation
        self.w, self.mut, self.world = w, mutation, world

    def begin(self, names) -> dict:
        """The state a run carries from step to step: every sequence's keys and values per layer, how many of its
        tokens are done, and the previous step's embedding rows."""
        L = self.w.arch.num_layers
        return dict(keys={s: [[] for _ in range(L)] for s in names}, vals={s: [[] for _ in range(L)] for s in names},
                    done={s: 0 for s in names}, prev_embed=None)

    @staticmethod
    def rewind(state: dict, name: str) -> None:
        """Take back the last token of one sequence (a draw that was rejected)."""
        state["done"][name] -= 1
        for per_layer in (state["keys"][name], state["vals"][name]):
            for lst in per_layer:
                lst.pop()

    def run(self, script: Script, state: Optional[dict] = None, steps: Optional[List[Step]] = None) -> Taps:
        """The whole script; or, with a ``state`` from :meth:`begin`, only ``steps``, carried on from it (the taps
        of those steps; K / V stay in the state)."""
        w, a, mut = self.w, self.w.arch, self.mut
        L, hq, hkv, d, eps = a.num_layers, a.num_heads, a.num_kv_heads, a.head_dim, a.rms_eps
        g = hq // hkv
        kvmap = [(h % hkv) if mut == "kv_head_mod" else h // g for h in range(hq)]
        W = self.world
        if mut == "tp_next_kv_head":  # head h lives on rank h // (hq / W); the next rank's first query head's kv head
            kvmap = [(((h // (hq // W) + 1) % W) * (hq // W)) // g for h in range(hq)]

        def partial_sum(act, wt, factor):
            """act @ wt^T summed over the W ranks' column shards, rank 1's partial times ``factor``."""
            n = wt.shape[1] // W
            return sum((act[:, r * n:(r + 1) * n] @ wt[:, r * n:(r + 1) * n].t()) * (factor if r == 1 else 1.0)
                       for r in range(W))
        scale = 1.0 if mut == "no_softmax_scale" else 1.0 / math.sqrt(d)
        whole = state is None
        state = self.begin(script.seqs) if whole else state
        keys, vals, done = state["keys"], state["vals"], state["done"]
        out = Taps([], [], [], {})
        prev_embed = state["prev_embed"]

        def stats(x):
            return torch.rsqrt(x.pow(2).mean(-1) + eps)

        def tap(name, t):
            out.moe.setdefault(name, []).append(t)

        for st in (script.steps if steps is None else steps):
            ids, pos, chunks = [], [], []
            for name, n in st.rows:
                p0 = done[name]
                chunks.append((name, len(ids), n, p0))
                ids += script.seqs[name][p0:p0 + n]
                pos += list(range(p0, p0 + n))
                done[name] = p0 + n
            pos_t = torch.tensor(pos)
            x = w.embed[torch.tensor(ids)].clone()
            embed_rows = x.clone()
            keep_rows = None
            if st.keep is not None:
                keep_rows = [(ci, (a0 if mut == "keep_first_row" else a0 + n - 1), a0 + n - 1)
                             for ci, (name, a0, n, _) in enumerate(chunks) if name in st.keep]
            x_pre_moe = None
            for li, lw in enumerate(w.layers):
                first = li == 0
                rs = stats(x_pre_moe if li == 1 and mut == "moe_stats_pre_add" else x)
                if first and mut == "ssp0_prev_step" and prev_embed is not None:
                    m = min(len(ids), prev_embed.shape[0])
                    rs[:m] = stats(prev_embed[:m])
                g1, g2 = lw["ln1"], lw["ln2"]
                if first and mut == "fold_twice":
                    g1, g2 = g1 * g1, g2 * g2
                if first and mut == "fold_none":
                    g1, g2 = torch.ones_like(g1), torch.ones_like(g2)
                rs_q = torch.roll(rs, 1) if first and mut == "rs_neighbour_qkv" else rs
                xn = x * rs_q[:, None] * g1
                q = (xn @ lw["q"].t()).view(-1, hq, d)
                k = (xn @ lw["k"].t()).view(-1, hkv, d)
                v = (xn @ lw["v"].t()).view(-1, hkv, d)
                dq = {"pos_q_plus": 1, "pos_q_minus": -1}.get(mut, 0)
                dk = {"pos_k_plus": 1, "pos_k_minus": -1}.get(mut, 0)
                q = _rope(q, (pos_t + dq).clamp(min=0), w.cos_sin)
                k = _rope(k, (pos_t + dk).clamp(min=0), w.cos_sin)
                attn = torch.zeros(len(ids), hq, d, dtype=torch.float64)
                for name, a0, n, p0 in chunks:  # the chunk's keys join its sequence's lists, then it attends
                    for r in range(n):
                        keys[name][li].append(k[a0 + r])
                        vals[name][li].append(v[a0 + r])
                for ci, (name, a0, n, p0) in enumerate(chunks):
                    kk, vv = torch.stack(keys[name][li]), torch.stack(vals[name][li])   # [p0 + n, hkv, d]
                    qpos = torch.arange(p0, p0 + n)[:, None]
                    kpos = torch.arange(p0 + n)[None, :]
                    allowed = kpos <= qpos
                    if mut == "prefix_ignored" and p0 > 0:
                        allowed = allowed & (kpos >= p0)
                    if mut == "own_key_absent":
                        allowed = allowed & ((kpos != qpos) | (qpos == 0))
                    attn[a0:a0 + n] = self._attend(q[a0:a0 + n], kk, vv, allowed, kvmap, scale)
                if mut == "keep_neighbour_table" and keep_rows and li == L - 1:
                    for ci, _, row in keep_rows:
                        nb = chunks[(ci + 1) % len(chunks)][0]
                        kk, vv = torch.stack(keys[nb][li]), torch.stack(vals[nb][li])
                        allowed = torch.ones(1, kk.shape[0], dtype=torch.bool)
                        attn[row:row + 1] = self._attend(q[row:row + 1], kk, vv, allowed, kvmap, scale)
                if first and mut == "tp_heads_next_o":
                    attn = torch.roll(attn, -(hq // W), 1)
                if first and mut in ("tp_o_dropped", "tp_o_doubled"):
                    o = partial_sum(attn.reshape(len(ids), hq * d), lw["o"], 0.0 if mut == "tp_o_dropped" else 2.0)
                else:
                    o = attn.reshape(len(ids), hq * d) @ lw["o"].t()
                x_pre = x
                x = x + o * ({"o_dropped": 0.0, "o_doubled": 2.0}.get(mut, 1.0) if first else 1.0)
                rs2 = stats(x_pre if first and mut == "mlp_stats_pre_o" else x)
                if first and mut == "rs_neighbour_mlp":
                    rs2 = torch.roll(rs2, 1)
                if first and mut == "moe_ln2_gain_off":
                    g2 = torch.ones_like(g2)
                xn = x * rs2[:, None] * g2
                if "router" in lw:
                    # the rows the layer's MoE block runs on in a model: all, or the kept ones in the last layer
                    sel = None
                    if keep_rows is not None and li == L - 1:
                        sel = torch.tensor([r for _, r, _ in keep_rows], dtype=torch.long)
                    x_pre_moe = x
                    y = self._moe(lw, xn, x if first and mut == "moe_router_raw" else xn, mut if first else None,
                                  lambda name, t, li=li, sel=sel: tap(f"{name}{li}", t if sel is None else t[sel]))
                    if first and mut == "ep_unmasked":
                        y = y * W
                    x = x + y * ({"moe_dropped": 0.0, "moe_doubled": 2.0}.get(mut, 1.0) if first else 1.0)
                    continue
                up = xn @ lw["up"].t()
                if first and mut == "tp_gate_next_up":
                    up = torch.roll(up, -(up.shape[1] // W), 1)
                act = torch.nn.functional.silu(xn @ lw["gate"].t()) * up
                if first and mut in ("tp_down_dropped", "tp_down_doubled"):
                    x = x + partial_sum(act, lw["down"], 0.0 if mut == "tp_down_dropped" else 2.0)
                    continue
                x = x + (act @ lw["down"].t()) * ({"down_dropped": 0.0, "down_doubled": 2.0}.get(mut, 1.0)
                                                  if first else 1.0)
            gain = w.layers[-1]["ln2"] if mut == "final_norm_layer_gain" else w.norm
            hidden = x * stats(x)[:, None] * gain
            if keep_rows is not None:
                sel = torch.tensor([r for _, r, _ in keep_rows], dtype=torch.long)
                x, hidden = x[sel], hidden[sel]
            if mut in ("sp_rank_minor", "sp_pad_counted") and st.prefill:
                T = hidden.shape[0]
                n = -(-T // W)
                padded = torch.cat([hidden, hidden.new_zeros(n * W - T, hidden.shape[1])])
                if mut == "sp_rank_minor":   # row i of rank r lands at i W + r
                    hidden = padded.view(W, n, -1).transpose(0, 1).reshape(n * W, -1)[:T]
                elif n * W > T:
                    hidden = padded[1:T + 1]
            logits = hidden @ w.lm_head.t()
            if mut == "tp_vocab_reversed":
                logits = torch.cat(list(logits.chunk(W, -1))[::-1], -1)
            out.hidden.append(hidden)
            out.resid.append(x)
            out.logits.append(logits)
            prev_embed = state["prev_embed"] = embed_rows
        for s in script.seqs if whole else ():
            if done[s]:
                out.kv[s] = torch.stack([torch.stack([torch.stack(keys[s][li]), torch.stack(vals[s][li])])
                                         for li in range(L)])
        return out

    def _moe(self, lw, xn, router_in, mut, tap):
        """The MoE block on the normalised rows xn [T, hidden]: router logits, the K largest (descending logit, the
        lowest index among equals: moe_reference.py's rule), a softmax over all experts renormalised over the K,
        and per expert SiLU(w1 x) * (w3 x) through w2, combined with the weights."""
        E, K = self.w.arch.num_experts, self.w.arch.top_k
        gl = router_in @ lw["router"].t()
        order = torch.sort(gl, dim=-1, descending=True, stable=True).indices
        ids = order[:, :K]
        wk = torch.softmax(gl, -1).gather(-1, ids)
        if mut != "moe_no_renorm":
            wk = wk / wk.sum(-1, keepdim=True)
        if mut == "moe_top1":
            ids, wk = ids[:, :1], torch.ones_like(wk[:, :1])
        if mut == "moe_slots_swapped":
            wk = wk.flip(-1)
        if mut == "moe_expert_plus1":
            ids = (ids + 1) % E
        if mut == "ep_next_expert0":
            ids = (ids + E // self.world) % E
        w1, w3 = (lw["w3"], lw["w1"]) if mut == "moe_w1_w3_swapped" else (lw["w1"], lw["w3"])
        y = torch.zeros_like(xn)
        for e in range(E):
            tok, slot = (ids == e).nonzero(as_tuple=True)
            if tok.numel():
                act = torch.nn.functional.silu(xn[tok] @ w1[e].t()) * (xn[tok] @ w3[e].t())
                y[tok] += (act @ lw["w2"][e].t()) * wk[tok, slot][:, None]
        # the taps, experts in index order
        by_id = ids.sort(-1)
        tap("route", by_id.values)
        tap("rw", wk.gather(-1, by_id.indices))
        tap("gl", gl)
        if ids.shape[1] == K and K < E:
            tap("gap", gl.gather(-1, order[:, K - 1:K])[:, 0] - gl.gather(-1, order[:, K:K + 1])[:, 0])
            # a relative error eps (L2) of the router's input moves a logit by at most eps |x| |router row|, and
            # a weight's logarithm by at most twice the largest logit error (softmax); the logits are rounded to
            # bf16 once more by both routers (2^-9 relative)
            ref = moer.topk(gl, K, True)
            lip = 2 * router_in.norm(dim=-1) * lw["router"].norm(dim=-1).max()
            own = ref.tol + ref.w * 2 * 2.0 ** -9 * gl.abs().max(-1, keepdim=True).values
            both = torch.stack([own, ref.w * lip[:, None]], -1)          # slot order, as ref.ids
            tap("rwtol", both.gather(1, by_id.indices[:, :, None].expand(-1, -1, 2)))
        return y

    @staticmethod
    def _attend(q, kk, vv, allowed, kvmap, scale):
        """q [n, hq, d], kk / vv [ctx, hkv, d], allowed bool [n, ctx] -> [n, hq, d]."""
        out = torch.empty_like(q)
        for h, kh in enumerate(kvmap):
            s = (q[:, h] @ kk[:, kh].t()) * scale
            s = s.masked_fill(~allowed, float("-inf"))
            out[:, h] = torch.softmax(s, -1) @ vv[:, kh]
        return out


# ------------------------------------------------------------------------------------- the same script, paged
COUNTED = ("attn_decode_fused", "attn_decode", "attn_prefill", "linear_slab_residual", "linear_slab",
           "linear_silu_mul_rownorm", "rms_row_scale", "linear_residual", "fused_add_rms_norm_slab",
           "fused_add_rms_norm", "rms_norm", "embed_sumsq", "row_sumsq", "rope_and_cache", "rope_and_cache_slab",
           "moe_route", "topk_softmax", "moe_forward_routed", "moe_apply", "residual_add_sumsq")
# the launches by which ``ops.moe_apply``'s three regimes differ, counted on the extension itself ("k.<name>");
# "k.segments" adds up the segments per expert of the grouped GEMM's launches (1 each in the streamed pass)
KERNELS = ("gemm_decode_grouped", "moe_gather", "moe_combine", "moe_combine_residual")
KERN_COUNTED = tuple(f"k.{n}" for n in KERNELS) + ("k.segments",)
# the collectives of the model's TPContext, counted on the instance ("tp.<name>")
TP_METHODS = ("all_reduce", "all_reduce_residual", "row_parallel_residual", "all_gather_last", "reduce_scatter_rows",
              "all_gather_rows")
TP_COUNTED = tuple(f"tp.{n}" for n in TP_METHODS)
# the residual stream is the argument of the path's last norm launch: (entry point, position of the residual)
_RESID_ARG = {"rms_norm": 0, "fused_add_rms_norm": 1, "fused_add_rms_norm_slab": 1}


class _CountingKernels:
    """The extension module with counters on KERNELS."""

    def __init__(self, mod, counts):
        self._mod, self._counts = mod, counts

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if name not in KERNELS:
            return fn

        def wrap(*args):  # positional, as src.ops calls them; the grouped GEMM's last argument: its segments
            self._counts["k." + name] = self._counts.get("k." + name, 0) + 1
            if name == "gemm_decode_grouped":
                self._counts["k.segments"] = self._counts.get("k.segments", 0) + int(args[-1])
            return fn(*args)

        return wrap


@contextlib.contextmanager
def counting(counts: Dict[str, int], last_norm: list, routed: Optional[list] = None, gating: Optional[list] = None,
             tp=None):
    """Counting wrappers on the ``src.ops`` entry points a forward composes (the model calls them as ``ops.<name>``)
    and on the MoE launches of the extension; ``last_norm`` receives the residual tensor of every norm launch,
    ``routed`` what every ``moe_route`` returned (weights, ids) and ``gating`` the logits given to ``topk_softmax``."""
    saved = {}
    for name in COUNTED:
        fn = getattr(ops, name)
        saved[name] = fn

        def wrap(*args, __fn=fn, __name=name, **kw):
            counts[__name] = counts.get(__name, 0) + 1
            if __name in _RESID_ARG:
                last_norm.append(args[_RESID_ARG[__name]])
            if __name == "topk_softmax" and gating is not None:
                gating.append(args[0])
            ret = __fn(*args, **kw)
            if __name == "moe_route" and routed is not None:
                routed.append(ret)
            return ret

        setattr(ops, name, wrap)
    kern = ops._kern
    if ops.native_available():
        ops._kern = lambda: _CountingKernels(kern(), counts)
    for name in TP_METHODS if tp is not None and tp.enabled else ():
        def wrap_tp(*args, __fn=getattr(tp, name), __name="tp." + name, **kw):  # calls among them count as well
            counts[__name] = counts.get(__name, 0) + 1
            return __fn(*args, **kw)

        setattr(tp, name, wrap_tp)   # on the instance: the class stays as it is
    try:
        yield
    finally:
        for name in TP_METHODS if tp is not None and tp.enabled else ():
            delattr(tp, name)
        ops._kern = kern
        for name, fn in saved.items():
            setattr(ops, name, fn)


def block_plan(script: Script, seed: int = 3):
    """Scattered block tables: every sequence's blocks are drawn from a shuffled pool in which block 0 and one block
    in five belong to nobody. Returns ({sequence: block ids}, blocks in the pool)."""
    need = {s: -(-sum(n for st in script.steps for nm, n in st.rows if nm == s) // BLOCK) for s in script.seqs}
    total = sum(need.values())
    nblocks = 1 + total + total // 4 + 2
    ids = list(range(1, nblocks))
    random.Random(seed).shuffle(ids)
    tables, at = {}, 0
    for s, n in need.items():
        tables[s] = ids[at:at + n]
        at += n
    return tables, nblocks


@torch.inference_mode()
def run_paged(model: CausalLM, script: Script, scratch: Optional[dict] = None, pre_embedded: bool = False,
              graph: bool = False) -> Taps:
    """``graph``: every decode step is captured with ``torch.cuda.graph`` and replayed."""
    dev, L = model.device, model.arch.num_layers
    tables, nblocks = block_plan(script)
    width = max(len(t) for t in tables.values())
    pool = torch.full((L, 2, nblocks, model.hkv, BLOCK, model.head_dim), SENTINEL, dtype=model.dtype, device=dev)
    owned = torch.zeros(nblocks, BLOCK, dtype=torch.bool)
    done = {s: 0 for s in script.seqs}
    out = Taps([], [], [], {}, pool=pool, owned=owned)
    max_rows = max(len(st.rows) for st in script.steps if not st.prefill) if any(
        not st.prefill for st in script.steps) else 1
    extra = {}
    if dev.type == "cuda":
        maxp = ops.decode_partials(width * BLOCK)
        extra = dict(part_o=torch.empty(max_rows * model.hq * maxp * 128, dtype=torch.float32, device=dev),
                     part_ml=torch.empty(max_rows * model.hq * maxp * 2, dtype=torch.float32, device=dev),
                     attn_cnt=torch.zeros(max_rows * model.hkv, dtype=torch.int32, device=dev))
    for st in script.steps:
        ids, pos, slots, cu, ctx, bt, keep = [], [], [], [0], [], [], []
        for name, n in st.rows:
            p0 = done[name]
            for p in range(p0, p0 + n):
                b = tables[name][p // BLOCK]
                slots.append(b * BLOCK + p % BLOCK)
                owned[b, p % BLOCK] = True
            ids += script.seqs[name][p0:p0 + n]
            pos += list(range(p0, p0 + n))
            done[name] = p0 + n
            cu.append(len(ids))
            ctx.append(p0 + n)
            bt.append(tables[name] + [0] * (width - len(tables[name])))
            if st.keep is not None and name in st.keep:
                keep.append(len(ids) - 1)
        t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)  # noqa: E731
        ids_t, pos_t = t(ids, torch.int64), t(pos, torch.int64)
        if st.prefill:
            meta = AttnMetadata(True, t(slots, torch.int64), t(bt, torch.int32), t(ctx, torch.int32),
                                t(cu, torch.int32), max(n for _, n in st.rows),
                                keep_rows=t(keep, torch.int64) if st.keep is not None else None)
        else:
            meta = AttnMetadata(False, t(slots, torch.int64), t(bt, torch.int32), t(ctx, torch.int32),
                                max_ctx=width * BLOCK, scratch=scratch, **extra)
            if pre_embedded:  # the entry the runner's sampling tail feeds: rows and statistics already in scratch
                ops.embed_sumsq(ids_t, model.embed, scratch["ssp0"], out=scratch["h_in"][: len(ids)])
                meta.pre_embedded = True
        counts: Dict[str, int] = {}
        norms: list = []
        routed: list = []
        gating: list = []
        with counting(counts, norms, routed, gating, model.tp):
            if graph and not st.prefill:
                # the step once eagerly (a captured step rewrites the same K / V slots with the same values), then
                # captured and replayed; the counts are those of the capture
                model.forward(ids_t, pos_t, meta, pool)
                counts.clear(), norms.clear(), routed.clear(), gating.clear()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    hidden = model.forward(ids_t, pos_t, meta, pool)
                g.replay()
                torch.cuda.synchronize()
            else:
                hidden = model.forward(ids_t, pos_t, meta, pool)
            # under sequence parallelism the residual is this rank's row shard, pad rows included
            resid = norms[-1].clone() if hidden.shape[0] else None
            logits = model.compute_logits(hidden) if hidden.shape[0] else None   # TP: the logits' all-gather
        if resid is None:  # a chunk that keeps no row: nothing behind the last layer's KV write
            resid, logits = hidden, hidden.new_zeros(0, model.arch.vocab_size)
        out.hidden.append(hidden.double().cpu())
        out.resid.append(resid.double().cpu())
        out.logits.append(logits.double().cpu())
        out.counts.append(counts)
        if model.arch.is_moe:  # one moe_route per layer, in layer order (none in the last layer of a chunk that
            # keeps no row); experts in index order
            K = model.arch.top_k
            for li in range(L):
                wk, ids = routed[li] if li < len(routed) else (torch.zeros(0, K), torch.zeros(0, K, dtype=torch.int32))
                by_id = ids.cpu().long().sort(-1)
                out.moe.setdefault(f"route{li}", []).append(by_id.values)
                out.moe.setdefault(f"rw{li}", []).append(wk.cpu().double().gather(-1, by_id.indices))
                if li < len(gating):
                    out.moe.setdefault(f"gl{li}", []).append(gating[li].double().cpu())
            assert len(routed) in (L, L - 1)
    cpu_pool = pool.cpu()
    for s, n in done.items():
        if n:
            out.kv[s] = read_kv(cpu_pool, tables[s], n)
    out.pool = cpu_pool
    return out


def read_kv(cpu_pool: torch.Tensor, table: List[int], n: int) -> torch.Tensor:
    """Positions 0 .. n-1 of one sequence through its block table: [layers, 2, n, kv heads, head_dim] float64."""
    p = torch.arange(n)
    blocks = torch.tensor(table)[p // BLOCK]
    sel = cpu_pool[:, :, blocks].permute(2, 4, 0, 1, 3, 5)[p, p % BLOCK]   # [n, L, 2, hkv, d]
    return sel.permute(1, 2, 0, 3, 4).double()


def untouched(taps: Taps) -> bool:
    """Every pool slot the script wrote nothing to (the blocks no sequence owns, and the tails of the others) still
    holds the sentinel, bit for bit."""
    pool = taps.pool  # [L, 2, blocks, hkv, BLOCK, d]
    want = torch.full((), SENTINEL, dtype=pool.dtype)
    same = (pool.view(torch.int16) == want.view(torch.int16)) if pool.element_size() == 2 else (pool == want)
    per_slot = same.all(-1).all(3).all(0).all(0)   # [blocks, BLOCK]
    return bool(per_slot[~taps.owned].all())


# ----------------------------------------------------------------------------------------------------- the metric
def tap_names(layers: int) -> List[str]:
    return ["hidden", "resid", "logits"] + [f"kv{li}" for li in range(layers)]


def _rows(t: Taps, tap: str) -> torch.Tensor:
    if tap in ("hidden", "resid", "logits"):
        return torch.cat([x.double() for x in getattr(t, tap)])
    li = int(tap[2:])
    return torch.cat([t.kv[s][li].reshape(-1, t.kv[s].shape[-1]) for s in sorted(t.kv)])


def row_errors(got: Taps, want: Taps, layers: int, taps: Optional[List[str]] = None) -> Dict[str, torch.Tensor]:
    """Per tap, the relative L2 error of every row (one token's hidden, residual or logits vector, or one
    (token, layer, kv head) K or V vector)."""
    out = {}
    for tap in taps or tap_names(layers):
        g, w = _rows(got, tap), _rows(want, tap)
        assert g.shape == w.shape, (tap, g.shape, w.shape)
        out[tap] = (g - w).norm(dim=-1) / w.norm(dim=-1)
    return out


# ---------------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    arch: str
    source: object                # the script, or a function that draws it when the case is first used (an MoE
    path: str                     # script is an oracle walk with rejection: only the tests that run it pay for it)
    fold: bool = True             # path: the chain of launches its judged steps must take
    claims: Tuple[str, ...] = ()
    opts: dict = field(default_factory=dict)   # gemm_residual, entry, tiled, p13, margin, graph; groups: group,
    world: int = 1                             # moe_parallel, sp. world: the ranks of the group that runs it

    @property
    def script(self) -> Script:
        if not isinstance(self.source, Script):
            self.source = self.source()
        return self.source


def expected_counts(path: str, L: int) -> Dict[str, int]:
    """Launches of one ``forward`` on each path (entry points not named: 0)."""
    z = {n: 0 for n in COUNTED}
    if path in ("slab_prefill", "slab_decode"):
        z.update(rms_norm=1, fused_add_rms_norm_slab=2 * L, linear_slab=3 * L, rope_and_cache_slab=L)
        z["attn_prefill" if path == "slab_prefill" else "attn_decode"] = L
    elif path == "rowscale_gemm":
        z.update(rms_row_scale=2 * L, linear_residual=2 * L, attn_prefill=L, rope_and_cache=L, rms_norm=1)
    elif path == "rowscale_add":
        z.update(rms_row_scale=2 * L, attn_prefill=L, rope_and_cache=L, fused_add_rms_norm=1)
    elif path == "rowscale_keep":
        z.update(rms_row_scale=2 * L - 1, linear_residual=2 * (L - 1), attn_prefill=L, rope_and_cache=L,
                 fused_add_rms_norm=2)
    elif path == "norm_loop":
        z.update(rms_norm=1, fused_add_rms_norm=2 * L, attn_prefill=L, rope_and_cache=L)
    elif path in ("fused_embed", "fused_pre"):
        z.update(attn_decode_fused=L, linear_slab_residual=2 * L, linear_slab=L, linear_silu_mul_rownorm=L,
                 rms_norm=1, embed_sumsq=1 if path == "fused_embed" else 0)
    else:
        raise KeyError(path)
    return z


def step_path(case: Case, step: Step) -> str:
    """The path one step of a case must take: the case's own for the steps it is about; a decode case's set-up
    prefill goes by its size, the decode steps behind a prefill case (no scratch) run on the slabs."""
    about_decode = case.path in ("slab_decode", "fused_embed", "fused_pre")
    if step.prefill == (not about_decode):
        return case.path
    if not step.prefill:
        return "slab_decode"
    if sum(n for _, n in step.rows) <= ops.DECODE_GEMM_MAX_M:
        return "slab_prefill"
    return "rowscale_gemm" if case.fold else "norm_loop"


def moe_regime(rows: int, hidden: int = 256, inter: int = 256) -> str:
    """Which of ``ops.moe_apply``'s three regimes an eager step of this many rows takes on experts of this (local)
    shape: by the row thresholds, and by whether the grouped decode GEMM has a tile for the shape at all."""
    if rows <= ops.MOE_DECODE_MAX_T and ops.moe_decode_tiles(hidden, inter, rows) is not None:
        return "streamed"
    if rows >= ops.MOE_LIBRARY_MIN_TOKENS or ops.moe_decode_tiles(hidden, inter, ops.MOE_DECODE_MAX_T) is None:
        return "library"
    return "segments"


GROUP_FUSED = ("tp_fused", "tp_separate", "tp_fallback", "ep_fused")   # group paths whose decode steps take scratch


def group_expected_counts(case: Case, step: Step, L: int) -> Dict[str, int]:
    """Launches and collectives of one ``forward`` + ``compute_logits`` of a step on every rank of a group (gloo
    for set-up, the one-shot collectives for the sums): the fused decode step with the tile exchange in the GEMM
    (``tp_fused``), with the separate ``all_reduce_residual`` launch (``tp_separate``; past 64 rows it falls back
    to ``all_reduce`` + ``residual_add_sumsq``: ``tp_fallback``), the MoE fused step under expert parallelism, the
    sequence-parallel prefill, else the norm loop or the row-scale prefill with their two all-reduces per layer."""
    a = arch_of(case.arch)
    z = {n: 0 for n in COUNTED + KERN_COUNTED + TP_COUNTED}
    rows = _step_rows(step)
    kept = None if step.keep is None else sum(1 for name, _ in step.rows if name in step.keep)
    inter = a.intermediate_size if case.opts.get("moe_parallel") == "ep" else a.intermediate_size // case.world
    z["tp.all_gather_last"] = int(kept != 0)   # the vocabulary-parallel head

    def moe_block(t):
        z["moe_route"] += 1
        z["moe_forward_routed"] += 1
        z["moe_apply"] += 1
        z["topk_softmax"] += t > ops.MOE_ROUTE_MAX_T
        regime = moe_regime(t, a.hidden_size, inter)
        if regime == "library":
            z["k.moe_gather"] += 1
        else:
            z["k.gemm_decode_grouped"] += 2
            z["k.segments"] += 2 * -(-t // ops.MOE_DECODE_MAX_T)
        z["k.moe_combine"] += 1

    if not step.prefill and case.path in GROUP_FUSED:
        z.update(embed_sumsq=1, linear_slab=L, attn_decode_fused=L)
        if a.is_moe:
            z["rms_norm"] = L + 1
            for _ in range(L):
                moe_block(rows)
        else:
            z.update(rms_norm=1, linear_silu_mul_rownorm=L)
        if case.path == "tp_fused":
            z["tp.row_parallel_residual"] = 2 * L
        else:
            z["tp.all_reduce_residual"] = 2 * L
            if rows > 64:   # past can_run_residual
                z["tp.all_reduce"] = z["residual_add_sumsq"] = 2 * L
        return z
    if case.opts.get("sp") and step.prefill:   # gloo has no reduce-scatter: an all-reduce and a slice
        z.update({"rms_norm": 1, "fused_add_rms_norm": 2 * L, "attn_prefill": L, "rope_and_cache": L,
                  "tp.all_gather_rows": 2 * L + 1, "tp.reduce_scatter_rows": 2 * L, "tp.all_reduce": 2 * L})
        return z
    full = L if kept is None else L - 1
    tail = {None: 1, 0: 0}.get(kept, 2)
    z["rope_and_cache"] = L
    z["attn_prefill" if step.prefill else "attn_decode"] = full + (1 if kept else 0)
    z["tp.all_reduce"] = 2 * full + (2 if kept else 0)
    if step.prefill and case.fold and rows > ops.DECODE_GEMM_MAX_M:
        if a.is_moe:
            z.update(rms_row_scale=L, fused_add_rms_norm=full + tail)
        else:
            z.update(rms_row_scale=L + full, fused_add_rms_norm=tail)
    else:
        z.update(rms_norm=1, fused_add_rms_norm=(L - 1) + full + tail)
    if a.is_moe:
        for _ in range(full):
            moe_block(rows)
        if kept:
            moe_block(kept)
    return z


def moe_expected_counts(case: Case, step: Step, L: int) -> Dict[str, int]:
    """Launches of one ``forward`` of an MoE case's step on one rank: the norm loop (steps of up to 128 rows,
    the unfolded model, decode without scratch), the row-scale prefill above 128 rows, either with the last layer
    cut to the kept rows, or the fused decode step; and per MoE block the router and regime its rows decide."""
    z = {n: 0 for n in COUNTED + KERN_COUNTED}
    rows = sum(n for _, n in step.rows)

    def moe_block(t):
        z["moe_route"] += 1
        z["moe_forward_routed"] += 1
        z["moe_apply"] += 1
        z["topk_softmax"] += t > ops.MOE_ROUTE_MAX_T     # the router GEMM + topk_softmax behind moe_route
        regime = moe_regime(t)
        if regime == "library":
            z["k.moe_gather"] += 1
        else:
            z["k.gemm_decode_grouped"] += 2
            z["k.segments"] += 2 * -(-t // ops.MOE_DECODE_MAX_T)
        z["k.moe_combine"] += 1

    if not step.prefill and case.path.startswith("moe_fused"):
        z.update({"linear_slab": L, "attn_decode_fused": L, "linear_slab_residual": L, "rms_norm": L + 1,
                  "embed_sumsq": int(case.path == "moe_fused_embed"), "moe_route": L, "moe_forward_routed": L,
                  "moe_apply": L, "k.gemm_decode_grouped": 2 * L, "k.segments": 2 * L, "k.moe_combine_residual": L})
        return z
    kept = None if step.keep is None else sum(1 for name, _ in step.rows if name in step.keep)
    full = L if kept is None else L - 1          # layers whose attention and MoE block run on every row
    tail = {None: 1, 0: 0}.get(kept, 2)          # norm launches behind them: the final one / none / ln2 and final
    z["rope_and_cache"] = L
    z["attn_prefill" if step.prefill else "attn_decode"] = full + (1 if kept else 0)
    if step.prefill and case.fold and rows > ops.DECODE_GEMM_MAX_M:
        z.update(rms_row_scale=L, fused_add_rms_norm=full + tail)
    else:
        z.update(rms_norm=1, fused_add_rms_norm=(L - 1) + full + tail)
    for _ in range(full):
        moe_block(rows)
    if kept:
        moe_block(kept)
    return z


RAGGED_128 = [("a", 37), ("b", 1), ("c", 64), ("d", 26)]
RAGGED_129 = [("a", 37), ("b", 1), ("c", 64), ("d", 27)]
_ATTN = ("pos_q_plus", "pos_q_minus", "pos_k_plus", "pos_k_minus", "kv_head_mod", "no_softmax_scale")
_ADDS = ("o_dropped", "o_doubled", "down_dropped", "down_doubled")
_SCALES = ("rs_neighbour_qkv", "rs_neighbour_mlp", "mlp_stats_pre_o")
_GAINS = ("fold_twice", "fold_none", "final_norm_layer_gain")
_DECODE = ("own_key_absent", "pos_q_plus", "pos_k_minus", "kv_head_mod", "no_softmax_scale", "mlp_stats_pre_o")
FUSED_ROWS = (1, 5, 32, 33, 65, 128)
MOE_FUSED_ROWS = (1, 5, 32, 33, 128)
_MOE_BLOCK = ("moe_router_raw", "moe_ln2_gain_off", "moe_no_renorm", "moe_top1", "moe_slots_swapped",
              "moe_expert_plus1", "moe_w1_w3_swapped", "moe_dropped", "moe_doubled")
_MOE = _MOE_BLOCK + ("moe_stats_pre_add",)
_TP = ("tp_o_dropped", "tp_o_doubled", "tp_down_dropped", "tp_down_doubled", "tp_heads_next_o", "tp_gate_next_up",
       "tp_next_kv_head", "tp_vocab_reversed")
_TP_SMALL = ("tp_o_doubled", "tp_down_dropped", "tp_heads_next_o", "tp_gate_next_up", "tp_vocab_reversed")
_EP = ("ep_unmasked", "ep_next_expert0")


@functools.lru_cache(maxsize=None)
def cases() -> Dict[str, Case]:
    c: Dict[str, Case] = {}
    P = functools.partial(prefill_script, "tiny")
    c["slab_prefill_5"] = Case("tiny", P([[("a", 3), ("b", 2)]]), "slab_prefill", claims=_GAINS + _ADDS)  # 3 + 2 tokens: too
    # few keys for a shifted position to clear the margin in every row it touches; the 128-row case claims those
    c["slab_prefill_128"] = Case("tiny", P([RAGGED_128]), "slab_prefill", claims=_ATTN + _GAINS + _ADDS)
    c["rowscale_129_gemm"] = Case("tiny", P([RAGGED_129]), "rowscale_gemm", claims=_SCALES + _ATTN + _ADDS,
                                  opts=dict(gemm_residual=True))
    c["rowscale_129_add"] = Case("tiny", P([RAGGED_129]), "rowscale_add", claims=_SCALES + _ADDS,
                                 opts=dict(gemm_residual=False))
    c["rowscale_long"] = Case("tiny", P([[("a", 150), ("b", 3), ("c", 20)]]), "rowscale_gemm",
                              claims=_SCALES + _ATTN[:4])
    c["rowscale_chunked"] = Case("tiny", P([[("a", 100), ("b", 40)], [("a", 90), ("c", 30), ("d", 20)]]),
                                 "rowscale_gemm", claims=("prefix_ignored", "pos_q_minus", "pos_k_plus"))
    c["rowscale_keep"] = Case("tiny", P([[("a", 70), ("b", 40), ("c", 1), ("d", 30)], [("a", 60), ("e", 80)]],
                                        keeps=[["b", "c", "d"], ["a", "e"]]), "rowscale_keep",
                              claims=("keep_first_row", "keep_neighbour_table", "prefix_ignored"))
    c["norm_loop_129"] = Case("tiny", P([RAGGED_129], decode_steps=2), "norm_loop", fold=False,
                              claims=_GAINS + ("own_key_absent",))
    for n in (1, 5, 33):
        c[f"slab_decode_{n}"] = Case("tiny", decode_script("tiny", n, steps=2), "slab_decode",
                                     claims=_DECODE[:4] + (() if n == 1 else ("rs_neighbour_mlp",)))
    for n in FUSED_ROWS:
        for entry in ("embed", "pre"):
            for tiled in (True, False):
                claims = _DECODE + ("ssp0_prev_step",) + (() if n == 1 else ("rs_neighbour_qkv", "rs_neighbour_mlp"))
                c[f"fused_{n}_{entry}_{'tiled' if tiled else 'rowmajor'}"] = Case(
                    "tiny", decode_script("tiny", n), f"fused_{entry}", claims=claims,
                    opts=dict(entry=entry, tiled=tiled))
    for on in (True, False):
        c[f"fused_mini_p13_{'on' if on else 'off'}"] = Case(
            "mini", decode_script("mini", 5), "fused_embed", claims=("rs_neighbour_mlp", "mlp_stats_pre_o", "fold_none"),
            opts=dict(entry="embed", tiled=True, p13=on))
    # ---- mixtral-tiny on one rank: the smallest shapes that reach each branch. Scripts are drawn on first use
    def M(*args, **kw):
        return functools.partial(prefill_script, "moe", *args, **kw)

    def D(arch, n):
        return functools.partial(decode_script, arch, n)

    # 5 rows: where the two chosen experts hold nearly all the mass, renormalising changes a weight by less than
    # MUT_FACTOR x its tolerance, and here every row would have to clear it; the larger cases claim that switch
    c["moe_norm_5"] = Case("moe", M([[("a", 3), ("b", 2)]]), "moe_norm",
                           claims=tuple(m for m in _MOE_BLOCK if m != "moe_no_renorm"))
    c["moe_norm_128"] = Case("moe", M([RAGGED_128]), "moe_norm", claims=_MOE + _ADDS[:2])
    c["moe_rowscale_129"] = Case("moe", M([RAGGED_129]), "moe_rowscale", claims=_MOE + ("rs_neighbour_qkv",))
    c["moe_rowscale_257"] = Case("moe", M([[("a", 150), ("b", 107)]]), "moe_rowscale", claims=_MOE)
    c["moe_chunked"] = Case("moe", M([[("a", 100), ("b", 40)], [("a", 90), ("c", 30), ("d", 20)]]), "moe_rowscale",
                            claims=("prefix_ignored", "moe_expert_plus1", "moe_stats_pre_add"))
    c["moe_keep"] = Case("moe", M([[("a", 70), ("b", 40), ("c", 1), ("d", 30)], [("a", 60), ("e", 80)],
                                   [("a", 10), ("e", 5)]], keeps=[["b", "c", "d"], [], ["a", "e"]]), "moe_keep",
                         claims=("keep_first_row", "keep_neighbour_table", "moe_router_raw", "moe_slots_swapped"))
    c["moe_unfolded"] = Case("moe", M([RAGGED_129], decode_steps=2), "moe_norm", fold=False,
                             claims=("fold_none", "moe_ln2_gain_off", "own_key_absent", "moe_top1"))
    for n in MOE_FUSED_ROWS:
        for entry in ("embed", "pre"):
            c[f"moe_fused_{n}_{entry}"] = Case("moe", D("moe", n), f"moe_fused_{entry}",
                                               claims=_MOE + ("ssp0_prev_step", "own_key_absent"),
                                               opts=dict(entry=entry))
    c["moe_fused_5_graph"] = Case("moe", D("moe", 5), "moe_fused_embed", claims=_MOE_BLOCK,
                                  opts=dict(entry="embed", graph=True))

    # ---- group W = 2, one spawn: every rank runs the cases in this order. The oracle and the tolerance are those of
    # the full model on the same script
    def G(name, arch, source, path, claims, **opts):
        c[name] = Case(arch, source, path, claims=claims, opts=dict(group="w2", **opts), world=2)

    for n in (1, 5, 32):   # llama-tiny, hq 2 and hkv 1 per rank: the exchange inside the o / down GEMMs
        G(f"tp2_fused_{n}", "tiny", D("tiny", n), "tp_fused", _TP if n > 1 else _TP_SMALL)
    for n in (5, 32):      # tp.fused_preferred = False: partial GEMM, then all_reduce_residual
        G(f"tp2_separate_{n}", "tiny", D("tiny", n), "tp_separate", _TP_SMALL)
    for n in (65, 128):    # past can_run_residual: all_reduce, then residual_add_sumsq
        G(f"tp2_fallback_{n}", "tiny", D("tiny", n), "tp_fallback", _TP_SMALL)
    G("tp2_norm_5", "tiny", P([[("a", 3), ("b", 2)]]), "tp_norm", _TP_SMALL)
    G("tp2_norm_128", "tiny", P([RAGGED_128]), "tp_norm", _TP)
    G("tp2_rowscale_129", "tiny", P([RAGGED_129]), "tp_rowscale", _TP)
    G("tp2_keep", "tiny", c["rowscale_keep"].script, "tp_keep", ("keep_first_row", "tp_heads_next_o", "tp_o_dropped"))
    G("tp2_prefix", "tiny", c["rowscale_chunked"].script, "tp_rowscale", ("prefix_ignored", "tp_next_kv_head"))
    G("tp2_sp_129", "tiny", P([RAGGED_129]), "tp_sp", ("sp_rank_minor", "sp_pad_counted", "tp_down_doubled"), sp=True)
    G("tp2_sp_5", "tiny", P([[("a", 3), ("b", 2)]]), "tp_sp", ("sp_rank_minor", "sp_pad_counted"), sp=True)
    G("tp2_sp_128", "tiny", P([RAGGED_128]), "tp_sp", ("sp_rank_minor", "tp_o_doubled"), sp=True)   # no pad row
    # mixtral-tiny, every expert's FFN dimension split (inter 128 per rank: no slab path, decode on the norm loop)
    G("tp2_moe_tp_5", "moe", M([[("a", 3), ("b", 2)]]), "tp_norm", ("moe_expert_plus1", "moe_dropped"), moe_parallel="tp")
    G("tp2_moe_tp_129", "moe", M([RAGGED_129]), "tp_rowscale", ("moe_slots_swapped", "moe_doubled", "tp_o_dropped"),
      moe_parallel="tp")
    G("tp2_moe_tp_decode_5", "moe", D("moe", 5), "tp_norm", ("moe_top1", "own_key_absent"), moe_parallel="tp")
    # expert parallelism: experts 0, 1 on rank 0 and 2, 3 on rank 1, the others' assignments in the null group
    G("tp2_moe_ep_5", "moe", M([[("a", 3), ("b", 2)]]), "tp_norm", _EP, moe_parallel="ep")
    G("tp2_moe_ep_129", "moe", M([RAGGED_129]), "tp_rowscale", _EP, moe_parallel="ep")
    for n in (1, 5, 33):
        G(f"tp2_moe_ep_fused_{n}", "moe", D("moe", n), "ep_fused", _EP, moe_parallel="ep")
    G("tp2_moe_ep_remote", "moe", ep_remote_script, "ep_fused", _EP, moe_parallel="ep")
    # ---- group W = 4, one spawn: llama-tiny with each kv head on two ranks, hq d = 128 per rank (no slab path)
    for name, source in (("tp4_norm_5", P([[("a", 3), ("b", 2)]])), ("tp4_decode_5", D("tiny", 5))):
        c[name] = Case("tiny", source, "tp_norm", opts=dict(group="w4"), world=4,
                       claims=("tp_next_kv_head", "tp_o_dropped", "tp_heads_next_o", "tp_vocab_reversed"))
    return c


def _chunked_off_grid(script: Script) -> bool:
    """Some prefill step holds a chunk behind a cached prefix that ends off the block grid, beside first chunks."""
    done = {s: 0 for s in script.seqs}
    for st in script.steps:
        if st.prefill and st.keep is None and any(done[s] % BLOCK for s, _ in st.rows) and any(
                done[s] == 0 for s, _ in st.rows):
            return True
        for s, n in st.rows:
            done[s] += n
    return False


def _step_rows(step: Step) -> int:
    return sum(n for _, n in step.rows)


def _moe_prefill_regimes(case: Case) -> set:
    """The ``moe_apply`` regimes the full-row MoE blocks of a case's prefill steps take."""
    return {moe_regime(_step_rows(st)) for st in case.script.steps if st.prefill}


# every path and entry the suite must cover -> a predicate over (name, case) that some case must satisfy
COVERAGE = {
    "slab prefill, 5 rows": lambda n, c: c.path == "slab_prefill" and c.script.tokens() == 5,
    "slab prefill, 128 rows ragged": lambda n, c: c.path == "slab_prefill" and c.script.tokens() == 128,
    "row-scale prefill at 129 rows, GEMM residual": lambda n, c: c.path == "rowscale_gemm" and c.script.tokens() == 129,
    "row-scale prefill at 129 rows, norm-pass add": lambda n, c: c.path == "rowscale_add" and c.script.tokens() == 129,
    "row-scale prefill, a sequence over one query tile": lambda n, c: c.path == "rowscale_gemm" and any(
        k >= 150 for st in c.script.steps for _, k in st.rows),
    "chunked prefill, prefix off the block grid, beside first chunks": lambda n, c: _chunked_off_grid(c.script),
    "row-scale prefill with keep_rows": lambda n, c: c.path == "rowscale_keep",
    "plain norm loop and its decode": lambda n, c: c.path == "norm_loop" and not c.fold and any(
        not st.prefill for st in c.script.steps),
    **{f"slab decode, {r} rows": (lambda n, c, r=r: c.path == "slab_decode" and len(c.script.steps[-1].rows) == r)
       for r in (1, 5, 33)},
    **{f"fused decode, {r} rows, {e} entry, {'tile-order' if t else 'row-major'} weights":
       (lambda n, c, r=r, e=e, t=t: c.path == f"fused_{e}" and c.arch == "tiny" and c.opts.get("tiled") == t
        and len(c.script.steps[-1].rows) == r and len(c.script.steps) == 4)
       for r in FUSED_ROWS for e in ("embed", "pre") for t in (True, False)},
    "fused decode on llama-mini, P13 on": lambda n, c: c.arch == "mini" and c.opts.get("p13") is True,
    "fused decode on llama-mini, P13 off": lambda n, c: c.arch == "mini" and c.opts.get("p13") is False,
    # mixtral-tiny on one rank
    "MoE norm loop, 5 rows": lambda n, c: c.path == "moe_norm" and c.script.tokens() == 5,
    "MoE norm loop, 128 rows ragged": lambda n, c: c.path == "moe_norm" and c.fold and c.script.tokens() == 128,
    **{f"moe_apply, {r} regime": (lambda n, c, r=r: c.arch == "moe" and r in _moe_prefill_regimes(c))
       for r in ("streamed", "segments", "library")},
    "fused moe_route": lambda n, c: c.arch == "moe" and any(_step_rows(st) <= ops.MOE_ROUTE_MAX_T for st in c.script.steps),
    "router GEMM + topk_softmax": lambda n, c: c.path == "moe_rowscale" and any(
        _step_rows(st) > ops.MOE_ROUTE_MAX_T for st in c.script.steps),
    "MoE row-scale prefill, 129 rows": lambda n, c: c.path == "moe_rowscale" and c.script.tokens() == 129,
    "MoE chunk behind a cached prefix of 100": lambda n, c: c.path == "moe_rowscale" and len(c.script.steps) == 2
    and c.script.steps[0].rows[0][1] == 100 and c.script.steps[1].rows[0][0] == c.script.steps[0].rows[0][0],
    "MoE keep_rows on the row-scale path, on the norm loop, and a chunk that keeps none": lambda n, c: (
        c.path == "moe_keep" and {(_step_rows(st) > ops.DECODE_GEMM_MAX_M, bool(st.keep)) for st in c.script.steps}
        >= {(True, True), (True, False), (False, True)}),
    "unfolded MoE model: norm loop, prefill and decode": lambda n, c: c.arch == "moe" and not c.fold and {
        st.prefill for st in c.script.steps} == {True, False},
    **{f"MoE fused decode, {r} rows, {e} entry": (lambda n, c, r=r, e=e: c.path == f"moe_fused_{e}"
                                                 and len(c.script.steps[-1].rows) == r and len(c.script.steps) == 4)
       for r in MOE_FUSED_ROWS for e in ("embed", "pre")},
    "MoE fused decode step captured in a graph": lambda n, c: c.arch == "moe" and c.opts.get("graph") is True,
    # the groups
    **{f"TP decode, {form} form, {r} rows": (lambda n, c, form=form, r=r: c.path == f"tp_{form}" and c.world == 2
                                             and len(c.script.steps[-1].rows) == r)
       for form, rows in (("fused", (1, 5, 32)), ("separate", (5, 32)), ("fallback", (65, 128))) for r in rows},
    "TP norm-loop prefill, 5 and 128 rows": lambda n, c: c.path == "tp_norm" and c.world == 2 and c.arch == "tiny",
    "TP row-scale prefill, 129 rows": lambda n, c: c.path == "tp_rowscale" and c.script.tokens() == 129,
    "TP keep_rows": lambda n, c: c.path == "tp_keep",
    "TP cached prefix": lambda n, c: c.path == "tp_rowscale" and len(c.script.steps) == 2,
    "SP prefill with a pad row, 129 rows": lambda n, c: c.opts.get("sp") and c.script.tokens() == 129,
    "SP prefill, 5 rows": lambda n, c: c.opts.get("sp") and c.script.tokens() == 5,
    "SP prefill without a pad row": lambda n, c: c.opts.get("sp") and c.script.tokens() % c.world == 0,
    "replicated kv heads": lambda n, c: c.world > arch_of(c.arch).num_kv_heads,
    "MoE with split experts under TP, prefill and decode": lambda n, c: c.opts.get("moe_parallel") == "tp" and any(
        not st.prefill for st in c.script.steps),
    "EP prefill and fused decode": lambda n, c: c.opts.get("moe_parallel") == "ep" and c.path == "ep_fused",
    "EP with an all-remote row": lambda n, c: c.opts.get("moe_parallel") == "ep" and bool(
        all_remote_steps(c.script, c.world)),
    "vocabulary-parallel head": lambda n, c: c.world > 1 and arch_of(c.arch).vocab_size % c.world == 0,
}


def moe_conditions(case: Case) -> dict:
    """What an MoE case must satisfy on the CPU before it judges anything: ``dev``, the largest deviation of the
    bf16 reference's router logits from the oracle's; ``undecided``, the (token, layer) pairs whose gap between the
    K-th and the (K+1)-th logit does not exceed GAP_FACTOR x dev; ``differ``, those where the bf16 reference chose
    another set than the oracle; ``experts``, how often each expert is chosen, per step."""
    L, E = arch_of(case.arch).num_layers, arch_of(case.arch).num_experts
    want = oracle_taps(case.arch, case.script)
    got = reference_taps(case.arch, case.script, case.fold)
    dev = max(float((g - w).abs().max()) for li in range(L)
              for g, w in zip(got.moe[f"gl{li}"], want.moe[f"gl{li}"]) if w.numel())
    gaps = torch.cat([t for li in range(L) for t in want.moe[f"gap{li}"]])
    differ = sum(int((g != w).any(-1).sum()) for li in range(L)
                 for g, w in zip(got.moe[f"route{li}"], want.moe[f"route{li}"]))
    experts = [sum(torch.bincount(want.moe[f"route{li}"][i].reshape(-1), minlength=E) for li in range(L)).tolist()
               for i in range(len(case.script.steps))]
    return dict(dev=dev, min_gap=float(gaps.min()), undecided=int((gaps <= GAP_FACTOR * dev).sum()), differ=differ,
                experts=experts)


def routing_errors(got: Taps, case: Case, tol_resid: float) -> dict:
    """A run's route taps against the oracle's: ``differ``, the (token, layer) pairs with another expert set
    (compared exactly), and ``rw``, the worst routing weight's error over its tolerance: moe_reference.py's bound
    for the weight itself plus its sensitivity to a relative error of the router's input, taken at the tolerance
    of ``resid`` and the bf16 rounding of the normalised row. That sensitivity is a worst case over every
    direction of the error (Cauchy-Schwarz over 256 features) and lets a weight move by more than itself; so the
    widening is cut at MARGIN x the largest routing-weight error of the bf16 reference on the same case, the
    yardstick of every other tap. ``beyond`` / ``affected``: the pairs that differ by more than MUT_FACTOR x the
    tolerance / at all (what a mutation is judged by)."""
    L = arch_of(case.arch).num_layers
    want = oracle_taps(case.arch, case.script)
    ref = reference_taps(case.arch, case.script, case.fold)
    ref_worst = max(float((a - b).abs().max()) for li in range(L)
                    for a, b in zip(ref.moe[f"rw{li}"], want.moe[f"rw{li}"]) if a.numel())
    eps = tol_resid + 2.0 ** -8
    differ, worst, beyond, affected = 0, 0.0, 0, 0
    for li in range(L):
        for g, w, gw, ww, tl in zip(got.moe[f"route{li}"], want.moe[f"route{li}"], got.moe[f"rw{li}"],
                                    want.moe[f"rw{li}"], want.moe[f"rwtol{li}"]):
            assert g.shape[0] == w.shape[0], (li, g.shape, w.shape)
            same = (g == w).all(-1) if g.shape == w.shape else torch.zeros(g.shape[0], dtype=torch.bool)
            differ += int((~same).sum())
            if not bool(same.any()):
                beyond, affected = beyond + int(same.numel()), affected + int(same.numel())
                continue
            tol = tl[..., 0] + torch.clamp(eps * tl[..., 1], max=MARGIN * ref_worst)
            err = (gw - ww).abs()[same]
            ratio = (err / tol[same]).max(-1).values
            worst = max(worst, float(ratio.max()))
            beyond += int((~same).sum()) + int((ratio > MUT_FACTOR).sum())
            affected += int((~same).sum()) + int((err.max(-1).values > 1e-9).sum())
    return dict(differ=differ, rw=worst, beyond=beyond, affected=affected, ref_worst=ref_worst)


# ------------------------------------------------------------------- per script: oracle, bf16 reference, tolerance
_memo: Dict[tuple, object] = {}


def _script_key(arch: str, script: Script, fold: bool) -> tuple:
    return (arch, fold, tuple((k, tuple(v)) for k, v in script.seqs.items()),
            tuple((s.prefill, tuple(s.rows), tuple(s.keep) if s.keep is not None else None) for s in script.steps))


def oracle_taps(arch: str, script: Script, mutation: Optional[str] = None, world: int = 1) -> Taps:
    key = ("oracle", mutation, world if mutation else 1) + _script_key(arch, script, True)
    if key not in _memo:
        _memo[key] = Oracle(family_weights(arch), mutation, world).run(script)
    return _memo[key]  # type: ignore[return-value]


@functools.lru_cache(maxsize=None)
def reference_model(arch: str, fold: bool, dtype) -> CausalLM:
    """The plain-PyTorch reference path of the model that a case runs: ``reference_copy("cpu", dtype)``."""
    return family_model(arch, "cpu", torch.bfloat16, fold).reference_copy("cpu", dtype)


def reference_taps(arch: str, script: Script, fold: bool = True) -> Taps:
    """The bf16 reference path's taps on a script."""
    key = ("bf16-taps",) + _script_key(arch, script, fold)
    if key not in _memo:
        _memo[key] = run_paged(reference_model(arch, fold, torch.bfloat16), script)
    return _memo[key]  # type: ignore[return-value]


def bf16_errors(arch: str, script: Script, fold: bool = True) -> Dict[str, torch.Tensor]:
    key = ("bf16",) + _script_key(arch, script, fold)
    if key not in _memo:
        _memo[key] = row_errors(reference_taps(arch, script, fold), oracle_taps(arch, script),
                                arch_of(arch).num_layers)
    return _memo[key]  # type: ignore[return-value]


def tolerance(arch: str, script: Script, fold: bool = True, margin: float = MARGIN) -> Dict[str, float]:
    assert MARGIN <= margin <= 4.0
    return {tap: margin * float(e.max()) for tap, e in bf16_errors(arch, script, fold).items()}


def case_tolerance(case: Case) -> Dict[str, float]:
    return tolerance(case.arch, case.script, case.fold, case.opts.get("margin", MARGIN))


# -------------------------------------------------------------------------------------------- the runner's scripts
RUNNER_PROMPTS = {3: [9, 17, 30], 7: [9, 17, 30, 4, 16, 33, 21]}   # prompt lengths: pads 4 and 8
RUNNER_TOKENS = 12


def runner_prompts(n: int) -> List[List[int]]:
    rng = random.Random(40 + n)
    vocab = arch_of("tiny").vocab_size
    out = [draw_tokens(rng, vocab, i, k) for i, k in enumerate(RUNNER_PROMPTS[n])]
    for i, p in enumerate(out):  # the last prompt token is loud (family_state_dict): the first step is decided too
        p[-1] = p[-1] - p[-1] % 5 + 4
    return out


def emitted_script(prompts: List[List[int]], outputs: List[List[int]]) -> Script:
    """The oracle's script for a generation: all prompts in one prefill step, then every sequence teacher-forced on
    the tokens it emitted (the last one is never fed back)."""
    seqs = {f"p{i}": list(p) + list(o[:-1]) for i, (p, o) in enumerate(zip(prompts, outputs))}
    sc = Script(seqs, [Step(True, [(f"p{i}", len(p)) for i, p in enumerate(prompts)],
                            keep=[f"p{i}" for i in range(len(prompts))])])
    for _ in range(len(outputs[0]) - 1):
        sc.steps.append(Step(False, [(name, 1) for name in seqs]))
    return sc


def oracle_greedy(prompts: List[List[int]], steps: int) -> List[List[int]]:
    """The oracle's own greedy continuation of the prompts."""
    outs: List[List[int]] = [[] for _ in prompts]
    for _ in range(steps):  # everything emitted so far is fed back; the last step's logits choose the next token
        last = Oracle(family_weights("tiny")).run(emitted_script(prompts, [o + [0] for o in outs])).logits[-1]
        for i in range(len(prompts)):
            outs[i].append(int(last[i].argmax()))
    return outs


def decided_steps(script: Script, tol_logits: float):
    """Per (step, row) of the script's oracle logits: (argmax, whether the top-2 gap exceeds the judged margin)."""
    out = []
    for lg in oracle_taps("tiny", script).logits:
        top = torch.topk(lg, 2, dim=-1)
        gap = top.values[:, 0] - top.values[:, 1]
        out.append((top.indices[:, 0], gap > GAP_FACTOR * tol_logits * lg.abs().max(dim=-1).values))
    return out


# ------------------------------------------------------------------------------------ a group of ranks on one GPU
def group_cases(group: str) -> List[str]:
    return [n for n, c in cases().items() if c.opts.get("group") == group]


def _digest(tensors) -> str:
    import hashlib

    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def _group_worker(rank: int, world: int, port: int, q, specs, limit: float) -> None:
    """One rank: gloo for set-up, the one-shot collectives for the sums; builds each model variant of the group
    once (the full family through ``load_state_dict``), runs the cases one after another through ``run_paged`` and
    reports its taps as numpy."""
    import faulthandler
    import os
    import traceback

    faulthandler.dump_traceback_later(limit, exit=True)   # a rank that hangs says where, and ends
    try:
        import torch.distributed as dist

        from src.parallel.tp import TPContext

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        tp = TPContext(rank=rank, world_size=world)
        assert tp.enable_custom_allreduce()
        models: Dict[tuple, tuple] = {}
        res = {}
        for name, case in specs:
            key = (case.arch, case.opts.get("moe_parallel", "tp"), bool(case.opts.get("sp")))
            if key not in models:
                m = CausalLM(arch_of(case.arch), "cuda:0", dtype=torch.bfloat16, tp=tp, seed=1, max_position=MAX_POS,
                             moe_parallel=key[1], sequence_parallel=key[2])
                m.load_state_dict(family_state_dict(case.arch))
                models[key] = (m, {})
            m, scratches = models[key]
            scratch, plans = None, {}
            if case.path in GROUP_FUSED:   # the plans are made when the scratch is: one scratch per form
                tp.fused_preferred = None if case.path == "tp_fused" else False
                if case.path not in scratches:
                    scratches[case.path] = m.alloc_decode_scratch(ops.DECODE_GEMM_MAX_M)
                scratch = scratches[case.path]
                assert scratch is not None
                plans = {b: bool(p["tp_fused"]) for b, p in scratch["plans"].items()}
            taps = run_paged(m, case.script, scratch=scratch)
            torch.cuda.synchronize()
            same = [*taps.hidden, *taps.logits] + ([] if key[2] else list(taps.resid))
            r = dict(digest=_digest(same), resid=[t.numpy() for t in taps.resid] if key[2] or rank == 0 else None,
                     kv={s: t.numpy() for s, t in taps.kv.items()}, counts=taps.counts, untouched=untouched(taps),
                     plans=plans, shape=(m.hq, m.hkv, m.experts_local, m.expert0, m.vocab_local))
            if rank == 0:
                r.update(hidden=[t.numpy() for t in taps.hidden], logits=[t.numpy() for t in taps.logits],
                         moe={k: [t.numpy() for t in v] for k, v in taps.moe.items()})
            res[name] = r
        ctl = tp.car.read_ctl()
        dist.barrier()
        q.put((rank, dict(cases=res, error=bool(ctl[2]), epoch=int(ctl[0]))))
        dist.destroy_process_group()
        faulthandler.cancel_dump_traceback_later()
    except Exception:  # surface the failure in the parent
        q.put((rank, traceback.format_exc()))
        raise


def spawn_group(group: str, world: int, deadline: float) -> dict:
    """Start the group's W processes once, wait for every rank's report for at most ``deadline`` seconds and return
    {rank: report}. On expiry, or when a rank dies, the children are terminated and a RuntimeError says why:
    nothing is retried."""
    import queue
    import socket
    import time

    import torch.multiprocessing as mp

    specs = [(n, cases()[n]) for n in group_cases(group)]
    for _, c in specs:
        c.script   # drawn here, once, not in every rank
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    t0 = time.time()
    procs = [ctx.Process(target=_group_worker, args=(r, world, port, q, specs, deadline)) for r in range(world)]
    for p in procs:
        p.start()
    res, why = {}, None
    while len(res) < world and why is None:
        try:
            rank, rep = q.get(timeout=1)
            res[rank] = rep
            if isinstance(rep, str):
                why = f"rank {rank} raised:\n{rep}"
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs) and q.empty():
                why = f"a rank ended without a report: exit codes {[p.exitcode for p in procs]}"
            elif time.time() - t0 > deadline:
                why = f"no report from every rank after {deadline} s"
    if why is not None:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(10)
        raise RuntimeError(f"group {group}: {why}")
    for p in procs:
        p.join(60)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    print(f"group {group}: {world} ranks, {len(specs)} cases in {time.time() - t0:.1f} s")
    return res


def assemble(case: Case, reports: dict, name: str) -> Taps:
    """One case's taps from the ranks' reports, as the full model's: hidden, residual and logits from rank 0 (bit
    for bit the same on every rank: asserted by digest); under sequence parallelism the residual is the ranks' row
    shards in rank order without the pad rows; K / V are the ranks' heads in rank order, a replicated head's
    copies bit-identical and counted once."""
    W = case.world
    r = [reports[k]["cases"][name] for k in range(W)]
    f = lambda a: torch.from_numpy(a)  # noqa: E731
    assert len({x["digest"] for x in r}) == 1, f"{name}: hidden / residual / logits differ between ranks"
    hidden, logits = [f(a) for a in r[0]["hidden"]], [f(a) for a in r[0]["logits"]]
    if case.opts.get("sp"):
        resid = [torch.cat([f(x["resid"][i]) for x in r])[: hidden[i].shape[0]] for i in range(len(hidden))]
    else:
        resid = [f(a) for a in r[0]["resid"]]
    nkv = arch_of(case.arch).num_kv_heads
    kv = {}
    for s in r[0]["kv"]:
        parts = [f(x["kv"][s]) for x in r]    # [L, 2, n, local heads, d] per rank
        if nkv < W:
            rep = W // nkv
            for j in range(nkv):
                assert all(torch.equal(parts[j * rep], parts[j * rep + i]) for i in range(1, rep)), (name, s, j)
            parts = parts[::rep]
        kv[s] = torch.cat(parts, 3)
    t = Taps(hidden, resid, logits, kv, counts=r[0]["counts"])
    t.moe = {k: [f(a) for a in v] for k, v in r[0]["moe"].items()}
    return t
