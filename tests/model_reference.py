"""Not a test: the float64 oracle of the dense Llama forward and everything the two files that use it share.

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
"""

from __future__ import annotations

import contextlib
import functools
import math
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from src import ops
from src.models.llama import AttnMetadata, CausalLM
from src.models.presets import get_preset

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

ARCHS = {"tiny": ("llama-tiny", {}), "mini": ("llama-mini", {"num_layers": 2})}

# the family's scales over the model's own init (std 0.02, o / down 0.02 / sqrt(2 L)); retuned per shape on the CPU:
# test_model_reference_cpu.py holds every case's tolerance under TOL_CAP and its mutations over MUT_FACTOR x tol
FAMILY = {"tiny": dict(q=1.5, k=1.5, v=1.0, o=16.0, down=16.0, gate_up=2.0, head_noise=0.1),
          "mini": dict(q=1.0, k=1.0, v=1.0, o=16.0, down=16.0, gate_up=2.0, head_noise=0.1)}


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
    sc = Script({name: draw_tokens(rng, vocab, i, total[name] + decode_steps) for i, name in enumerate(names)})
    for i, st in enumerate(chunks):
        sc.steps.append(Step(True, list(st), keeps[i] if keeps else None))
    for _ in range(decode_steps):
        sc.steps.append(Step(False, [(name, 1) for name in names]))
    return sc


def decode_contexts(n: int) -> List[int]:
    """Prompt lengths of a decode case with n rows, ragged within the step: the first decoded token sits at position
    15 (steps cross the block edge 15 -> 16), at 16 (16 -> 17), behind a context over 200, and at position 1 (a
    context of 2); the others are short."""
    rng = random.Random(100 + n)
    base = [15, 16, 205, 1]
    return base[:n] + [rng.randrange(2, 13) for _ in range(max(0, n - len(base)))]


def decode_script(arch_name: str, n: int, steps: int = 3) -> Script:
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
            layers.append(dict(ln1=f(sd[p + "input_layernorm.weight"]), ln2=f(sd[p + "post_attention_layernorm.weight"]),
                               q=f(sd[p + "self_attn.q_proj.weight"]), k=f(sd[p + "self_attn.k_proj.weight"]),
                               v=f(sd[p + "self_attn.v_proj.weight"]), o=f(sd[p + "self_attn.o_proj.weight"]),
                               gate=f(sd[p + "mlp.gate_proj.weight"]), up=f(sd[p + "mlp.up_proj.weight"]),
                               down=f(sd[p + "mlp.down_proj.weight"])))
        return cls(arch, f(sd["model.embed_tokens.weight"]), layers, f(sd["model.norm.weight"]),
                   f(sd["lm_head.weight"]), f(cos_sin))

    @classmethod
    def from_model(cls, m: CausalLM):
        f = lambda t: t.detach().to("cpu", torch.float64)  # noqa: E731
        nq, nk, i = m.hq * m.head_dim, m.hkv * m.head_dim, m.inter
        layers = []
        for lw in m.layers:
            qkv, gu = f(lw.qkv), f(lw.gate_up)
            layers.append(dict(ln1=f(lw.ln1), ln2=f(lw.ln2), q=qkv[:nq], k=qkv[nq:nq + nk], v=qkv[nq + nk:],
                               o=f(lw.o), gate=gu[:i], up=gu[i:], down=f(lw.down)))
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
    def __init__(self, w: Weights, mutation: Optional[str] = None):
        assert mutation is None or mutation in MUTATIONS, mutation
        self.w, self.mut = w, mutation

    def run(self, script: Script) -> Taps:
        w, a, mut = self.w, self.w.arch, self.mut
        L, hq, hkv, d, eps = a.num_layers, a.num_heads, a.num_kv_heads, a.head_dim, a.rms_eps
        g = hq // hkv
        kvmap = [(h % hkv) if mut == "kv_head_mod" else h // g for h in range(hq)]
        scale = 1.0 if mut == "no_softmax_scale" else 1.0 / math.sqrt(d)
        keys: Dict[str, List[List[torch.Tensor]]] = {s: [[] for _ in range(L)] for s in script.seqs}
        vals: Dict[str, List[List[torch.Tensor]]] = {s: [[] for _ in range(L)] for s in script.seqs}
        done = {s: 0 for s in script.seqs}
        out = Taps([], [], [], {})
        prev_embed = None

        def stats(x):
            return torch.rsqrt(x.pow(2).mean(-1) + eps)

        for st in script.steps:
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
            for li, lw in enumerate(w.layers):
                first = li == 0
                rs = stats(x)
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
                o = attn.reshape(len(ids), hq * d) @ lw["o"].t()
                x_pre = x
                x = x + o * ({"o_dropped": 0.0, "o_doubled": 2.0}.get(mut, 1.0) if first else 1.0)
                rs2 = stats(x_pre if first and mut == "mlp_stats_pre_o" else x)
                if first and mut == "rs_neighbour_mlp":
                    rs2 = torch.roll(rs2, 1)
                xn = x * rs2[:, None] * g2
                act = torch.nn.functional.silu(xn @ lw["gate"].t()) * (xn @ lw["up"].t())
                x = x + (act @ lw["down"].t()) * ({"down_dropped": 0.0, "down_doubled": 2.0}.get(mut, 1.0)
                                                  if first else 1.0)
            gain = w.layers[-1]["ln2"] if mut == "final_norm_layer_gain" else w.norm
            hidden = x * stats(x)[:, None] * gain
            if keep_rows is not None:
                sel = torch.tensor([r for _, r, _ in keep_rows], dtype=torch.long)
                x, hidden = x[sel], hidden[sel]
            out.hidden.append(hidden)
            out.resid.append(x)
            out.logits.append(hidden @ w.lm_head.t())
            prev_embed = embed_rows
        for s in script.seqs:
            if done[s]:
                out.kv[s] = torch.stack([torch.stack([torch.stack(keys[s][li]), torch.stack(vals[s][li])])
                                         for li in range(L)])
        return out

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
           "fused_add_rms_norm", "rms_norm", "embed_sumsq", "row_sumsq", "rope_and_cache", "rope_and_cache_slab")
# the residual stream is the argument of the path's last norm launch: (entry point, position of the residual)
_RESID_ARG = {"rms_norm": 0, "fused_add_rms_norm": 1, "fused_add_rms_norm_slab": 1}


@contextlib.contextmanager
def counting(counts: Dict[str, int], last_norm: list):
    """Counting wrappers on the ``src.ops`` entry points a forward composes (the model calls them as ``ops.<name>``);
    ``last_norm`` receives the residual tensor of every norm launch."""
    saved = {}
    for name in COUNTED:
        fn = getattr(ops, name)
        saved[name] = fn

        def wrap(*args, __fn=fn, __name=name, **kw):
            counts[__name] = counts.get(__name, 0) + 1
            if __name in _RESID_ARG:
                last_norm.append(args[_RESID_ARG[__name]])
            return __fn(*args, **kw)

        setattr(ops, name, wrap)
    try:
        yield
    finally:
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
def run_paged(model: CausalLM, script: Script, scratch: Optional[dict] = None, pre_embedded: bool = False) -> Taps:
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
        with counting(counts, norms):
            hidden = model.forward(ids_t, pos_t, meta, pool)
        resid = norms[-1].clone()
        logits = model.compute_logits(hidden)
        out.hidden.append(hidden.double().cpu())
        out.resid.append(resid.double().cpu())
        out.logits.append(logits.double().cpu())
        out.counts.append(counts)
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
    script: Script
    path: str                     # the chain of launches its judged steps must take (PATHS)
    fold: bool = True
    claims: Tuple[str, ...] = ()
    opts: dict = field(default_factory=dict)   # gemm_residual, entry, tiled, p13, margin


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


RAGGED_128 = [("a", 37), ("b", 1), ("c", 64), ("d", 26)]
RAGGED_129 = [("a", 37), ("b", 1), ("c", 64), ("d", 27)]
_ATTN = ("pos_q_plus", "pos_q_minus", "pos_k_plus", "pos_k_minus", "kv_head_mod", "no_softmax_scale")
_ADDS = ("o_dropped", "o_doubled", "down_dropped", "down_doubled")
_SCALES = ("rs_neighbour_qkv", "rs_neighbour_mlp", "mlp_stats_pre_o")
_GAINS = ("fold_twice", "fold_none", "final_norm_layer_gain")
_DECODE = ("own_key_absent", "pos_q_plus", "pos_k_minus", "kv_head_mod", "no_softmax_scale", "mlp_stats_pre_o")
FUSED_ROWS = (1, 5, 32, 33, 65, 128)


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
}


# ------------------------------------------------------------------- per script: oracle, bf16 reference, tolerance
_memo: Dict[tuple, object] = {}


def _script_key(arch: str, script: Script, fold: bool) -> tuple:
    return (arch, fold, tuple((k, tuple(v)) for k, v in script.seqs.items()),
            tuple((s.prefill, tuple(s.rows), tuple(s.keep) if s.keep is not None else None) for s in script.steps))


def oracle_taps(arch: str, script: Script, mutation: Optional[str] = None) -> Taps:
    key = ("oracle", mutation) + _script_key(arch, script, True)
    if key not in _memo:
        _memo[key] = Oracle(family_weights(arch), mutation).run(script)
    return _memo[key]  # type: ignore[return-value]


@functools.lru_cache(maxsize=None)
def reference_model(arch: str, fold: bool, dtype) -> CausalLM:
    """The plain-PyTorch reference path of the model that a case runs: ``reference_copy("cpu", dtype)``."""
    return family_model(arch, "cpu", torch.bfloat16, fold).reference_copy("cpu", dtype)


def bf16_errors(arch: str, script: Script, fold: bool = True) -> Dict[str, torch.Tensor]:
    key = ("bf16",) + _script_key(arch, script, fold)
    if key not in _memo:
        got = run_paged(reference_model(arch, fold, torch.bfloat16), script)
        _memo[key] = row_errors(got, oracle_taps(arch, script), arch_of(arch).num_layers)
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
