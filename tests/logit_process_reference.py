"""
The tests' own oracle of the logit-processing contract (csrc/kernels/logit_process.hip, ops.logit_process):
pure torch, fp32, every step ONE individually rounded operation in the kernel's order, so that torch on the CPU
reproduces the kernel bit for bit. Deliberately a copy of src/ops/reference.py's function, not an import.

For the bf16 logit z of token t, with c = how often t was generated so far (saturating at 32767):
    1. x = float(z) + bias[t]                      (0 where there is no bias)
    2. if t is in the prompt or c > 0:             x = x * inv_rp if x > 0 else x * rp
    3. x = x - freq * float(c)
    4. if c > 0:                                   x = x - pres
    5. one rounding to bf16
inv_rp is fp32(1 / rp), computed once on the host: nothing divides per element.
"""

from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

COUNT_MAX = 32767


def inv_f32(rp: float) -> float:
    """fp32(1 / fp32(rp)) as the host passes it to the kernel."""
    return float(np.float32(1.0) / np.float32(rp))


def logit_process(logits: torch.Tensor, in_prompt: torch.Tensor, counts: torch.Tensor, rp: float, inv_rp: float,
                  freq: float, pres: float, bias: torch.Tensor = None) -> torch.Tensor:
    """One row (or rows sharing the parameters): logits bf16 [..., V], in_prompt bool [..., V], counts integer
    [..., V] (already saturated), bias fp32 [..., V] or None -> the processed bf16 row(s)."""
    f32 = torch.float32
    x = logits.to(f32)
    b = torch.zeros_like(x) if bias is None else bias.to(f32)
    x = x + b
    c = counts.to(torch.int64).clamp(max=COUNT_MAX)
    seen = in_prompt.to(torch.bool) | (c > 0)
    t_rp, t_inv = torch.tensor(rp, dtype=f32), torch.tensor(inv_rp, dtype=f32)
    x = torch.where(seen, torch.where(x > 0, x * t_inv, x * t_rp), x)
    x = x - torch.tensor(freq, dtype=f32) * c.to(f32)
    x = torch.where(c > 0, x - torch.tensor(pres, dtype=f32), x)
    return x.to(torch.bfloat16)


@torch.inference_mode()
def greedy_reference_processed(model, prompt, n, rp=1.0, freq=0.0, pres=0.0, bias=None):
    """Greedy no-cache recompute with the oracle applied to every step's last row: (tokens, top1 - top2 margins of
    the PROCESSED row). The state is rebuilt from the token lists at every step: the prompt's tokens are "in the
    prompt", every token generated so far is counted."""
    from tests.logprobs_reference import all_rows_logits

    ids, toks, margins = list(prompt), [], []
    vocab = model.arch.vocab_size
    in_prompt = torch.zeros(vocab, dtype=torch.bool)
    in_prompt[torch.tensor(sorted(set(prompt)))] = True
    b = None
    if bias:
        b = torch.zeros(vocab, dtype=torch.float32)
        for t, v in bias.items():
            b[int(t)] = v
    for _ in range(n):
        lg = all_rows_logits(model, ids)[-1].to(torch.bfloat16).cpu()
        counts = torch.zeros(vocab, dtype=torch.int64)
        if toks:
            counts.index_add_(0, torch.tensor(toks), torch.ones(len(toks), dtype=torch.int64))
        out = logit_process(lg, in_prompt, counts, rp, inv_f32(rp), freq, pres, b).float()
        top = torch.topk(out, 2)
        best = float(top.values[0])
        toks.append(int((out == best).nonzero()[0, 0]))  # the lowest index holding the maximum
        margins.append(best - float(top.values[1]))
        ids.append(toks[-1])
    return toks, margins


def agree_until_near_tie(got, want, margins, threshold=0.25):
    """The number of leading steps compared: `got` must equal `want` up to the reference's first near-tie
    (a processed margin below `threshold`), where rounding may legitimately pick the other token."""
    first = next((i for i, m in enumerate(margins) if m < threshold), len(want))
    assert got[:first] == want[:first], (got, want, margins)
    return first


# ======================================================================================================================
# The second oracle, the designed rows and the mutants (tests/test_logit_process_reference_cpu.py judges them,
# tests/test_logit_process_kernel_gpu.py runs the kernel on them).
#
# `process_np` is the contract again in numpy float64 with an explicit float32 rounding after each of the five steps:
# one +, - or x of two fp32 values in float64 (53 >= 2 * 24 + 2 bits) followed by the cast IS the fp32 operation.
# The final rounding to bf16 is written out (round to nearest, ties to even, on the bit pattern). The CPU test asks it
# to be bit-identical to the torch function above on every case, so the two implementations check each other.
#
# Element mutants (`mutation=`), the likely violations of the contract:
#   fma3          step 3 contracted into one FMA: fp32(x - freq * c) with the product exact
#   fold34        steps 3 + 4 as x - (freq * c + pres)
#   f64           nothing rounded before the end
#   div           x / rp instead of x * inv_rp
#   bias_after    the bias added after the penalties
#   pres_prompt   the presence penalty also on tokens that only occur in the prompt
#   norep_prompt  no repetition penalty on tokens that only occur in the prompt
# Row mutants (`rows_oracle(mutation=)`): count_before (the count used before count_ids is added), nosat (counts not
# saturated at 32767), params_by_row / state_by_row (indexed by row instead of slot), count_ids_by_slot.
# The final bf16 rounding hides almost every fp32-level difference, so the `rounding` rows come from a seeded search
# (`search_rounding`): candidates (z, bias, count) whose step 3 (or 3 + 4) cancels — bias chosen so that
# (z + bias) * inv_rp lands within a few fp32 ulps of freq * c + pres — kept where the contract's bf16 result and the
# mutant's differ. With the bias free to place x, every element mutant above is observable, x / rp included (on bare
# bf16 z, with no bias, a search over 2 * 10^6 draws found none for x / rp: it needs the 24-bit x that a bias gives).
#
# The bias table of the kernel: a 1024-slot open-addressing hash, slot (id * 2654435761 mod 2^32) >> 22, linear
# probing with wrap-around, behind a bitmap of one byte per 16-byte group. The families (at vocab 8200): `chain` (the
# fullest slot's ids, >= 8), `wrap` (>= 12 ids of slots 1021..1023 and some of slots 0 and 1: the chain continues at
# slot 0), `full` (300 entries, bias_cnt = cap + 5 reads cap), `group` (all eight ids of one group, a group with only
# bit 0 and one with only bit 7), `edges` (ids 0 and vocab - 1), `stray` (list entries -1, vocab and 2^31 - 1 among
# valid ones are skipped, entries beyond bias_cnt ignored, bias_cnt = -3 reads none), `banned` (bias -inf).

LP_HASH, LP_HASH_MULT, LP_HASH_SHIFT = 1024, 2654435761, 22
CAP = 300
ELEMENT_MUTATIONS = ("fma3", "fold34", "f64", "div", "bias_after", "pres_prompt", "norep_prompt")
ROW_MUTATIONS = ("count_before", "nosat", "params_by_row", "state_by_row", "count_ids_by_slot")
NEG_INF_BITS, NO_INDEX = 0xff800000, 0x7fffffff


def lp_hash(ids) -> np.ndarray:
    return ((np.asarray(ids, dtype=np.uint64) * LP_HASH_MULT) & 0xffffffff) >> LP_HASH_SHIFT


def bits_f32(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def rne_bf16(x32) -> np.ndarray:
    """fp32 -> bf16 bit patterns, round to nearest, ties to even (no NaN among the inputs)."""
    u = np.asarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _r(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def process_np(zbits, in_prompt, counts, rp, inv_rp, freq, pres, bias=None, mutation=None) -> np.ndarray:
    """One row: bf16 bit patterns in, bf16 bit patterns out. rp, inv_rp, freq, pres are fp32 values."""
    assert mutation is None or mutation in ELEMENT_MUTATIONS or mutation == "nosat"
    rnd = (lambda a: np.asarray(a, dtype=np.float64)) if mutation == "f64" else _r
    rp, inv_rp, freq, pres = (float(np.float32(v)) for v in (rp, inv_rp, freq, pres))
    z = bits_f32(zbits).astype(np.float64)
    b = np.zeros_like(z) if bias is None else np.asarray(bias, dtype=np.float32).astype(np.float64)
    c = np.asarray(counts, dtype=np.int64)
    if mutation != "nosat":
        c = np.minimum(c, COUNT_MAX)
    prompt = np.asarray(in_prompt, dtype=bool)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x = z if mutation == "bias_after" else rnd(z + b)
        seen = (c > 0) if mutation == "norep_prompt" else (prompt | (c > 0))
        up = rnd(x / rp) if mutation == "div" else rnd(x * inv_rp)
        x = np.where(seen, np.where(x > 0, up, rnd(x * rp)), x)
        cf = c.astype(np.float64)
        if mutation == "fma3":
            x = rnd(x - freq * cf)                     # the product of a 24-bit and a 16-bit number is exact here
            x = np.where(c > 0, rnd(x - pres), x)
        elif mutation == "fold34":
            x = np.where(c > 0, rnd(x - rnd(rnd(freq * cf) + pres)), rnd(x - rnd(freq * cf)))
        else:
            x = rnd(x - rnd(freq * cf))
            x = np.where((prompt | (c > 0)) if mutation == "pres_prompt" else (c > 0), rnd(x - pres), x)
        if mutation == "bias_after":
            x = rnd(x + b)
        return rne_bf16(x.astype(np.float32))


@dataclasses.dataclass(frozen=True)
class RowsCase:
    name: str
    vocab: int
    x: np.ndarray            # uint16 [R, V] bf16 bit patterns
    slot: np.ndarray         # int32 [R]
    state: np.ndarray        # uint16 [S, V]
    params: np.ndarray       # float32 [S, 4] = rp, fp32(1 / rp), freq, pres
    bias_cnt: np.ndarray     # int32 [S]
    bias_ids: np.ndarray     # int32 [S, CAP]
    bias_vals: np.ndarray    # float32 [S, CAP]
    count_ids: np.ndarray    # int64 [R]
    families: dict           # slot -> the families its row stands for
    claims: dict             # row -> the element mutants that change >= 8 of its elements
    row_claims: tuple        # the row mutants that change the case's rows or state


def bias_row(case: RowsCase, s: int):
    """The dense bias of slot s, or None: the first min(max(cnt, 0), cap) entries, ids outside [0, vocab) skipped."""
    nb = min(max(int(case.bias_cnt[s]), 0), case.bias_ids.shape[1])
    if nb == 0:
        return None
    b = np.zeros(case.vocab, dtype=np.float32)
    ids = case.bias_ids[s, :nb].astype(np.int64)
    ok = (ids >= 0) & (ids < case.vocab)
    b[ids[ok]] = case.bias_vals[s, :nb][ok]
    return b


def rows_oracle(case: RowsCase, counted: bool = True, mutation: str = None, impl=None):
    """The whole launch: (rows uint16 [R, V], state uint16 [S, V], candidates {row: (fp32 bits of the maximum, its
    lowest index)}). `impl(zbits, prompt, counts, rp, inv_rp, freq, pres, bias)` replaces process_np."""
    rows, nslots = case.x.shape[0], case.state.shape[0]
    out, state, cand = case.x.copy(), case.state.copy(), {}
    elem = mutation if mutation in ELEMENT_MUTATIONS else None
    for r in range(rows):
        s = int(case.slot[r])
        if s < 0 or s >= nslots:
            continue
        ss = r % nslots if mutation == "state_by_row" else s
        st = state[ss].astype(np.int64)
        c = st & 0x7fff
        cid = int(case.count_ids[s % rows if mutation == "count_ids_by_slot" else r]) if counted else -1
        if 0 <= cid < case.vocab:
            new = int(c[cid]) + 1 if mutation == "nosat" else min(int(c[cid]) + 1, COUNT_MAX)
            state[ss, cid] = ((int(st[cid]) & 0x8000) | new) & 0xffff if mutation != "nosat" else \
                ((int(st[cid]) & 0x8000) + new) & 0xffff
            if mutation != "count_before":
                c = c.copy()
                c[cid] = new
        rp, inv, freq, pres = case.params[r % nslots if mutation == "params_by_row" else s]
        args = (case.x[r], (st & 0x8000) != 0, c, rp, inv, freq, pres, bias_row(case, s))
        if impl is not None:
            out[r] = impl(*args)
        else:
            out[r] = process_np(*args, mutation="nosat" if mutation == "nosat" else elem)
        v = bits_f32(out[r])
        m = v.max()
        cand[r] = (int(np.float32(m).view(np.uint32)), int(np.flatnonzero(v == m)[0]))
    return out, state, cand


def search_rounding(params, mutation: str, seed: int, want: int = 16, draws: int = 200000):
    """Seeded search for elements (z bits, bias, count, prompt bit) under a slot's (rp, inv_rp, freq, pres) whose bf16
    result differs between the contract and `mutation`. Returns up to `want` of them (arrays)."""
    rng = np.random.default_rng(seed)
    rp, inv, freq, pres = (float(np.float32(v)) for v in params)
    z = rne_bf16((rng.standard_normal(draws) * 6).astype(np.float32))
    c = rng.integers(1, 40, draws)
    prompt = rng.random(draws) < 0.3
    fc = _r(freq * c.astype(np.float64))
    x1 = _r(fc + pres)                                            # where steps 3 + 4 cancel
    xb = np.where(x1 > 0, x1 * rp, x1 / rp) * (1.0 + rng.integers(-4, 5, draws) * 2.0 ** -23)
    bias = (xb - bits_f32(z).astype(np.float64)).astype(np.float32)
    good = process_np(z, prompt, c, rp, inv, freq, pres, bias)
    bad = process_np(z, prompt, c, rp, inv, freq, pres, bias, mutation)
    keep = np.flatnonzero((good != bad) & np.isfinite(bias) & (bias != 0))[:want]
    return z[keep], bias[keep], c[keep], prompt[keep]


def _params(rp, freq, pres):
    return np.array([rp, inv_f32(rp), freq, pres], dtype=np.float32)


def _random_state(rng, slots, vocab):
    """Prompt bits on 30 %, counts 0 mostly, some 1..39; per slot one saturated, one 32766 and one prompt-only entry
    (`_planted` finds them again)."""
    pick = rng.random((slots, vocab))
    counts = np.where(pick < 0.25, rng.integers(1, 40, (slots, vocab)), 0)
    prompt = rng.random((slots, vocab)) < 0.3
    return (counts | (prompt.astype(np.int64) << 15)).astype(np.uint16)


def _noninteger(rng, n, scale=20.0):
    return ((rng.random(n) * 2 - 1) * scale + 0.37).astype(np.float32)


class _Builder:
    def __init__(self, name, vocab, nslots, row_slot, seed):
        self.name, self.vocab, self.rng = name, vocab, np.random.default_rng(seed)
        rows = len(row_slot)
        self.x = rne_bf16((self.rng.standard_normal((rows, vocab)) * 6).astype(np.float32))
        self.slot = np.array(row_slot, dtype=np.int32)
        self.state = _random_state(self.rng, nslots, vocab)
        self.params = np.tile(_params(1.0, 0.0, 0.0), (nslots, 1))
        self.bias_cnt = np.zeros(nslots, dtype=np.int32)
        # beyond bias_cnt the table holds other values, which must be ignored
        self.bias_ids = self.rng.integers(0, vocab, (nslots, CAP)).astype(np.int32)
        self.bias_vals = np.full((nslots, CAP), 77.0, dtype=np.float32)
        self.count_ids = np.full(rows, -1, dtype=np.int64)
        self.families, self.claims = {}, {}

    def row_of(self, s):
        return int(np.flatnonzero(self.slot == s)[0])

    def set_bias(self, s, ids, vals, cnt=None):
        ids = np.asarray(ids, dtype=np.int64)
        assert ids.size <= CAP and np.unique(ids[(ids >= 0) & (ids < self.vocab)]).size == ((ids >= 0) & (ids < self.vocab)).sum()
        self.bias_ids[s, :ids.size] = ids.astype(np.int32)
        self.bias_vals[s, :ids.size] = vals
        self.bias_cnt[s] = ids.size if cnt is None else cnt

    def rounding(self, s, rp, freq, pres, mutants, seed):
        """Searched elements at random places of the slot's row, each mutant with 16 of them."""
        self.params[s] = _params(rp, freq, pres)
        r = self.row_of(s)
        n = 16 * len(mutants)
        places = self.rng.permutation(self.vocab)[:n]
        bias = np.zeros(n, dtype=np.float32)
        for i, m in enumerate(mutants):
            z, b, c, p = search_rounding(self.params[s], m, seed + i)
            k = z.size
            at = places[16 * i:16 * i + k]
            self.x[r, at] = z
            self.state[s, at] = (c | (p.astype(np.int64) << 15)).astype(np.uint16)
            bias[16 * i:16 * i + k] = b
        used = bias != 0
        self.set_bias(s, places[used], bias[used])
        self.families[s] = ("rounding",)
        self.claims[r] = tuple(mutants) + ("bias_after", "norep_prompt") + (("pres_prompt",) if pres else ())

    def plant_count_id(self, s, kind):
        """This step's input id of the slot's row: an entry of the kind, planted into the state."""
        r = self.row_of(s)
        if kind in ("minus_one", "vocab"):
            self.count_ids[r] = -1 if kind == "minus_one" else self.vocab
            return
        nb = max(int(self.bias_cnt[s]), 0)
        if kind == "biased":
            ids = self.bias_ids[s, :min(nb, CAP)]
            t = int(ids[(ids >= 0) & (ids < self.vocab)][0])
        else:
            t = int(self.rng.integers(0, self.vocab))
            self.state[s, t] = {"saturated": COUNT_MAX, "c32766": 0x8000 | (COUNT_MAX - 1), "prompt_only": 0x8000,
                                "unseen": 0}[kind]
        self.count_ids[r] = t

    def build(self, row_claims=()):
        return RowsCase(self.name, self.vocab, self.x, self.slot, self.state, self.params, self.bias_cnt,
                        self.bias_ids, self.bias_vals, self.count_ids, self.families, self.claims, tuple(row_claims))


def slot_ids(vocab: int):
    """ids by table slot: (slots of every id, ids sorted by slot occupancy helper)."""
    h = lp_hash(np.arange(vocab))
    return h, np.bincount(h.astype(np.int64), minlength=LP_HASH)


def _main_case():
    """vocab 8200, every family. Rows map to permuted slots; row 1 has slot -1, row 5 slot = num_slots."""
    v, ns = 8200, 9
    b = _Builder("main_8200", v, ns, (3, -1, 0, 6, 2, ns, 1, 4, 5, 7), 9100)
    rng = b.rng
    b.rounding(0, 1.3, 0.7, 0.0, ("fma3", "div", "f64"), 9110)
    b.rounding(1, 1.3, 0.7, 0.3, ("fold34", "f64"), 9120)
    # slot 2: chain, wrap, group, edges
    h, occ = slot_ids(v)
    chain = np.flatnonzero(h == int(np.argmax(occ)))
    wrap = np.flatnonzero((h >= 1021) | (h <= 1))
    g0, g1, g2 = 8 * 300, 8 * 511, 8 * 777
    ids = np.unique(np.concatenate([chain, wrap, np.arange(g0, g0 + 8), [g1, g2 + 7, 0, v - 1]]))
    b.set_bias(2, rng.permutation(ids), _noninteger(rng, ids.size))
    b.params[2] = _params(2.0, -0.25, 1.1)
    b.families[2] = ("chain", "wrap", "group", "edges")
    # slot 3: the full list, bias_cnt beyond the cap
    b.set_bias(3, rng.permutation(v)[:CAP], _noninteger(rng, CAP), cnt=CAP + 5)
    b.params[3] = _params(0.5, 1.5, -2.0)
    b.families[3] = ("full",)
    # slot 4: stray entries among valid ones, other values beyond bias_cnt
    ids = rng.permutation(v)[:40].astype(np.int64)
    ids[[0, 7, 20, 39]] = [-1, v, 2 ** 31 - 1, -2 ** 31]
    b.set_bias(4, ids, _noninteger(rng, 40))
    b.params[4] = _params(1.1, 0.013, 0.2)
    b.families[4] = ("stray",)
    # slot 5: a negative count over a full table
    b.set_bias(5, rng.permutation(v)[:CAP], _noninteger(rng, CAP), cnt=-3)
    b.params[5] = _params(1.1, 0.013, 0.2)
    b.families[5] = ("stray",)
    # slot 6 (row 3): integers, nothing rescaled, the raw argmax banned; the processed maximum 5 ties between ids of
    # different threads, waves and sweeps — the lowest id wins
    r = b.row_of(6)
    b.x[r] = rne_bf16(rng.integers(-3, 4, v).astype(np.float32))
    tie = [8 * 70 + 3, 8 * 700, 8192 + 5, 8 * 1023 + 7]
    b.x[r, tie] = rne_bf16(np.float32(5.0))
    b.x[r, [40, 6000]] = rne_bf16(np.float32(9.0))
    b.state[6] = 0
    b.set_bias(6, [40, 6000, 3, v - 1], np.array([-np.inf] * 4, dtype=np.float32))
    b.families[6] = ("banned", "tie")
    # slot 7 (row 9): the processed maximum at vocab - 1
    b.set_bias(7, [v - 1, 11], np.array([60.5, -3.25], dtype=np.float32))
    b.params[7] = _params(1.3, 0.7, 0.3)
    b.families[7] = ("edges", "last_max")
    for s, kind in ((3, "saturated"), (0, "c32766"), (6, "unseen"), (2, "biased"), (1, "prompt_only"),
                    (4, "minus_one"), (5, "vocab"), (7, "unseen")):
        b.plant_count_id(s, kind)
    b.count_ids[1], b.count_ids[5] = 1, 2        # the unprocessed rows' ids count nothing
    return b.build(ROW_MUTATIONS)


def _small_case(v, seed):
    """The other vocabularies: a rounding row, a full list with ids 0 and vocab - 1, a stray list; unprocessed rows."""
    ns = 4
    b = _Builder(f"shape_{v}", v, ns, (2, ns, 0, -1, 1), seed)
    rng = b.rng
    b.rounding(0, 1.3, 0.7, 0.3, ("fold34", "fma3"), seed + 10)
    ids = np.concatenate([[v - 1], rng.permutation(v - 2)[:CAP - 2] + 1, [0]])
    b.set_bias(1, ids, _noninteger(rng, CAP), cnt=CAP + 5)
    b.params[1] = _params(0.5, 1.5, -2.0)
    b.families[1] = ("full", "edges")
    ids = rng.permutation(v)[:40].astype(np.int64)
    ids[[3, 11, 30]] = [-1, v, 2 ** 31 - 1]
    b.set_bias(2, ids, _noninteger(rng, 40))
    b.params[2] = _params(2.0, -0.25, 1.1)
    b.families[2] = ("stray",)
    for s, kind in ((0, "c32766"), (1, "biased"), (2, "saturated")):
        b.plant_count_id(s, kind)
    return b.build()


def _tiny_case():
    """vocab 8: one 16-byte group, every id of it biased; a banned row; a row without a list."""
    v, ns = 8, 3
    b = _Builder("shape_8", v, ns, (1, -1, 2, 0, ns), 9300)
    b.set_bias(0, b.rng.permutation(8), _noninteger(b.rng, 8))
    b.params[0] = _params(1.3, 0.7, 0.3)
    b.families[0] = ("group",)
    b.set_bias(1, [2, 5], np.array([-np.inf, -np.inf], dtype=np.float32))
    b.params[1] = _params(2.0, -0.25, 1.1)
    b.families[1] = ("banned",)
    b.params[2] = _params(0.5, 1.5, -2.0)
    for s, kind in ((0, "biased"), (1, "prompt_only"), (2, "saturated")):
        b.plant_count_id(s, kind)
    return b.build()


def _cap_case():
    """vocab 393,216, the LDS cap of the bitmap: one processed row, two slots."""
    v, ns = 393216, 2
    b = _Builder("cap_393216", v, ns, (1,), 9400)
    rng = b.rng
    ids = np.concatenate([[v - 1], rng.permutation(v - 2)[:CAP - 2] + 1, [0]])
    b.set_bias(1, ids, _noninteger(rng, CAP))
    b.params[1] = _params(1.3, 0.7, 0.3)
    b.families[1] = ("full", "edges")
    b.plant_count_id(1, "biased")
    return b.build()


ROWS_CASE_NAMES = ("shape_8", "shape_1016", "shape_8192", "main_8200", "shape_32776", "cap_393216")


@functools.lru_cache(maxsize=None)
def rows_case(name: str) -> RowsCase:
    if name == "main_8200":
        return _main_case()
    if name == "shape_8":
        return _tiny_case()
    if name == "cap_393216":
        return _cap_case()
    v = int(name.split("_")[1])
    return _small_case(v, 9200 + v % 97)


@functools.lru_cache(maxsize=None)
def rows_expected(name: str, counted: bool = True):
    return rows_oracle(rows_case(name), counted)
