"""Not a test: the float64 oracle of the one-shot collectives (csrc/kernels/allreduce.hip: custom_all_reduce_kernel,
custom_all_reduce_residual_kernel, custom_all_gather_kernel) and of the tensor-parallel branch of the decode GEMM's
residual epilogue (car_tile_exchange in gemm_decode.hip, car_common.h), the input families, the plan of calls and,
per case, the mutations it claims to notice. test_collective_reference_cpu.py judges all of this on the CPU,
test_collective_kernel_gpu.py judges the kernels by it.

Oracle. Everything is float64 torch; fp32 is modelled by rounding to fp32 after every add (f32()), bf16 by the one
RNE helper bf16(). With x_p the bf16 input of rank p (p = 0 .. W-1):
  all-reduce            out = bf16(s), s = f32(.. f32(f32(x_0 + x_1) + x_2) .. + x_{W-1}); the same on every rank
  all-reduce + residual h = bf16(f32(resid + bf16(s))), ssp[row] = sum of h^2 of the rounded h
  all-gather            out[r, p cols + c] = x_p[r, c], bit for bit
  row-parallel GEMM     y_p = bf16(sum over the split-K slices, in slice order in fp32, of gemm_decode_reference
                        .partials(x_p, w_p)), h = bf16(f32(resid + bf16(s(y)))), ssp_out[tile][row] = sum of h^2 over
                        the tile's wr columns. Rows M .. RR - 1 of ssp_out (RR = the epilogue's row pitch, max(32, XR))
                        are written as 0, which gemm_decode_reference's single-rank test already pins; rows >= RR
                        and everything outside [M, N] of resid stay untouched.
f32(resid + a) is exact whenever the exponents of two bf16 values are within 16 of each other, and where it is not
the fp32 rounding cannot create a bf16 tie, so h has one meaning.

The protocol state is modelled too: every rank owns a staging buffer of two halves; call e (the device epoch after
the call, 1, 2, ...) publishes its message at [0, n) of half e & 1 and reads the peers' there. simulate() keeps those
halves for the whole plan, so a mutation can read what a wrong kernel would read: the other half (call e - 1's message)
or the own input stamped with the previous call. Every input is seeded with the call's epoch (position stamping),
so two calls never carry the same values.

Families (each generator's docstring says what it decides): order, own, twice, exact, random.

Tolerances. Outputs: bit for bit (the random GEMM: the bracket of random_gemm_bracket()). Statistics of the exact
family: bit for bit. Other statistics of the residual kernel: ss_bound(), derived there. Per-tile statistics of the
GEMM outside the exact family: gemm_decode_reference's mode-3 rule, wr 2^-24 ss (one rounding per add of a tile
row's wr terms in any order), restated in gemm_ss_bound().

Plan. PLAN lists every call of the GPU test in the order every rank makes it, with the object it runs on and its
epoch; the parity of every call follows from it, and coverage() reports what the lists reach. plan(world) is PLAN
with every case fitted to what `world` ranks sharing one GPU can keep resident (RESIDENT, fit()): same names, same
epochs, fewer requested workgroups or residual rows at 4 and 8 ranks."""

from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Optional

import torch

from src.ops.decode_tiles import SSP_LD, gd_tile_valid
from tests import gemm_decode_reference as gr

WORLDS = (2, 4, 8)
NTH = 512                   # threads of the collective kernels
MAX_BLOCKS = 256            # flag slots per parity (CAR_MAX_BLOCKS)
MAX_RANKS = 8
MAIN_BYTES = 1 << 20        # max_bytes of the object most cases run on: cap = 512 Ki elements per half
SMALL_BYTES = 256 << 10     # ... of the object whose half the n == cap case fills
CAPS = {"main": MAIN_BYTES // 2, "small": SMALL_BYTES // 2}
SENT = 12352.0              # sentinel of the output buffers (no family produces it)
SENT_I = -7777
MIN_CHANGED = 8
U24 = 2.0 ** -24
# Workgroups of one launch that all the ranks SHARING ONE GPU may keep waiting for each other at once. Every workgroup
# of the all-reduce, residual and gather kernels waits for the same workgroup of every peer, so the W launches only
# drain if all of them are resident together: a 256-CU MI355X holds 4 workgroups of 512 threads per CU, and half of
# that is left free for whatever else runs there. 256 requested workgroups at 8 ranks (2048) ended only at the bounded
# spin with the error word set, which is what the GEMM's fused_exchange_ok guards against and nothing guards here: a
# node runs one rank per GPU. fit() therefore lowers the requested workgroups (and the residual form's rows) of a case
# to RESIDENT / W: 256 (flag slot 255) runs at 2 ranks, 128 at 4, 64 at 8.
RESIDENT = 512


# ---------------------------------------------------------------------------------------------- rounding

def half_ulp_bf16(o: torch.Tensor) -> torch.Tensor:
    _, e = torch.frexp(o.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(o), (e - 1).clamp_min(-126) - 8)


def bf16(o: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (ties to even) in one rounding, as float64: THE bf16 rounding here."""
    sp = 2 * half_ulp_bf16(o)
    return torch.round(o / sp) * sp


def f32(o: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest fp32 value (ties to even), as float64."""
    return o.float().double()


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ---------------------------------------------------------------------------------------------- cases

@dataclass(frozen=True)
class Case:
    name: str
    kind: str                 # ar | res | gat | gemm
    family: str               # order | own | twice | exact | random
    obj: str = "main"
    group: str = "cases"      # cases | seq
    nvec: int = 0             # ar: 16-byte vectors
    blocks: int = 16          # ar, gat: requested workgroups
    inplace: bool = False     # ar
    rows: int = 0             # res, gat, gemm (M)
    hidden: int = 0           # res
    cols: int = 0             # gat
    wr: int = 0               # gemm ..
    kc: int = 128
    sk: int = 1
    tiled: bool = False
    half_ring: bool = False
    ntiles: int = 0
    tch: int = 2              # K chunks per rank
    twin: str = ""            # gemm: the full-ring case whose result this half-ring one must equal bit for bit
    stamp: int = -1           # seq: the pass; cases: unused

    @property
    def n(self) -> int:       # elements of one rank's message
        return {"ar": self.nvec * 8, "res": self.rows * self.hidden, "gat": self.rows * self.cols,
                "gemm": self.rows * self.ntiles * self.wr}[self.kind]

    @property
    def ncols(self) -> int:   # gemm N
        return self.ntiles * self.wr

    @property
    def k(self) -> int:
        return self.tch * self.kc

    @property
    def xr(self) -> int:      # the activation image (row_parallel_residual always loads nt)
        return gr.select_xr(self.wr, self.kc, self.rows, True)

    @property
    def rr(self) -> int:
        return max(32, self.xr)

    @property
    def grid(self) -> int:
        """Workgroups that signal: the launchers' rule, restated (ar / gat: at least 64 vectors each)."""
        if self.kind in ("ar", "gat"):
            nv = self.n // 8
            return min(self.blocks, (nv + 63) // 64)
        return self.rows if self.kind == "res" else self.ntiles

    @property
    def per(self) -> int:     # ar / gat: vectors per workgroup
        nv = self.n // 8
        return (nv + self.grid - 1) // self.grid

    @property
    def unit(self) -> int:
        """Elements between a position and the same position of the neighbouring workgroup's range."""
        return {"ar": self.per * 8, "gat": self.per * 8, "res": self.hidden, "gemm": self.wr}[self.kind]

    @property
    def passes(self) -> int:  # turns of a thread's loop over its workgroup's vectors
        v = self.per if self.kind in ("ar", "gat") else self.hidden // 8
        return (v + NTH - 1) // NTH


def _ar_cases():
    """(nvec, blocks): 1 vector; 64 -> one workgroup; 65 -> two; 512 16 + 1 at 16 blocks: a thread loops twice;
    64 256: all 256 flag slots; 64 256 + 1 at 256 blocks: per = 65, so the last workgroups are empty and still signal;
    n == cap on the small object: the last vector of the staging half. Families and in place / guarded out rotate."""
    spec = [(1, 1, "own"), (1, 16, "random"), (64, 16, "own"), (65, 16, "order"), (65, 1, "random"),
            (512 * 16 + 1, 16, "order"), (512 * 16 + 1, 256, "own"), (64 * 256, 256, "own"), (64 * 256, 1, "random"),
            (64 * 256 + 1, 256, "order"), (64 * 256 + 1, 256, "random")]
    out = []
    for j, (nv, b, fam) in enumerate(spec):
        for inplace in ((False, True) if nv in (1, 64 * 256 + 1) else (bool(j % 2),)):
            out.append(Case(f"ar-v{nv}-b{b}-{fam}-{'in' if inplace else 'out'}", "ar", fam, nvec=nv, blocks=b,
                            inplace=inplace))
    cap = CAPS["small"] // 8
    assert cap == 64 * 256
    out.append(Case(f"ar-cap-b256-own-out", "ar", "own", obj="small", nvec=cap, blocks=256))
    out.append(Case(f"ar-cap-b16-random-in", "ar", "random", obj="small", nvec=cap, blocks=16, inplace=True))
    out.append(Case(f"ar-cap-b1-order-out", "ar", "order", obj="small", nvec=cap, blocks=1))
    return out


def _res_cases():
    """hidden 8 (one vector), 4096 (exactly one 512-thread pass), 4104 (one past it), 8192 (two passes); rows 1, 19,
    128 (flag slots 0 .. 127). Pairs are chosen so that no tensor exceeds a few hundred KiB."""
    spec = [(1, 8, "exact"), (19, 8, "twice"), (128, 8, "exact"), (128, 8, "random"), (1, 4096, "twice"),
            (19, 4096, "exact"), (19, 4096, "random"), (1, 4104, "random"), (19, 4104, "twice"), (19, 4104, "order"),
            (1, 8192, "exact"), (19, 8192, "random"), (19, 8192, "twice"), (19, 8192, "exact")]
    return [Case(f"res-r{r}-h{h}-{fam}", "res", fam, rows=r, hidden=h) for r, h, fam in spec]


def _gat_cases():
    """(rows, cols): a workgroup's slice crosses row ends in each but the first, so row = i / cvec is exercised."""
    out = []
    for r, c in ((1, 8), (3, 8), (24, 4000), (7, 1032)):
        for fam in ("own", "random"):
            out.append(Case(f"gat-r{r}-c{c}-{fam}", "gat", fam, rows=r, cols=c, blocks=16 if fam == "own" else 256))
    return out


def _gemm_cases():
    """Rows 1, 16, 17, 32, 33 (the 16- and 32-row activation images and the first large-M one), tiles (64, 128) and
    (32, 128), sk 1 and 2, row-major and tile-order weights, N = 3 wr and 16 wr alternate over the list; every case
    of <= 32 rows whose tile has a half-ring form runs again on it and must be bit-identical. 16 tiles at 8 ranks
    sharing one GPU is the most the residency rule allows (16 x 8 x 2 = 256 CUs)."""
    out = []
    j = 0
    for wr, kc in ((64, 128), (32, 128)):
        for m in (1, 16, 17, 32, 33):
            sk = 1 + (j + (wr == 32)) % 2
            tiled = bool((j // 2) % 2)
            nt = 16 if j % 3 != 1 else 3
            fam = ("exact", "twice")[(j + j // 5) % 2]
            assert gd_tile_valid(wr, kc, gr.select_xr(wr, kc, m, True))
            c = Case(f"gemm-{wr}x{kc}-m{m}-s{sk}-{'tile' if tiled else 'row'}-n{nt}-{fam}", "gemm", fam, rows=m, wr=wr,
                     kc=kc, sk=sk, tiled=tiled, ntiles=nt, tch=2 * sk)
            out.append(c)
            if m <= 32 and gr.half_ring_slots(wr, kc, c.xr):
                out.append(Case(c.name + "-half", "gemm", fam, rows=m, wr=wr, kc=kc, sk=sk, tiled=tiled, ntiles=nt,
                                tch=2 * sk, half_ring=True, twin=c.name))
            j += 1
    out.append(Case("gemm-64x128-m19-s2-row-n16-random", "gemm", "random", rows=19, wr=64, kc=128, sk=2, ntiles=16,
                    tch=4))
    return out


SEQ_PASSES = 5              # the chain runs eagerly twice, then three replays of one captured graph
SEQ_EAGER = 2
SEQ_ROWS, SEQ_TILES, SEQ_WR = 17, 16, 64


def seq_chain(p: int):
    """One decode layer pair plus the head: row-parallel GEMM -> all-reduce + residual -> row-parallel GEMM ->
    all-reduce -> all-gather. Five calls: the next pass starts on the other parity. The residual stream of a pass is
    one buffer that calls 0 .. 2 update in turn."""
    m, n = SEQ_ROWS, SEQ_TILES * SEQ_WR
    g = dict(group="seq", stamp=p)
    return [Case(f"seq-p{p}-c0-gemm", "gemm", "exact", rows=m, wr=SEQ_WR, sk=2, ntiles=SEQ_TILES, tch=2, **g),
            Case(f"seq-p{p}-c1-res", "res", "exact", rows=m, hidden=n, **g),
            Case(f"seq-p{p}-c2-gemm", "gemm", "exact", rows=m, wr=SEQ_WR, sk=2, ntiles=SEQ_TILES, tch=2, tiled=True, **g),
            Case(f"seq-p{p}-c3-ar", "ar", "own", nvec=m * n // 8, blocks=16, **g),
            Case(f"seq-p{p}-c4-gat", "gat", "own", rows=m, cols=1032, blocks=16, **g)]


AR_CASES, RES_CASES, GAT_CASES, GEMM_CASES = _ar_cases(), _res_cases(), _gat_cases(), _gemm_cases()
SEQ_CASES = [c for p in range(SEQ_PASSES) for c in seq_chain(p)]


def fit(c: Case, world: int) -> Case:
    """The case as a group of `world` ranks on one GPU runs it (see RESIDENT); the name stays."""
    lim = RESIDENT // world
    return replace(c, blocks=min(c.blocks, lim), rows=min(c.rows, lim) if c.kind == "res" else c.rows)


def case(name: str, world: int) -> Case:
    return fit(CASES[name], world)


def plan(world: int):
    return [(fit(c, world), e) for c, e in PLAN]


def _plan():
    """[(case, epoch)] in the order every rank runs them; the epoch counts the launches of the case's object."""
    ep = {"main": 0, "small": 0}
    out = []
    for c in AR_CASES + RES_CASES + GAT_CASES + GEMM_CASES + SEQ_CASES:
        ep[c.obj] += 1
        out.append((c, ep[c.obj]))
    return out, dict(ep)


PLAN, FINAL_EPOCH = _plan()
CASES = {c.name: c for c, _ in PLAN}
EPOCH = {c.name: e for c, e in PLAN}
assert len(CASES) == len(PLAN)
GROUPS = ("ar", "res", "gat", "gemm", "seq")


def group_of(c: Case) -> str:
    return "seq" if c.group == "seq" else c.kind


def names(group: str):
    return [c.name for c, _ in PLAN if group_of(c) == group]


def epoch_after(group: str) -> dict:
    """{object: epoch word} once every call of the groups up to and including `group` has run."""
    ep = {"main": 0, "small": 0}
    for c, e in PLAN:
        if GROUPS.index(group_of(c)) <= GROUPS.index(group):
            ep[c.obj] = e
    return ep


# ---------------------------------------------------------------------------------------------- families

def _gen(c: Case, world: int, epoch: int) -> torch.Generator:
    return torch.Generator().manual_seed((zlib.crc32(c.name.encode()) + 1000003 * epoch + 7919 * world) % (1 << 31))


def _scale(gen, n, lo=-6, hi=6):
    k = torch.randint(lo, hi + 1, (n,), generator=gen)
    s = torch.randint(0, 2, (n,), generator=gen) * 2 - 1
    return s.double() * torch.ldexp(torch.ones(n, dtype=torch.float64), k)


def fam_order(world: int, n: int, gen) -> torch.Tensor:
    """[W, n]. Decides the ORDER of the fp32 sum. Per element the ranks hold A = +-2^k at rank i, -A at an even rank
    j > i, a = 2^(k-26) (same sign as A) at rank j + 1 and zeros elsewhere. a is far below half an fp32 ulp of A (the
    issue's 2^(k-24) is a tie in one direction and representable in the other, so the triple is moved two bits down):
    added while the running sum is +-A it is lost, added after A and -A have cancelled it survives. Rank order gives
    a; the reversed order meets a first and loses it in A (0); the pairwise tree adds -A + a first and loses it (0).
    i, j, k and the sign vary per element. W = 2: order cannot matter for two terms; the ranks hold 2^k and 3 2^(k-1)
    so that dropping either is visible."""
    sc = _scale(gen, n)
    x = torch.zeros(world, n, dtype=torch.float64)
    if world == 2:
        x[0], x[1] = sc, 1.5 * sc
        return x
    j = 2 * torch.randint(1, world // 2, (n,), generator=gen)
    i = (torch.rand(n, generator=gen) * j).long().clamp_max(world - 1)
    big = sc * 2.0 ** 20
    col = torch.arange(n)
    x[i, col] = big
    x[j, col] = -big
    x[j + 1, col] = big * 2.0 ** -26
    return x


def fam_own(world: int, n: int, gen) -> torch.Tensor:
    """[W, n]. Decides WHICH ranks are summed, once each: rank p holds +-2^(p + k) with k and the sign per element, so
    the sum (2^W - 1) 2^k has at most 8 significant bits (exact in bf16) and its bit pattern names the ranks: a
    dropped rank clears a bit, a doubled one carries."""
    sc = _scale(gen, n)
    return torch.stack([sc * 2.0 ** p for p in range(world)])


def fam_twice(world: int, n: int, gen):
    """([W, n], resid [n]). Decides the intermediate bf16 rounding of the residual forms: the sum is 257 (a bf16 tie
    that goes to 256) with resid 0.5, or 259 (-> 260) with resid -0.5, times +-2^k. Two roundings give 256 and 260,
    one rounding of resid + s gives 258 both times. Two ranks hold 256 and 1 (or 3), the others 0."""
    sc = _scale(gen, n, -3, 3)
    t = torch.randint(0, 2, (n,), generator=gen)
    i = torch.randint(0, world, (n,), generator=gen)
    j = (i + torch.randint(1, world, (n,), generator=gen)) % world
    col = torch.arange(n)
    x = torch.zeros(world, n, dtype=torch.float64)
    x[i, col] = 256.0 * sc
    x[j, col] = (1.0 + 2.0 * t) * sc
    return x, (0.5 - t.double()) * sc


def fam_exact(world: int, n: int, gen):
    """([W, n], resid [n]). Integers +-{1..3} per rank and +-{1..4} in the residual, no zeros: every sum is exact
    in fp32 in any order, |h| <= 28 is exact in bf16, and sum of h^2 < 2^24 per row, so residual AND statistics are
    bit for bit; dropping or doubling any rank moves every element."""
    return gr._signed(gen, (world, n), 3).double(), gr._signed(gen, (n,), 4).double()


def fam_random(world: int, n: int, gen):
    """([W, n], resid [n]). Seeded randn rounded to bf16: magnitudes like the workload's."""
    return (torch.randn(world, n, generator=gen).to(torch.bfloat16).double(),
            torch.randn(n, generator=gen).to(torch.bfloat16).double())


def fam_gather_own(world: int, n: int, gen) -> torch.Tensor:
    """[W, n] bf16. Decides WHERE every element of the gather comes from: bits 11..13 hold the rank, the low 11 bits
    a seeded hash of the position (bit 14 clear: every pattern is a finite bf16)."""
    h = torch.randint(0, 1 << 11, (n,), generator=gen)
    pat = (torch.arange(world)[:, None] << 11) | h[None, :]
    return pat.to(torch.int16).view(torch.bfloat16)


def inputs(name: str, world: int, shift: int = 0) -> SimpleNamespace:
    """The tensors of a call as every rank gets them: xs [W, ...] bf16 (rank p's input is xs[p]), resid bf16,
    ws [W, N, K] bf16 for the GEMM, stamped with the call's epoch; shift = -1 gives the values the previous call
    would have stamped. A half-ring GEMM case takes the inputs of its full-ring twin, stamp included: the two results
    have to be bit-identical, and the twin and the sequences carry the stamping."""
    c = case(name, world)
    src = case(c.twin, world) if c.twin else c
    epoch = EPOCH[src.name] + shift
    gen = _gen(src, world, epoch)
    i = SimpleNamespace(c=c, epoch=epoch, resid=None)
    n = c.n
    if c.kind == "gemm":
        m, nn, k = c.rows, c.ncols, c.k
        if c.family == "exact":
            x, w = gr._signed(gen, (world, m, k), 1), gr._signed(gen, (world, nn, k), 1)
            r = gr._signed(gen, (m, nn), 4)
        elif c.family == "twice":
            # integer partials with 256 < |y_p| < 2^15: bf16 keeps 8 bits of them, so the rounding before the
            # exchange acts, and their sum falls between bf16 values, so the rounding after it acts too
            x = torch.randint(1, 3, (world, m, k), generator=gen).to(torch.bfloat16)
            sg = torch.randint(0, 2, (1, nn, 1), generator=gen) * 2 - 1
            w = (torch.randint(1, 4, (world, nn, k), generator=gen) * sg).to(torch.bfloat16)
            r = (gr._signed(gen, (m, nn), 8).double() * 8).to(torch.bfloat16)
        else:
            x = torch.randn(world, m, k, generator=gen).to(torch.bfloat16)
            w = (torch.randn(world, nn, k, generator=gen) / k ** 0.5).to(torch.bfloat16)
            r = torch.randn(m, nn, generator=gen).to(torch.bfloat16)
        i.xs, i.ws, i.resid = x, w, r
        return i
    if c.kind == "gat" and c.family == "own":
        i.xs = fam_gather_own(world, n, gen).view(world, c.rows, c.cols)
        return i
    if c.family == "order":
        x, r = fam_order(world, n, gen), None
        if c.kind == "res":
            r = 3.0 * x.abs().max(0).values * 2.0 ** -26     # 3 a: h = 4 a in rank order, 3 a in the others
    elif c.family == "own":
        x, r = fam_own(world, n, gen), None
    else:
        x, r = {"twice": fam_twice, "exact": fam_exact, "random": fam_random}[c.family](world, n, gen)
    shape = {"ar": (n,), "res": (c.rows, c.hidden), "gat": (c.rows, c.cols)}[c.kind]
    i.xs = x.to(torch.bfloat16).view(world, *shape)
    assert torch.equal(i.xs.double().view(world, -1), x), f"{name}: a family value is no bf16"
    if c.kind == "res":
        i.resid = r.to(torch.bfloat16).view(shape)
        assert torch.equal(i.resid.double().view(-1), r)
    return i


def seq_resid(p: int, world: int) -> torch.Tensor:
    """The residual stream a pass of the sequence starts from (calls 0 .. 2 then update it in turn)."""
    gen = torch.Generator().manual_seed(4242 + 31 * p + world)
    return gr._signed(gen, (SEQ_ROWS, SEQ_TILES * SEQ_WR), 4)


# ---------------------------------------------------------------------------------------------- oracle

def rank_sum(v: torch.Tensor, order=None) -> torch.Tensor:
    """The fp32 sum of v[p] over `order` (default: rank order 0 .. W-1), every add rounded to fp32."""
    s = torch.zeros_like(v[0])
    for p in (range(v.shape[0]) if order is None else order):
        s = f32(s + v[p])
    return s


def tree_sum(v: torch.Tensor) -> torch.Tensor:
    """The pairwise tree ((v0 + v1) + (v2 + v3)) + ..., every add rounded to fp32."""
    level = [v[p] for p in range(v.shape[0])]
    while len(level) > 1:
        level = [f32(level[q] + level[q + 1]) for q in range(0, len(level), 2)]
    return level[0]


def gemm_partial(c: Case, x: torch.Tensor, w: torch.Tensor):
    """(y fp32-modelled [M, N], |x| |w|^T): one rank's K-shard product as the tile's last arriver holds it, the
    split-K slices of gemm_decode_reference.partials added in slice order."""
    parts = gr.partials(x.double(), w.double(), c.kc, c.sk)
    y = f32(parts[0])
    for q in range(1, c.sk):
        y = f32(y + f32(parts[q]))
    return y, x.double().abs() @ w.double().abs().T


def ss_depth(hidden: int) -> int:
    """Roundings on the longest path of the residual kernel's row statistic: a thread adds its
    ceil(hidden / 8 / 512) vectors' 8 squares one after the other (the squares of bf16 values are exact in fp32, and
    the first add to 0 is exact, counted all the same), six xor-shuffle levels merge a wave's 64 lanes, and thread 0
    adds the eight waves' sums in turn."""
    return ((hidden // 8 + NTH - 1) // NTH) * 8 + 6 + 8


def ss_bound(ss: torch.Tensor, hidden: int) -> torch.Tensor:
    """|kernel - exact| for a sum of non-negative terms along a path of d roundings: every rounding is relative
    2^-24 of a partial sum that is at most the final one, so gamma_d ss with gamma_d = d u / (1 - d u), u = 2^-24."""
    d = ss_depth(hidden) * U24
    return d / (1 - d) * ss


def gemm_ss_bound(ss: torch.Tensor, wr: int) -> torch.Tensor:
    """gemm_decode_reference's rule for mode 3's per-tile statistics (its random family): wr 2^-24 ss."""
    return wr * U24 * ss


def gather(xs: torch.Tensor) -> torch.Tensor:
    """[W, rows, cols] -> [rows, W cols], rank-major along the last dimension."""
    return torch.cat([xs[p] for p in range(xs.shape[0])], -1)


MUTATIONS = ("drop", "double", "prev_stamp", "neighbour", "reversed", "no_mid_round", "ss_unrounded", "ss_drop_chunk",
             "ss_next_row", "rank_minor", "cvec_plus", "cvec_minus", "partial_unrounded", "neighbour_tile", "clamp_row",
             "other_half", "own_other_half")


def claims(c: Case, world: int) -> tuple:
    """The mutations this case has to notice (each: >= MIN_CHANGED elements, or all of a smaller case; a statistic:
    by more than 4 times its tolerance)."""
    m = [] if c.twin else ["other_half", "own_other_half", "prev_stamp"]
    if c.n <= MIN_CHANGED and c.family != "random":
        # one vector, and all of it would have to change: two stamps of a small alphabet agree somewhere (own: one
        # of 26 values per element, exact: one of 6), so these leave the stamp to the cases around them
        m = ["other_half", "own_other_half"] if c.family == "own" else []
    if c.kind == "gat":
        m += ["rank_minor"] + (["cvec_plus", "cvec_minus"] if c.rows > 1 else [])
        if c.grid > 1 and c.family == "random":
            m.append("neighbour")
        return tuple(m)
    if c.family in ("own", "exact", "random"):
        m += ["drop", "double"]
    if c.family == "order" and world > 2:
        m.append("reversed")
    if c.family == "twice":
        m.append("no_mid_round")
    if c.kind == "ar":
        if c.grid > 1 and c.family in ("own", "random") and c.n // 8 - c.per >= MIN_CHANGED:
            m.append("neighbour")
    if c.kind == "res":
        if c.family != "order":                 # its magnitudes span 2^12: the weakest chunk is below the bound
            m.append("ss_drop_chunk")
        if c.family in ("twice", "random"):
            m.append("ss_unrounded")
        if c.rows > 1:
            m += ["ss_next_row", "neighbour"]
    if c.kind == "gemm":
        m += ["neighbour_tile", "ss_drop_chunk"]
        if c.family == "twice":
            m += ["partial_unrounded", "ss_unrounded"]
        if c.rows > 1:
            m += ["clamp_row", "ss_next_row"]
    return tuple(m)


def evaluate(name: str, world: int, st: SimpleNamespace, mut: Optional[str] = None, who: int = 0, me: int = 1):
    """The expectation of call `name` for rank `me`, or what a kernel with mutation `mut` would return there.
    st: the call's record from simulate() (inputs, messages, the staging halves before the call). who: the rank a
    drop / double mutation acts on. Returns out (float64, or bf16 for the gather), ss, and for the GEMM y [W, M, N]."""
    c, i = st.c, st.i
    e = SimpleNamespace(ss=None, out=None)
    if c.kind == "gat":
        xs = i.xs.clone()
        if mut == "prev_stamp":
            xs[me] = inputs(name, world, -1).xs[me]
        if mut == "other_half":
            for p in range(world):
                if p != me:
                    xs[p] = st.stale[p].to(torch.bfloat16).view(c.rows, c.cols)
        if mut == "own_other_half":
            xs[me] = st.stale[me].to(torch.bfloat16).view(c.rows, c.cols)
        if mut == "neighbour":
            for p in range(world):
                if p != me:
                    xs[p] = torch.roll(xs[p].reshape(-1), -c.unit).view(c.rows, c.cols)
        if mut == "rank_minor":
            e.out = xs.permute(1, 2, 0).reshape(c.rows, c.cols * world)
        elif mut in ("cvec_plus", "cvec_minus"):
            # dst[(row W + p) cvec + c] with row = i / cvec', c = i - row cvec', cvec' = cvec +- 1: a scatter, the
            # positions nobody writes keep the sentinel
            cv, cv2 = c.cols // 8, c.cols // 8 + (1 if mut == "cvec_plus" else -1)
            iv = torch.arange(c.n // 8)
            out = torch.full((c.rows * world * cv + 2 * world * cv, 8), SENT, dtype=torch.bfloat16)
            for p in range(world):
                if cv2 == 0:
                    continue
                row = iv // cv2
                out[((row * world + p) * cv + iv - row * cv2).clamp(0, out.shape[0] - 1)] = xs[p].reshape(-1, 8)
            e.out = out[: c.rows * world * cv].reshape(c.rows, world * c.cols)
        else:
            e.out = gather(xs)
        return e
    # the reducing kinds: msgs [W, n] float64 is what each rank published
    if c.kind == "gemm":
        msgs = (st.y_raw if mut == "partial_unrounded" else st.msgs).clone()
    else:
        msgs = st.msgs.clone()
    shape = msgs.shape[1:]
    if mut == "prev_stamp":
        msgs[me] = st.prev_msg[me]
    if mut == "other_half":
        for p in range(world):
            if p != me:
                msgs[p] = st.stale[p].double().view(shape)
    if mut == "own_other_half":                 # the own term read back from staging, and from the wrong half
        msgs[me] = st.stale[me].double().view(shape)
    if mut == "neighbour":
        for p in range(world):
            if p != me:
                msgs[p] = torch.roll(msgs[p].reshape(-1), -c.unit).view(shape)
    if mut == "neighbour_tile":
        for p in range(world):
            if p != me:
                msgs[p] = torch.roll(msgs[p], -c.wr, dims=-1)
    if mut == "clamp_row":                      # min(m, M - 1) taken one row too early: the last row reads its neighbour
        for p in range(world):
            if p != me:
                msgs[p][-1] = msgs[p][-2]
    order = list(range(world))
    if mut == "drop":
        order.remove(who)
    if mut == "double":
        order.insert(who, who)
    if mut == "reversed":
        order.reverse()
    s = rank_sum(msgs, order)
    if c.kind == "ar":
        e.out = bf16(s)
        return e
    a = s if mut == "no_mid_round" else bf16(s)
    resid = st.resid.double()
    h32 = f32(resid + a)
    e.out = bf16(h32)
    sq = (h32 if mut == "ss_unrounded" else e.out) ** 2
    if mut == "ss_drop_chunk":                  # the weakest 16-byte chunk of every row (of every tile row) left out
        ch = sq.reshape(sq.shape[0], -1, 8).sum(-1)
        if c.kind == "gemm":
            ch = ch.view(c.rows, c.ntiles, c.wr // 8)
            idx = ch.argmin(-1, keepdim=True)
            ch = ch.scatter(-1, idx, 0.0).view(c.rows, -1)
        else:
            ch = ch.scatter(-1, ch.argmin(-1, keepdim=True), 0.0)
        sq = None
    if c.kind == "res":
        e.ss = sq.sum(-1) if sq is not None else ch.sum(-1)
    else:
        t = (sq.view(c.rows, c.ntiles, c.wr).sum(-1) if sq is not None
             else ch.view(c.rows, c.ntiles, c.wr // 8).sum(-1))
        e.ss = t.T.contiguous()                 # [tile, M]
    if mut == "ss_next_row":
        e.ss = torch.roll(e.ss, -1, dims=-1)
    return e


@functools.lru_cache(maxsize=None)
def simulate(world: int) -> dict:
    """Runs PLAN for a group of `world` ranks: {name: record} with the inputs, the published messages, the staging
    halves as the call found them and the expectation `exp`."""
    stage = {o: torch.zeros(world, 2, cap, dtype=torch.float32) for o, cap in CAPS.items()}
    out = {}
    stream = None
    for c, epoch in plan(world):
        i = inputs(c.name, world)
        st = SimpleNamespace(c=c, i=i, epoch=epoch, par=epoch & 1, resid=i.resid)
        n = c.n
        assert n <= CAPS[c.obj], c.name
        prev = inputs(c.name, world, -1)
        if c.group == "seq":                    # the pass's residual stream, handed from call to call
            k = int(c.name.split("-c")[1][0])
            if k == 0:
                stream = seq_resid(c.stamp, world)
            if k < 3:
                st.resid = stream
        if c.kind == "gemm":
            ys, ab = zip(*(gemm_partial(c, i.xs[p], i.ws[p]) for p in range(world)))
            st.y_raw, st.absum = torch.stack(ys), torch.stack(ab)
            st.msgs = bf16(st.y_raw)
            st.prev_msg = bf16(torch.stack([gemm_partial(c, prev.xs[p], prev.ws[p])[0] for p in range(world)]))
        else:
            st.msgs = i.xs.double()
            st.prev_msg = prev.xs.double()
        half = stage[c.obj]
        st.stale = half[:, 1 - st.par, :n].clone()
        half[:, st.par, :n] = (i.xs.float() if c.kind == "gat" else st.msgs.float()).reshape(world, -1)
        st.exp = evaluate(c.name, world, st)
        if c.group == "seq" and c.kind != "ar" and st.exp.ss is not None:
            stream = st.exp.out.to(torch.bfloat16)
        out[c.name] = st
    return out


def random_gemm_bracket(st: SimpleNamespace):
    """(lo, hi) float64 of the random GEMM's residual. The kernel's fp32 partial differs from the exact product y_p
    by at most E_p = (K + sk) 2^-24 sum |x w| (gemm_decode_reference's bound: every product added one at a time, the
    worst any order can do). RNE to bf16, the fp32 adds of the rank-order sum and the final rounding are all monotone,
    so the chain applied to y_p - E_p and to y_p + E_p brackets what the kernel may write; where both ends agree the
    element is decided bit for bit."""
    c = st.c
    ex = torch.stack([gr.partials(st.i.xs[p].double(), st.i.ws[p].double(), c.kc, c.sk).sum(0)
                      for p in range(st.msgs.shape[0])])
    err = (c.k + c.sk) * U24 * st.absum
    resid = st.resid.double()
    return tuple(bf16(f32(resid + bf16(rank_sum(bf16(ex + sg * err))))) for sg in (-1.0, 1.0))


# ---------------------------------------------------------------------------------------------- premises, coverage

def premise(name: str, world: int) -> dict:
    """Asserts the premise of the case's family; returns figures."""
    st = simulate(world)[name]
    c = st.c
    fig = {}
    if c.kind == "gat":
        return fig
    if c.family == "order":
        if world == 2:
            fig["excepted"] = "W = 2: two terms have one order; both terms are non-zero instead"
            assert bool((st.msgs != 0).all())
            return fig
        ro, rev, tree = rank_sum(st.msgs), rank_sum(st.msgs, reversed(range(world))), tree_sum(st.msgs)
        assert bool((bf16(ro) != bf16(rev)).all()) and bool((bf16(ro) != bf16(tree)).all()), name
    if c.family == "twice":
        resid = st.resid.double()
        s = rank_sum(st.msgs)
        one, two = bf16(f32(resid + s)), bf16(f32(resid + bf16(s)))
        if c.kind == "gemm":
            y = st.y_raw.abs()
            assert bool((y > 256).all()) and bool((y < 2 ** 15).all()), name
            # a partial in (256, 2^15) is an integer where bf16 values are >= 2 apart: at least half of them move.
            # Two rounded partials of one binade (spacing u) add up to a multiple of u in the next binade (spacing
            # 2 u): about half of the sums are odd multiples, fewer where the binades differ, more with more ranks;
            # a seeded case has to reach half of that
            fig["sum_off_grid"] = float((bf16(s) != s).double().mean())
            fig["partial_off_grid"] = float((st.msgs != st.y_raw).double().mean())
            assert fig["sum_off_grid"] >= 0.25 and fig["partial_off_grid"] >= 0.5, (name, fig)
        else:
            assert bool((one != two).all()), name
    if c.family == "exact":
        assert float(st.exp.ss.max()) < 2 ** 24, name
        if c.kind == "gemm":
            assert float(st.absum.max()) < 2 ** 24, name
            assert bool((st.y_raw == st.y_raw.round()).all())
    if c.family == "random" and c.kind in ("res", "gemm"):
        # the bound on the statistic against the smallest effect a mutation has on it: leaving out the weakest
        # 16-byte chunk of a row must move it by more than 4 bounds
        tol = ss_bound(st.exp.ss, c.hidden) if c.kind == "res" else gemm_ss_bound(st.exp.ss, c.wr)
        eff = (st.exp.ss - evaluate(name, world, st, "ss_drop_chunk").ss).abs()
        fig["fraction"] = float((tol / eff).max())
        assert fig["fraction"] <= 0.25, (name, fig)
    return fig


def coverage(world: int = 2) -> dict:
    """What the plan of a group of `world` ranks reaches, for the CPU test to assert."""
    cov = {"parity": {k: set() for k in ("ar", "res", "gat", "gemm")}, "slots": set(), "passes": set(), "xr": set(),
           "ring": set(), "sk": set(), "tiled": set(), "empty_wg": False}
    for c, e in plan(world):
        cov["parity"][c.kind].add(e & 1)
        cov["slots"] |= {0, c.grid - 1}
        if c.kind in ("ar", "gat", "res"):
            cov["passes"].add(min(c.passes, 2))
        if c.kind in ("ar", "gat") and c.per * (c.grid - 1) >= c.n // 8:
            cov["empty_wg"] = True
        if c.kind == "gemm":
            cov["xr"].add(c.xr)
            cov["ring"].add(c.half_ring)
            cov["sk"].add(min(c.sk, 2))
            cov["tiled"].add(c.tiled)
    return cov
