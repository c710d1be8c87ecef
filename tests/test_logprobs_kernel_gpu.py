"""ops.token_logprobs (token_logprobs_kernel, csrc/kernels/sampling.hip): ids and ranks exactly, logprobs within
the bound derived in tests/token_logprobs_reference.py,
    tol = (N_add(vocab) + c_exp + c_log) * 2^-24 + 2^-23 * |lp|        (1.0e-5 + 1.2e-7 |lp| at vocab 128,256).

The named cases of that module (ladder, zero, slabs, rank, mass, random: rows built from bf16 bit patterns, each
reaching one branch of the kernel, proven on the CPU by tests/test_token_logprobs_reference_cpu.py) are judged by
its float64 oracle. The workload-shaped tests below them compare with ref.token_logprobs, which returns fp32: its
own rounding, 2^-24 |lp|, is added to the bound there."""

import functools
import math

import pytest
import torch

from src import ops
from src.ops import reference as ref

from tests import token_logprobs_reference as tlr

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOPS = (0, 1, 5, 20)


def strided(x: torch.Tensor, stride: int) -> torch.Tensor:
    """x [R, V] as bf16 rows `stride` apart on the GPU; the gap holds large finite values, so a read past the
    vocabulary would show in every result."""
    rows, vocab = x.shape
    buf = torch.full((rows, stride), 1000.0, dtype=torch.bfloat16)
    buf[:, :vocab] = x.to(torch.bfloat16)
    return buf.to(DEV)[:, :vocab]


@functools.lru_cache(maxsize=None)
def case(kind: str, rows: int, vocab: int):
    """(bf16 logits on the CPU, targets, the oracle at N = 20): computed once, shared by the stride variants."""
    g = torch.Generator().manual_seed(1000 * rows + vocab % 997 + len(kind))
    if kind == "gauss":   # boundary ties: among the top 21 of a 128K bf16 row only 15-18 values are distinct
        x = torch.randn(rows, vocab, generator=g) * 4
    else:                 # integers in [-3, 3]: massive ties
        x = torch.randint(-3, 4, (rows, vocab), generator=g).float()
    x = x.to(torch.bfloat16)
    t = torch.randint(0, vocab, (rows,), generator=g)
    t[0] = int(ref.token_logprobs(x[:1], torch.zeros(1, dtype=torch.long), 1)[3][0, 0])  # the argmax of row 0
    if rows > 1:
        t[1] = vocab + 5   # out of range
    if rows > 2:
        t[2] = -1
    return x, t, ref.token_logprobs(x, t, 20)


def tol_vs_fp32_ref(vocab: int, want: torch.Tensor) -> torch.Tensor:
    """The derived bound at the reference's values, plus the fp32 reference's own rounding."""
    return torch.from_numpy(tlr.tol_of(vocab, want.double().numpy())) + 2.0 ** -24 * want.double().abs()


def check(got, want, n: int, vocab: int):
    lp, rank, top_lp, top_id = (g.cpu() for g in got)
    wlp, wrank, wtop_lp, wtop_id = want
    assert torch.equal(rank, wrank)
    assert torch.equal(top_id, wtop_id[:, :n])
    worst = 0.0
    for a, b in ((lp, wlp), (top_lp, wtop_lp[:, :n])):
        fin = torch.isfinite(b)
        assert torch.equal(a[~fin], b[~fin])  # -inf exactly
        if fin.any():
            ratio = (a[fin].double() - b[fin].double()).abs() / tol_vs_fp32_ref(vocab, b[fin])
            worst = max(worst, ratio.max().item())
    assert worst <= 1.0, worst
    return worst


SENT_F, SENT_I, WIDE = 7.0, -7, 24


def launch_case(c):
    """One launch of a named case: logits in a strided buffer with a loud gap, outputs in sentinel-filled buffers
    one row longer and wider than asked. Returns the four whole buffers on the CPU."""
    rows = c.bits.shape[0]
    x = torch.from_numpy(c.bits.view("int16")).view(torch.bfloat16)
    logits = strided(x, c.vocab + 64)
    assert logits.stride(0) == c.vocab + 64
    out = (torch.full((rows + 1,), SENT_F, device=DEV), torch.full((rows + 1,), SENT_I, dtype=torch.int32, device=DEV),
           torch.full((rows + 1, WIDE), SENT_F, device=DEV),
           torch.full((rows + 1, WIDE), SENT_I, dtype=torch.int32, device=DEV))
    got = ops.token_logprobs(logits, torch.from_numpy(c.targets).to(DEV), c.top_n, out=out)
    assert got[2].shape == (rows, c.top_n) and got[3].shape == (rows, c.top_n)
    torch.cuda.synchronize()
    return tuple(o.cpu() for o in out)


@pytest.mark.parametrize("name", tlr.case_names())
def test_named_case_matches_the_float64_oracle(name):
    c = tlr.by_name(name)
    (wlp, wrank, wtop_lp, wtop_id), (tol_lp, tol_top) = tlr.expected(name)
    rows, n = c.bits.shape[0], c.top_n
    lp, rank, top_lp, top_id = launch_case(c)
    again = launch_case(c)
    for a, b in zip((lp, rank, top_lp, top_id), again):      # two launches, bit for bit
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # beyond what was asked for, the sentinels stand
    assert lp[rows] == SENT_F and rank[rows] == SENT_I
    assert bool((top_lp[:, n:] == SENT_F).all()) and bool((top_id[:, n:] == SENT_I).all())
    assert bool((top_lp[rows] == SENT_F).all()) and bool((top_id[rows] == SENT_I).all())
    assert torch.equal(rank[:rows].long(), torch.from_numpy(wrank))
    assert torch.equal(top_id[:rows, :n].long(), torch.from_numpy(wtop_id))
    worst = 0.0
    for a, b, tol in ((lp[:rows], wlp, tol_lp), (top_lp[:rows, :n], wtop_lp, tol_top)):
        a, b, tol = a.double(), torch.from_numpy(b), torch.from_numpy(tol)
        fin = torch.isfinite(b)
        assert torch.equal(a[~fin], b[~fin])                  # -inf exactly
        if fin.any():
            worst = max(worst, ((a[fin] - b[fin]).abs() / tol[fin]).max().item())
    print(f"RATIO {c.family} {name} {worst:.3f}")
    assert worst <= 1.0, worst


def test_row_without_a_finite_entry_stays_in_range():
    """Outside the numeric contract: only the ids are judged, and that the launch ends cleanly."""
    vocab = 1000
    x = torch.full((2, vocab), -math.inf, dtype=torch.bfloat16)
    for n in (5, 20):
        lp, rank, top_lp, top_id = ops.token_logprobs(strided(x, vocab + 64), torch.tensor([5, 999], device=DEV), n)
        torch.cuda.synchronize()
        assert 0 <= int(top_id.min()) and int(top_id.max()) < vocab


def test_launcher_rejects_top_n_beyond_the_vocabulary_or_the_buffers():
    t = torch.zeros(1, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError):
        ops.token_logprobs(torch.zeros(1, 8, dtype=torch.bfloat16, device=DEV), t, 20)      # top_n > vocab
    out = (torch.full((1,), SENT_F, device=DEV), torch.full((1,), SENT_I, dtype=torch.int32, device=DEV),
           torch.full((1, 4), SENT_F, device=DEV), torch.full((1, 4), SENT_I, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.token_logprobs(torch.zeros(1, 1000, dtype=torch.bfloat16, device=DEV), t, 5, out=out)  # top_stride < top_n
    torch.cuda.synchronize()
    assert out[0][0] == SENT_F and out[1][0] == SENT_I and bool((out[2] == SENT_F).all())   # nothing ran


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("vocab", [1000, 32000, 128256])
@pytest.mark.parametrize("rows", [1, 7, 33])
@pytest.mark.parametrize("kind", ["gauss", "ints"])
def test_matches_oracle(kind, rows, vocab, pad):
    x, t, want = case(kind, rows, vocab)
    logits = strided(x, vocab + pad)
    assert logits.stride(0) == vocab + pad
    tg = t.to(DEV)
    for n in TOPS:
        got = ops.token_logprobs(logits, tg, n)
        assert got[2].shape == (rows, n) and got[3].shape == (rows, n)
        check(got, want, n, vocab)
    lp, rank, top_lp, top_id = (g.cpu() for g in ops.token_logprobs(logits, tg, 20))
    # a target equal to the argmax: rank 0, first of the list, the list's first logprob is its logprob
    assert rank[0] == 0 and top_id[0, 0] == t[0] and top_lp[0, 0] == lp[0]
    if rows > 2:  # out-of-range targets: -inf and rank vocab
        assert lp[1] == -math.inf and rank[1] == vocab and lp[2] == -math.inf and rank[2] == vocab
    if kind == "ints":
        # independent of the oracle: the list is the first 20 ids that hold the row's maximum (3), in id order
        for r in range(rows):
            first = (x[r].float() == 3).nonzero()[:20, 0]
            assert first.numel() == 20 and torch.equal(top_id[r].long(), first)


def test_constant_row():
    vocab = 32000
    logits = torch.full((3, vocab), 1.5, dtype=torch.bfloat16, device=DEV)
    t = torch.tensor([0, 77, vocab - 1], device=DEV)
    for n in TOPS:
        lp, rank, top_lp, top_id = (g.cpu() for g in ops.token_logprobs(logits, t, n))
        assert rank.tolist() == [0, 77, vocab - 1]            # the target's rank equals its id
        assert torch.equal(top_id, torch.arange(n, dtype=torch.int32).expand(3, n))
        tol = float(tlr.tol_of(vocab, -math.log(vocab)))
        assert (lp.double() + math.log(vocab)).abs().max() <= tol
        assert n == 0 or (top_lp.double() + math.log(vocab)).abs().max() <= tol


@pytest.mark.parametrize("vocab", [1000, 128256])
def test_mostly_minus_inf_row(vocab):
    g = torch.Generator().manual_seed(vocab)
    x = (torch.randn(4, vocab, generator=g) * 4).to(torch.bfloat16)
    dead = torch.rand(4, vocab, generator=g) < 0.9
    x[dead] = -math.inf
    t = torch.stack([(~dead[r]).nonzero()[0, 0] for r in range(4)])
    t[0] = dead[0].nonzero()[5, 0]                          # one target on a -inf entry
    want = ref.token_logprobs(x, t, 20)
    for pad in (0, 64):
        logits = strided(x, vocab + pad)
        for n in TOPS:
            got = ops.token_logprobs(logits, t.to(DEV), n)
            check(got, want, n, vocab)
            assert got[0][0].item() == -math.inf
            assert n == 0 or (0 <= int(got[3].min()) and int(got[3].max()) < vocab)


def test_fewer_finite_entries_than_asked():
    """3 finite entries, 20 asked: the -inf ties fill the list in id order, logprob -inf."""
    vocab = 1000
    x = torch.full((1, vocab), -math.inf, dtype=torch.bfloat16)
    x[0, [900, 17, 450]] = torch.tensor([2.0, 1.0, 2.0], dtype=torch.bfloat16)
    t = torch.tensor([17])
    check(ops.token_logprobs(x.to(DEV), t.to(DEV), 20), ref.token_logprobs(x, t, 20), 20, vocab)


def test_outlier_above_a_flat_row():
    """The top entries lie further apart than the kernel's window of 256 bf16 values below the maximum (its
    general radix select finds the threshold), or straddle the window's edge."""
    vocab = 32000
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(3, vocab, generator=g) * 0.01).to(torch.bfloat16)
    x[0, 5] = 50.0
    x[1, [7, 31999]] = torch.tensor([50.0, 12.0], dtype=torch.bfloat16)
    x[2, :] = -x[2].abs() - 1.0
    x[2, 100] = 3.0                       # keys that cross zero
    t = torch.tensor([5, 9, 100])
    want = ref.token_logprobs(x, t, 20)
    for n in TOPS:
        check(ops.token_logprobs(x.to(DEV), t.to(DEV), n), want, n, vocab)


def test_signed_zeros_tie():
    """-0.0 == +0.0 in a float compare and in the reference's sort: they tie, and the lower id goes first."""
    vocab = 1000
    x = torch.full((1, vocab), -1.0, dtype=torch.bfloat16)
    x[0, 10], x[0, 20], x[0, 30] = -0.0, 0.0, -0.0
    t = torch.tensor([30])
    want = ref.token_logprobs(x, t, 5)
    assert want[3][0, :3].tolist() == [10, 20, 30] and want[1][0] == 2
    check(ops.token_logprobs(x.to(DEV), t.to(DEV), 5), want, 5, vocab)


def test_all_nan_row_stays_in_range():
    vocab = 32000
    x = torch.full((2, vocab), math.nan, dtype=torch.bfloat16, device=DEV)
    x[1] = -x[1]  # both NaN signs
    for n in TOPS:
        lp, rank, top_lp, top_id = ops.token_logprobs(x, torch.tensor([5, 6], device=DEV), n)
        torch.cuda.synchronize()
        assert n == 0 or (0 <= int(top_id.min()) and int(top_id.max()) < vocab)


def test_out_buffers_wider_than_top_n():
    """The engine's layout: lists 20 wide, a launch with top_n 5 writes 5 columns and leaves the rest."""
    x, t, want = case("gauss", 7, 32000)
    out = (torch.zeros(8, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV),
           torch.full((8, 20), 7.0, device=DEV), torch.full((8, 20), -7, dtype=torch.int32, device=DEV))
    got = ops.token_logprobs(x.to(DEV), t.to(DEV), 5, out=out)
    check(got, want, 5, 32000)
    assert bool((out[2][:, 5:] == 7.0).all()) and bool((out[3][:, 5:] == -7).all())
    assert bool((out[2][7] == 7.0).all())


def test_launcher_rejects_bad_arguments():
    t = torch.zeros(2, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError):
        ops.token_logprobs(torch.zeros(2, 1001, dtype=torch.bfloat16, device=DEV), t, 1)   # vocab % 8 != 0
    with pytest.raises(RuntimeError):  # a vocabulary that is no multiple of 8, in rows that are aligned
        ops.token_logprobs(torch.zeros(2, 1008, dtype=torch.bfloat16, device=DEV)[:, :1001], t, 1)
    with pytest.raises(RuntimeError):
        ops.token_logprobs(torch.zeros(2, 1000, dtype=torch.bfloat16, device=DEV), t, 21)  # top_n > 20
