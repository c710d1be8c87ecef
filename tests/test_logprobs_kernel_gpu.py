"""ops.token_logprobs (token_logprobs_kernel, csrc/kernels/sampling.hip) against ref.token_logprobs on the same
bf16 logits: ids and ranks exactly, logprobs within 1e-4 absolute.

The bound is derived, not tuned: torch's own fp32 log_softmax is within 6.5e-6 of float64 at 32 x 128,256;
z - max - lse rounds at 40 * 2^-24 ~ 2.4e-6; a tree sum of 2^17 fast-exp terms adds about 1e-5; 1e-4 leaves a
10x margin."""

import functools
import math

import pytest
import torch

from src import ops
from src.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
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


def check(got, want, n: int):
    lp, rank, top_lp, top_id = (g.cpu() for g in got)
    wlp, wrank, wtop_lp, wtop_id = want
    assert torch.equal(rank, wrank)
    assert torch.equal(top_id, wtop_id[:, :n])
    err = 0.0
    for a, b in ((lp, wlp), (top_lp, wtop_lp[:, :n])):
        fin = torch.isfinite(b)
        assert torch.equal(a[~fin], b[~fin])  # -inf exactly
        if fin.any():
            err = max(err, (a[fin] - b[fin]).abs().max().item())
    assert err <= TOL, err
    return err


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
        check(got, want, n)
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
        assert (lp + math.log(vocab)).abs().max() <= TOL
        assert n == 0 or (top_lp + math.log(vocab)).abs().max() <= TOL


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
            check(got, want, n)
            assert got[0][0].item() == -math.inf
            assert n == 0 or (0 <= int(got[3].min()) and int(got[3].max()) < vocab)


def test_fewer_finite_entries_than_asked():
    """3 finite entries, 20 asked: the -inf ties fill the list in id order, logprob -inf."""
    vocab = 1000
    x = torch.full((1, vocab), -math.inf, dtype=torch.bfloat16)
    x[0, [900, 17, 450]] = torch.tensor([2.0, 1.0, 2.0], dtype=torch.bfloat16)
    t = torch.tensor([17])
    check(ops.token_logprobs(x.to(DEV), t.to(DEV), 20), ref.token_logprobs(x, t, 20), 20)


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
        check(ops.token_logprobs(x.to(DEV), t.to(DEV), n), want, n)


def test_signed_zeros_tie():
    """-0.0 == +0.0 in a float compare and in the reference's sort: they tie, and the lower id goes first."""
    vocab = 1000
    x = torch.full((1, vocab), -1.0, dtype=torch.bfloat16)
    x[0, 10], x[0, 20], x[0, 30] = -0.0, 0.0, -0.0
    t = torch.tensor([30])
    want = ref.token_logprobs(x, t, 5)
    assert want[3][0, :3].tolist() == [10, 20, 30] and want[1][0] == 2
    check(ops.token_logprobs(x.to(DEV), t.to(DEV), 5), want, 5)


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
    check(got, want, 5)
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
