"""ops.pool_embed (csrc/kernels/pooling.hip) on the MI355X against the float64 oracle of
tests/pool_embed_reference.py, within the tolerance derived there. Inputs are NaN outside the segments (a row the
kernel must not read poisons the result), outputs and accumulators start as sentinels (what the kernel must not
write stays visible). Every comparison prints its measured error next to the tolerance
(profiles/pool_embed_kernel_error.txt holds a run's lines)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from tests import pool_embed_reference as R  # noqa: E402

SENT = -12345.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available()
    return torch.device("cuda:0")


def poisoned(rows_list, dev, stride=None, gap=3):
    """The segments' rows laid out in one [T, H] tensor (row stride `stride`) with `gap` NaN rows before, between
    and after them -> (hidden view, first row of each segment)."""
    h = rows_list[0].shape[1]
    t = sum(r.shape[0] for r in rows_list) + gap * (len(rows_list) + 1)
    buf = torch.full((t, stride or h), float("nan"), dtype=torch.bfloat16)
    firsts, at = [], gap
    for r in rows_list:
        buf[at:at + r.shape[0], :h] = r
        firsts.append(at)
        at += r.shape[0] + gap
    return buf.to(dev)[:, :h], firsts


def segs_tensor(rows, dev):
    return torch.tensor(rows, dtype=torch.int32, device=dev)


def split_scratch(parts, h, n_segs, dev):
    """(part, tickets) for `parts` partial rows: the partials start as NaN (a partial read before it was written
    shows), one spare row behind them as a sentinel, the tickets zero."""
    part = torch.full((parts + 1, h), float("nan"), device=dev)
    part[parts] = SENT
    return part, torch.zeros(n_segs, dtype=torch.int32, device=dev)


def check(name, got, x, mode, dims, normalize):
    want = R.oracle(x, mode, dims, normalize)
    tol = R.tolerance(x, mode, dims, normalize)
    err = np.abs(got.double().cpu().numpy() - want)
    ratio = float((err / np.maximum(tol, 1e-300)).max()) if tol.max() > 0 else float(err.max())
    print(f"{name} normalize={normalize}: max |err| {err.max():.3e}, max tol {tol.max():.3e}, err/tol {ratio:.3f}")
    assert not np.isnan(err).any() and (err <= tol).all(), (name, normalize, float(err.max()), float(tol.max()))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_single_segment_cases(dev, name):
    h, n, mode, dims, family = R.CASES[name]
    x = R.case_rows(name)
    hidden, (first,) = poisoned([x], dev)
    d = dims or h
    parts = ops.pool_parts(n) if mode == "mean" else 1
    assert parts == -(-n // R.PART_ROWS) or mode == "last"
    for normalize in (True, False):
        acc = torch.full((2, h), SENT, device=dev)
        out = torch.full((1, h), SENT, device=dev)
        scratch = split_scratch(parts, h, 1, dev)
        segs = segs_tensor([ops.pool_segment(first, n, 1, n, mean=mode == "mean", parts=parts)], dev)
        ops.pool_embed(hidden, segs, acc, out, dims=dims, normalize=normalize, scratch=scratch, max_parts=parts)
        again = torch.full((1, h), SENT, device=dev)
        ops.pool_embed(hidden, segs, acc, again, dims=dims, normalize=normalize, scratch=scratch, max_parts=parts)
        assert torch.equal(out, again)                       # the ticket was re-armed, nothing else left over
        assert int(scratch[1].abs().sum()) == 0 and bool((scratch[0][parts] == SENT).all())
        assert bool((out[0, d:] == SENT).all())              # the columns beyond dims stay
        assert bool((acc == SENT).all())                     # FIRST | FINAL: the accumulator is not touched
        check(name, out[0, :d], x, mode, dims, normalize)
        if family == "int" and not normalize:
            want = torch.from_numpy(R.oracle(x, mode, dims, False).astype(np.float32))
            assert torch.equal(out[0, :d].cpu(), want), name


def test_ragged_segments_of_both_kinds_strided(dev):
    """Seven ragged segments, last and mean, final and not, in one launch on a strided hidden; non-FINAL segments
    leave out alone and store their sum; untouched accumulator slots keep their sentinel."""
    h = 1024
    lens = [5, 1, 33, 17, 2, 64, 9]
    xs = [R.make_rows(h, n, "rand", 100 + i) for i, n in enumerate(lens)]
    hidden, firsts = poisoned(xs, dev, stride=h + 64)
    assert hidden.stride(0) == h + 64
    kinds = ["mean", "last", "mean_open", "last", "mean", "mean_open", "mean"]
    rows = []
    for i, (k, f, n) in enumerate(zip(kinds, firsts, lens)):
        if k == "last":
            rows.append(ops.pool_segment(f, n))
        else:
            rows.append(ops.pool_segment(f, n, i, n, mean=True, first_chunk=True, final=k == "mean"))
    acc = torch.full((len(lens) + 1, h), SENT, device=dev)
    out = torch.full((len(lens), h), SENT, device=dev)
    ops.pool_embed(hidden, segs_tensor(rows, dev), acc, out)
    for i, (k, x) in enumerate(zip(kinds, xs)):
        if k == "mean_open":
            assert bool((out[i] == SENT).all())
            s = x.double().sum(0).numpy()
            e = (len(x) - 1) * R.U * x.double().abs().sum(0).numpy() * R.SLACK
            assert (np.abs(acc[i].double().cpu().numpy() - s) <= e).all()
        else:
            assert bool((acc[i] == SENT).all())
            check(f"ragged{i}_{k}", out[i], x, k, 0, True)
    assert bool((acc[len(lens)] == SENT).all())


@pytest.mark.parametrize("h,n", [(8, 17), (1024, 1024), (4096, 1000), (R.H_PASS_PLUS_ONE, 17)])
@pytest.mark.parametrize("normalize", [False, True])
def test_integer_mean_in_three_chunks_is_bit_identical(dev, h, n, normalize):
    x = R.make_rows(h, n, "int", 7)
    assert R.integer_family_exact(x)
    hidden, (first,) = poisoned([x], dev)
    acc = torch.full((3, h), SENT, device=dev)
    one = torch.full((1, h), SENT, device=dev)
    ops.pool_embed(hidden, segs_tensor([ops.pool_segment(first, n, 0, n, mean=True)], dev), acc, one,
                   normalize=normalize)
    cuts = [0, max(1, n // 3), max(2, n - n // 5), n] if n >= 3 else [0, n]
    out = torch.full((len(cuts) - 1, h), SENT, device=dev)
    for k in range(len(cuts) - 1):  # one launch per chunk, as consecutive prefill steps do
        a, b = cuts[k], cuts[k + 1]
        seg = ops.pool_segment(first + a, b - a, 2, n, mean=True, first_chunk=a == 0, final=b == n)
        ops.pool_embed(hidden, segs_tensor([seg], dev), acc, out[k:k + 1], normalize=normalize)
    assert bool((out[:-1] == SENT).all())
    assert torch.equal(out[-1], one[0])
    assert bool((acc[:2] == SENT).all())
    if not normalize:
        assert torch.equal(one[0].cpu(), torch.from_numpy(R.oracle(x, "mean", 0, False).astype(np.float32)))


@pytest.mark.parametrize("h", [8, 4096, R.H_PASS_PLUS_ONE])
@pytest.mark.parametrize("normalize", [False, True])
def test_any_split_of_an_integer_mean_is_bit_identical(dev, h, normalize):
    """The integer family's sums are exact in every order: 1 part, 2, 3 (uneven), 5, more parts than rows (empty
    parts) and the 64 of the cap give the same bits, in one launch of six segments over the same rows with a part
    base each, launched twice (re-armed tickets), and the scratch beyond the parts stays as it was."""
    n = 1000 if h == 4096 else 37
    x = R.make_rows(h, n, "int", 11)
    hidden, (first,) = poisoned([x], dev)
    splits = [1, 2, 3, 5, 64, 40]
    bases, at = [], 2
    for k in splits:
        bases.append(at)
        at += k
    segs = segs_tensor([ops.pool_segment(first, n, i, n, mean=True, part_base=b, parts=k)
                        for i, (k, b) in enumerate(zip(splits, bases))], dev)
    part = torch.full((at + 2, h), SENT, device=dev)
    tickets = torch.zeros(len(splits), dtype=torch.int32, device=dev)
    acc = torch.full((len(splits), h), SENT, device=dev)
    outs = []
    for _ in range(2):
        out = torch.full((len(splits), h), SENT, device=dev)
        ops.pool_embed(hidden, segs, acc, out, normalize=normalize, scratch=(part, tickets), max_parts=64)
        outs.append(out)
        assert int(tickets.abs().sum()) == 0
    assert torch.equal(outs[0], outs[1])
    for i in range(1, len(splits)):
        assert torch.equal(outs[0][i], outs[0][0]), splits[i]
    assert bool((part[:2] == SENT).all()) and bool((part[at:] == SENT).all()) and bool((acc == SENT).all())
    if not normalize:
        assert torch.equal(outs[0][0].cpu(), torch.from_numpy(R.oracle(x, "mean", 0, False).astype(np.float32)))


def test_split_chunks_through_the_accumulator(dev):
    """A 700-row random mean in chunks of 300 (two parts, not FINAL), 390 (two parts) and 10 rows: within the
    tolerance of the whole sum, the open chunks write no output."""
    h, n = 1024, 700
    x = R.make_rows(h, n, "rand", 12)
    hidden, (first,) = poisoned([x], dev)
    acc = torch.full((2, h), SENT, device=dev)
    out = torch.full((3, h), SENT, device=dev)
    scratch = split_scratch(4, h, 1, dev)
    for k, (a, b) in enumerate(((0, 300), (300, 690), (690, 700))):
        parts = ops.pool_parts(b - a)
        seg = ops.pool_segment(first + a, b - a, 1, n, mean=True, first_chunk=a == 0, final=b == n, parts=parts)
        ops.pool_embed(hidden, segs_tensor([seg], dev), acc, out[k:k + 1], scratch=scratch, max_parts=parts)
    assert bool((out[:2] == SENT).all()) and bool((acc[0] == SENT).all())
    check("chunks_300_390_10", out[2], x, "mean", 0, True)


def test_zero_vector_stays_zero(dev):
    h = 1024
    z = torch.zeros(4, h, dtype=torch.bfloat16)
    hidden, (first,) = poisoned([z], dev)
    acc = torch.full((1, h), SENT, device=dev)
    out = torch.full((2, h), SENT, device=dev)
    segs = segs_tensor([ops.pool_segment(first, 4, 0, 4, mean=True), ops.pool_segment(first, 4)], dev)
    ops.pool_embed(hidden, segs, acc, out)
    assert torch.equal(out, torch.zeros(2, h, device=dev))


def test_descriptors_outside_the_tensors_write_nothing(dev):
    h = 256
    x = R.make_rows(h, 6, "rand", 3)
    hidden = x.to(dev)
    acc = torch.full((2, h), SENT, device=dev)
    out = torch.full((6, h), SENT, device=dev)
    bad = [ops.pool_segment(-1, 2), ops.pool_segment(4, 3), ops.pool_segment(0, 0),
           ops.pool_segment(0, 6, 2, 6, mean=True), ops.pool_segment(0, 6, -1, 6, mean=True),
           ops.pool_segment(0, 6, 0, 0, mean=True)]
    ops.pool_embed(hidden, segs_tensor(bad, dev), acc, out)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((acc == SENT).all())
    # parts beyond the grid, beyond the scratch, before it: nothing is written, no ticket is taken
    part = torch.full((4, h), SENT, device=dev)
    tickets = torch.zeros(3, dtype=torch.int32, device=dev)
    bad = [ops.pool_segment(0, 6, 0, 6, mean=True, part_base=0, parts=3),
           ops.pool_segment(0, 6, 0, 6, mean=True, part_base=3, parts=2),
           ops.pool_segment(0, 6, 0, 6, mean=True, part_base=-1, parts=2)]
    ops.pool_embed(hidden, segs_tensor(bad, dev), acc, out[:3], scratch=(part, tickets), max_parts=2)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((acc == SENT).all()) and bool((part == SENT).all())
    assert int(tickets.abs().sum()) == 0


def test_refused_shapes_raise(dev):
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    segs = segs_tensor([ops.pool_segment(0, 4)], dev)
    out = torch.zeros(1, 64, device=dev)
    with pytest.raises(RuntimeError):   # H % 8
        ops.pool_embed(torch.zeros(4, 60, dtype=torch.bfloat16, device=dev), segs, None, torch.zeros(1, 60, device=dev))
    with pytest.raises(RuntimeError):   # a row stride that breaks the 16-byte alignment
        ops.pool_embed(torch.zeros(4, 68, dtype=torch.bfloat16, device=dev)[:, :64], segs, None, out)
    with pytest.raises(RuntimeError):   # a misaligned base
        ops.pool_embed(torch.zeros(4 * 64 + 8, dtype=torch.bfloat16, device=dev)[4:4 + 256].view(4, 64), segs, None, out)
    for dims in (4, 12, 72, -8):
        with pytest.raises(RuntimeError):
            ops.pool_embed(x, segs, None, out, dims=dims)
    with pytest.raises(RuntimeError):   # fp16 rows
        ops.pool_embed(x.to(torch.float16), segs, None, out)
    with pytest.raises(RuntimeError):   # out too small for the segments
        ops.pool_embed(x, segs_tensor([ops.pool_segment(0, 4)] * 2, dev), None, out)
    with pytest.raises(RuntimeError):   # descriptor rows of the wrong width
        ops.pool_embed(x, torch.zeros(1, 5, dtype=torch.int32, device=dev), None, out)
    part, tickets = torch.zeros(4, 64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):   # a split without its scratch
        ops.pool_embed(x, segs, None, out, max_parts=2)
    with pytest.raises(RuntimeError):   # more parts than the cap
        ops.pool_embed(x, segs, None, out, scratch=(part, tickets), max_parts=ops.POOL_MAX_PARTS + 1)
    with pytest.raises(RuntimeError):   # fewer tickets than segments
        ops.pool_embed(x, segs_tensor([ops.pool_segment(0, 4)] * 2, dev), None, torch.zeros(2, 64, device=dev),
                       scratch=(part, tickets), max_parts=2)
    with pytest.raises(RuntimeError):   # partial rows of another width
        ops.pool_embed(x, segs, None, out, scratch=(torch.zeros(4, 32, device=dev), tickets), max_parts=2)
    with pytest.raises(RuntimeError):   # acc of another width
        ops.pool_embed(x, segs, torch.zeros(1, 32, device=dev), out)
    torch.cuda.synchronize()
