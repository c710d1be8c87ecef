"""tests/pool_embed_reference.py judged before the kernel is judged by it: the oracle is the torch expression, and on
every GPU case its tolerance is small against what a wrong row set would change."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from src import ops
from tests import pool_embed_reference as R


def test_oracle_is_the_torch_expression():
    for h, n, seed in ((256, 1, 1), (256, 37, 2), (1024, 300, 3)):
        x = R.make_rows(h, n, "rand", seed)
        mean = F.normalize(x.float().mean(0), dim=0).double().numpy()
        last = F.normalize(x[-1].float(), dim=0).double().numpy()
        assert np.abs(R.oracle(x, "mean") - mean).max() <= R.tolerance(x, "mean").max()
        assert np.abs(R.oracle(x, "last") - last).max() <= R.tolerance(x, "last").max()
        # unnormalised and truncated forms
        assert np.array_equal(R.oracle(x, "last", normalize=False), x[-1].double().numpy())
        assert np.allclose(R.oracle(x, "mean", dims=8, normalize=False), x[:, :8].double().mean(0).numpy(), rtol=1e-13)
        assert np.allclose(R.oracle(x, "mean", dims=8), F.normalize(x[:, :8].double().mean(0), dim=0).numpy(),
                           rtol=1e-12)
    z = torch.zeros(5, 16, dtype=torch.bfloat16)
    for mode in ("last", "mean"):
        assert np.array_equal(R.oracle(z, mode), np.zeros(16)) and np.array_equal(R.tolerance(z, mode), np.zeros(16))
        assert np.array_equal(F.normalize(z.float().mean(0), dim=0).numpy(), np.zeros(16, dtype=np.float32))


def test_cpu_op_follows_the_oracle():
    """The torch path of ops.pool_embed (what the CPU engine tests run) within the float32 tolerance, chunks
    through the accumulator included."""
    x = R.make_rows(256, 41, "rand", 5)
    pad = torch.full((3, 256), float("nan"), dtype=torch.bfloat16)
    hidden = torch.cat([pad, x, pad])
    acc = torch.full((2, 256), 7.0)
    segs = torch.tensor([ops.pool_segment(3, 41, 1, 41, mean=True), ops.pool_segment(3, 41)], dtype=torch.int32)
    out = ops.pool_embed(hidden, segs, acc)
    assert np.abs(out[0].double().numpy() - R.oracle(x, "mean")).max() <= R.tolerance(x, "mean").max()
    assert (np.abs(out[1].double().numpy() - R.oracle(x, "last")) <= R.tolerance(x, "last")).all()
    assert torch.equal(acc, torch.full((2, 256), 7.0))  # a FIRST | FINAL segment neither reads nor writes it
    out3 = torch.full((3, 256), -5.0)
    for k, (a, b) in enumerate(((0, 10), (10, 30), (30, 41))):
        segs = torch.tensor([ops.pool_segment(3 + a, b - a, 0, 41, True, a == 0, b == 41)], dtype=torch.int32)
        ops.pool_embed(hidden, segs, acc, out3[k:k + 1])
    assert torch.equal(out3[:2], torch.full((2, 256), -5.0))  # non-FINAL chunks write no output
    assert np.abs(out3[2].double().numpy() - R.oracle(x, "mean")).max() <= R.tolerance(x, "mean").max()
    assert torch.equal(acc[1], torch.full((256,), 7.0))
    with pytest.raises(RuntimeError):
        ops.pool_embed(hidden, segs, acc, dims=12)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_tolerance_separates_wrong_row_sets(name):
    """Leaving out any single row of a mean (same divisor), or taking the row before the last, moves the oracle by
    at least 4 tolerances: a kernel that reads a wrong set of rows cannot pass."""
    h, n, mode, dims, family = R.CASES[name]
    x = R.case_rows(name)
    assert x.shape == (n, h) and x.dtype == torch.bfloat16
    if family == "int":
        assert R.integer_family_exact(x)
    for normalize in (True, False):
        want = R.oracle(x, mode, dims, normalize)
        tol = R.tolerance(x, mode, dims, normalize).max()
        assert want.shape == ((dims or h),) and np.isfinite(want).all() and np.abs(want).max() > 0
        if mode == "last":
            if n > 1:
                wrong = R.oracle(x[:-1], "last", dims, normalize)
                assert np.abs(wrong - want).max() >= 4 * tol, (name, normalize)
            continue
        d = dims or h
        xs = x.double().numpy()[:, :d]
        wrong = (xs.sum(0)[None, :] - xs) / n  # row i left out, the divisor kept
        if normalize:
            wrong = wrong / np.maximum(np.sqrt((wrong * wrong).sum(1, keepdims=True)), 1e-12)
        moved = np.abs(wrong - want[None, :]).max(1)
        assert moved.min() >= 4 * tol, (name, normalize, float(moved.min()), float(tol))


def test_integer_family_is_exact_in_float32():
    """Every order of float32 additions gives the true column sums, and the float32 quotient is the correctly
    rounded one."""
    x = R.make_rows(64, R.INT_MAX_ROWS, "int", 9)
    assert R.integer_family_exact(x)
    true = x.double().sum(0)
    f = x.float()
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(1))
    seq = torch.zeros(64)
    for i in perm.tolist():
        seq = seq + f[i]
    assert torch.equal(seq.double(), true) and torch.equal(f.sum(0).double(), true)
    q32 = seq / torch.tensor(float(x.shape[0]))
    assert np.array_equal(q32.numpy(), R.oracle(x, "mean", normalize=False).astype(np.float32))
    assert not R.integer_family_exact(R.make_rows(8, 4, "rand", 0))
