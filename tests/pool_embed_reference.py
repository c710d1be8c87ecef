"""Float64 oracle of ops.pool_embed (csrc/kernels/pooling.hip), its input families and the tolerance a float32
implementation is allowed against it. Not a test: tests/test_pool_embed_reference_cpu.py judges this file,
tests/test_pool_embed_kernel_gpu.py judges the kernel by it.

Contract. For one request whose prompt rows are x[0..L) (bf16, exact in fp32 and float64), H columns:

    last:  v = x[L - 1]
    mean:  v = (sum_i x[i]) / L        the kernel sums in fp32, in chunks through an fp32 accumulator, in any order
    v  <- v[:D]                        D = dims or H
    out = v / max(||v||_2, 1e-12)      with normalize (torch.nn.functional.normalize), else v

Tolerance (per component j, absolute), u = 2^-24 the unit roundoff of fp32. Every step is bounded to first order and
the sum is widened by SLACK for the second-order terms ((L + D) u < 1e-3 at every shape used here).

  sum       any order of adding L numbers performs L - 1 additions and no number passes through more than L - 1 of
            them, so |s^_j - s_j| <= g * A_j with g = (L - 1) u / (1 - (L - 1) u) and A_j = sum_i |x_ij|
            (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: the bound holds for every ordering);
  division  v^_j = fl(s^_j / L): |v^_j - v_j| <= e_j := g A_j / L + u |v_j|   (last pooling: e_j = 0, a copy);
  without normalize that is the tolerance. With it, N = ||v||_2 and t_j = v_j / N the true output:
  squares   ss^ = fl(sum_j v^_j^2), D products and D - 1 additions of non-negative terms in any order (a fused
            multiply-add only removes a rounding): relative error <= (D + 1) u; the square root halves it and
            rounds once more; the quotient rounds once: the factor 1 / N^ carries a relative error
            r = ((D + 1) / 2 + 2) u;
  direction ||v^|| differs from N by at most ||e||_2, so |v^_j / ||v^|| - t_j| <= e_j / N + |t_j| ||e||_2 / N;

            tol_j = SLACK * (e_j / N + |t_j| * (||e||_2 / N + r))

  A zero vector (N = 0, only reached with e = 0: all rows zero, or last pooling of a zero row) must come back as
  exact zeros: 0 / 1e-12.

Integer family: every entry an integer with |x| <= 64 and L <= 1024. Then every partial sum of every column is an
integer below 2^24 in magnitude, so every fp32 addition is exact in every order: the kernel's sum IS the true sum,
a mean taken in chunks equals the mean taken at once bit for bit, and without normalize the output is the
correctly rounded quotient — which float64 division followed by rounding to float32 also gives (53 >= 2 * 24 + 2:
double rounding is innocuous for division)."""

import numpy as np
import torch

U = 2.0 ** -24
SLACK = 1.0 + 1e-3
INT_MAX_ABS = 64
INT_MAX_ROWS = 1024

PART_ROWS = 256              # ops.POOL_PART_ROWS: a mean segment of more rows is split over several workgroups
POOL_THREADS = 1024          # the kernel's workgroup: one 16-byte column group per thread and pass
H_ONE_VECTOR = 8
H_PASS_PLUS_ONE = 8 * (POOL_THREADS + 1)


def oracle(rows: torch.Tensor, mode: str, dims: int = 0, normalize: bool = True, total: int = 0) -> np.ndarray:
    """float64 [D] from the request's rows [L, H] (any float dtype; bf16 values are exact in float64).
    total: the divisor of the mean (default: L)."""
    x = rows.to(torch.float64).numpy()
    d = dims if dims else x.shape[1]
    if mode == "last":
        v = x[-1, :d].copy()
    elif mode == "mean":
        v = x[:, :d].sum(0) / float(total or x.shape[0])
    else:
        raise ValueError(mode)
    if normalize:
        v = v / max(float(np.sqrt((v * v).sum())), 1e-12)
    return v


def tolerance(rows: torch.Tensor, mode: str, dims: int = 0, normalize: bool = True) -> np.ndarray:
    """float64 [D]: the absolute error per component a float32 implementation of the contract may show."""
    x = rows.to(torch.float64).numpy()
    n, h = x.shape
    d = dims if dims else h
    x = x[:, :d]
    if mode == "last":
        v, e = x[-1], np.zeros(d)
    else:
        g = (n - 1) * U / (1.0 - (n - 1) * U)
        v = x.sum(0) / n
        e = g * np.abs(x).sum(0) / n + U * np.abs(v)
    if not normalize:
        return SLACK * e
    norm = float(np.sqrt((v * v).sum()))
    if norm == 0.0:
        return np.zeros(d)
    t = v / norm
    r = ((d + 1) / 2.0 + 2.0) * U
    return SLACK * (e / norm + np.abs(t) * (float(np.sqrt((e * e).sum())) / norm + r))


def make_rows(h: int, n: int, family: str, seed: int) -> torch.Tensor:
    """bf16 [n, h]. "rand": normal(0, 1) with a per-column offset (so that a mean does not cancel to nothing);
    "int": integers in [-INT_MAX_ABS, INT_MAX_ABS]."""
    g = torch.Generator().manual_seed(seed)
    if family == "int":
        assert n <= INT_MAX_ROWS
        return torch.randint(-INT_MAX_ABS, INT_MAX_ABS + 1, (n, h), generator=g).to(torch.bfloat16)
    assert family == "rand"
    off = torch.randn(1, h, generator=g) * 0.5
    return (torch.randn(n, h, generator=g) + off).to(torch.bfloat16)


def integer_family_exact(rows: torch.Tensor) -> bool:
    """The exactness condition of the integer family: integer entries and every column's sum of magnitudes below
    2^24 (then every partial sum in every order is an exactly representable integer)."""
    x = rows.to(torch.float64)
    return bool((x == x.round()).all()) and float(x.abs().sum(0).max()) < 2.0 ** 24 and \
        float(x.abs().max()) <= INT_MAX_ABS and x.shape[0] <= INT_MAX_ROWS


def _cases() -> dict:
    """name -> (H, rows, mode, dims, family): the single-segment cases of the GPU kernel test. H: one vector, one
    vector more than a whole pass of the workgroup, 1024, 4096, 8192; rows 1, 2, 17; the row counts around which a
    lane's unrolled row loop (8 loads per row group) takes a second trip: 2 groups at H = 4096 (16 rows: 17 above),
    8 groups at H = 1024 (64 | 65), 16 groups at H = 8 (128 | 129); and each side of the row split (PART_ROWS rows
    per workgroup: 256 | 257 rows are one | two parts, 600 three, 1000 and 1024 four)."""
    c = {}
    for h in (H_ONE_VECTOR, H_PASS_PLUS_ONE, 1024, 4096, 8192):
        for n in (1, 2, 17):
            for mode in ("last", "mean"):
                c[f"h{h}_r{n}_{mode}"] = (h, n, mode, 0, "rand")
    for h, n in ((1024, 64), (1024, 65), (8, 128), (8, 129), (4096, 16), (4096, PART_ROWS), (4096, PART_ROWS + 1),
                 (8, PART_ROWS + 1), (H_PASS_PLUS_ONE, PART_ROWS + 1), (1024, 600)):
        c[f"h{h}_r{n}_mean"] = (h, n, "mean", 0, "rand")
    c[f"h4096_r{PART_ROWS + 1}_last"] = (4096, PART_ROWS + 1, "last", 0, "rand")
    c[f"h1024_r{PART_ROWS + 1}_mean_d8"] = (1024, PART_ROWS + 1, "mean", 8, "rand")
    for h in (1024, 8192, H_PASS_PLUS_ONE):
        for dims in (8, h - 8):
            c[f"h{h}_r17_mean_d{dims}"] = (h, 17, "mean", dims, "rand")
            c[f"h{h}_r17_last_d{dims}"] = (h, 17, "last", dims, "rand")
    for h, n in ((8, 17), (1024, 1024), (4096, 1000), (H_PASS_PLUS_ONE, 17), (4096, PART_ROWS + 1)):
        c[f"h{h}_r{n}_mean_int"] = (h, n, "mean", 0, "int")
    c["h4096_r17_last_int"] = (4096, 17, "last", 0, "int")
    c["h4096_r1000_mean"] = (4096, 1000, "mean", 0, "rand")
    return c


CASES = _cases()


def case_rows(name: str) -> torch.Tensor:
    h, n, _, _, family = CASES[name]
    return make_rows(h, n, family, seed=sum(map(ord, name)))
