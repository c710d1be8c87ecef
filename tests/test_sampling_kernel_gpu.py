"""ops.sample (csrc/kernels/sampling.hip) draw by draw against the float64 oracle of tests/sampling_reference.py,
and ops.decode_advance / ops.sample_advance against its plain-Python model of the decode-step advance.

The rule of every comparison: a draw is *decided* when the oracle's gap between its two best scores exceeds
DELTA = 64 * E32 = 1.024e-4 (E32 = 1.6e-6, the float32 score error of these inputs; see the oracle's docstring).
Decided draws must equal the oracle's token, undecided ones must be one of its two best tokens, EVERY draw must lie
inside its kept set, and at most 2 % of a case's draws may be undecided. The inputs are the oracle module's cases;
tests/test_sampling_reference_cpu.py holds the conditions (margins, undecided share, E32) they meet.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from tests import sampling_reference as sr  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), "HIP extension must be built for GPU tests"
    return torch.device("cuda:0")


def params(dev, temperature, top_k, top_p, seeds, steps):
    n = len(seeds)
    return (torch.full((n,), temperature, device=dev), torch.full((n,), top_k, dtype=torch.int32, device=dev),
            torch.full((n,), top_p, device=dev), torch.as_tensor(np.asarray(seeds), device=dev),
            torch.as_tensor(np.asarray(steps), device=dev))


_TOKENS = {}


def gpu_tokens(dev, name):
    """The kernel's draws of a case: one launch, the case's row n times at row stride 0."""
    if name not in _TOKENS:
        c = sr.case(name)
        logits = c.row.to(dev)[None].expand(c.seeds.size, c.row.numel())
        args = params(dev, c.temperature, c.top_k, c.top_p, c.seeds, c.steps)
        _TOKENS[name] = ops.sample(logits, *args).cpu().numpy()
    return _TOKENS[name]


def check(name, got, pred, seeds, steps):
    assert got.shape == pred.token.shape and got.min() >= 0 and got.max() < pred.mask.size, name
    decided = pred.gap > sr.DELTA
    if pred.mask.any():
        outside = ~pred.mask[got]
    else:
        outside = got != 0  # no finite entry: token 0
    wrong = decided & (got != pred.token)
    stray = ~decided & (got != pred.token) & (got != pred.second)
    share = 1.0 - decided.mean()
    print(f"{name}: {got.size} draws, kept {int(pred.mask.sum())}, undecided {share:.4f}, outside the kept set "
          f"{int(outside.sum())}, decided and wrong {int(wrong.sum())}, undecided and not among the two best "
          f"{int(stray.sum())}")
    for i in np.nonzero(outside | wrong | stray)[0][:8]:
        print(f"  seed {seeds[i]} step {steps[i]}: got {got[i]} (kept: {bool(pred.mask[got[i]])}), oracle "
              f"{pred.token[i]} then {pred.second[i]}, gap {pred.gap[i]:.3g}")
    assert not outside.any(), f"{name}: {int(outside.sum())} draws outside the kept set"
    assert not wrong.any(), f"{name}: {int(wrong.sum())} decided draws differ from the oracle"
    assert not stray.any(), f"{name}: {int(stray.sum())} undecided draws are not among the oracle's two best"
    assert share <= sr.UNDECIDED_CAP


def check_case(dev, name):
    c = sr.case(name)
    check(name, gpu_tokens(dev, name), sr.reference(name), c.seeds, c.steps)


@pytest.mark.parametrize("name", list(sr.GROUPS["topk"]))
def test_topk_boundary(dev, name):
    """Near-flat rows: a kept set one token too large or too small shows in about 512 / k draws; the tie variant
    has four equal logits across the k-th place, all of them drawable and nothing below them."""
    check_case(dev, name)
    if sr.case(name).top_k <= 5:
        kept = set(np.nonzero(sr.reference(name).mask)[0])
        assert set(np.unique(gpu_tokens(dev, name))) == kept, "every kept token is drawn in 512 draws"


@pytest.mark.parametrize("name", list(sr.GROUPS["radix"]))
def test_radix_digits(dev, name):
    """Thresholds whose neighbours differ only below the top 16 key bits, among negative entries (complemented
    keys), and across exponents: what a wrong shift, prefix mask or key mapping of the radix select gets wrong."""
    check_case(dev, name)


@pytest.mark.parametrize("name", list(sr.GROUPS["topp"]))
def test_topp_cut(dev, name):
    """Ladder rows, p midway between two cumulative masses at least 2e-2 apart: no fp32 summation order moves the
    cut, and a cut one level off shows in at least 10 of the 512 draws."""
    check_case(dev, name)


@pytest.mark.parametrize("name", list(sr.GROUPS["combined"]))
def test_topk_with_topp(dev, name):
    """Top-p on the renormalised top-k set (kp_differ: the whole-row cut keeps other levels), the top-k floor
    surviving a looser top-p, top_k = 0 / vocab / above it, top_p = 1 / 0 / 1e-6, and no filter at all."""
    check_case(dev, name)


def test_topk_zero_and_at_least_vocab_draw_alike(dev):
    a, b, z = (gpu_tokens(dev, n) for n in ("k_eq_vocab", "k_gt_vocab", "k_zero"))
    assert np.array_equal(a, z) and np.array_equal(b, z)


def test_degenerate_topp_gives_the_argmax(dev):
    top = int(torch.argmax(sr.case("p_zero").row.float()))
    assert (gpu_tokens(dev, "p_zero") == top).all() and (gpu_tokens(dev, "p_tiny") == top).all()


@pytest.mark.parametrize("name", list(sr.GROUPS["masked"]))
def test_masked_rows(dev, name):
    """top_k = 50 over 3 finite entries: only those are drawn, with the oracle's frequencies (draw by draw); a row
    without a finite entry gives token 0."""
    check_case(dev, name)


def test_extreme_uniforms_do_not_decide_the_draw(dev):
    """Draws in which a token 20 below the maximum has the largest uniform (or the smallest): it must lose, as the
    noise spans 19.45 at most. With a uniform that can round to 1.0 the noise is +inf and such a token wins."""
    c = sr.case("extreme")
    got = gpu_tokens(dev, "extreme")
    special = np.nonzero(sr.row_f32(c.row) == -10.0)[0]
    print("extreme draws:", list(zip(c.seeds.tolist(), got.tolist(), sr.reference("extreme").token.tolist())))
    assert not np.isin(got, special).any(), "a token won on its noise alone"
    check_case(dev, "extreme")


SUBJECTS = [("topk_v128256_k50", 3), ("topp_v128256_t1.0_p0.9", 17), ("gauss_unfiltered", 40)]


@pytest.mark.parametrize("name,i", SUBJECTS)
def test_batch_independence(dev, name, i):
    """The same (row, parameters, seed, step) gives the same token alone, at index 5 of 7 rows, at index 100 of 128
    rows with other rows and parameters around it, and in the split launch (scratch=) among greedy rows."""
    c = sr.case(name)
    vocab = c.row.numel()
    g = torch.Generator(device="cpu").manual_seed(i)
    one = ops.sample(c.row.to(dev)[None], *params(dev, c.temperature, c.top_k, c.top_p, c.seeds[i:i + 1],
                                                  c.steps[i:i + 1])).cpu()
    want = int(one[0])
    pred = sr.reference(name)
    assert pred.mask[want]
    if pred.gap[i] > sr.DELTA:
        assert want == pred.token[i]
    part = torch.zeros(128 * 32, dtype=torch.int32, device=dev)
    cnt = torch.zeros(128, dtype=torch.int32, device=dev)
    for rows, at, scratch in ((7, 5, None), (128, 100, None), (7, 5, (part, cnt)), (128, 100, (part, cnt))):
        logits = (torch.randn(rows, vocab, generator=g) * 3).to(torch.bfloat16)
        logits[at] = c.row
        logits = logits.to(dev)
        temp = torch.rand(rows, generator=g) + 0.5
        topk = torch.randint(0, 60, (rows,), generator=g, dtype=torch.int32)
        topp = torch.rand(rows, generator=g) * 0.5 + 0.5
        seeds = torch.randint(0, 1 << 40, (rows,), generator=g)
        steps = torch.randint(0, 500, (rows,), generator=g)
        if scratch is not None:
            temp[::2] = 0.0  # greedy rows, argmax'ed by several workgroups each
        temp[at], topk[at], topp[at] = c.temperature, c.top_k, c.top_p
        seeds[at], steps[at] = int(c.seeds[i]), int(c.steps[i])
        got = ops.sample(logits, temp.to(dev), topk.to(dev), topp.to(dev), seeds.to(dev), steps.to(dev),
                         scratch=scratch).cpu()
        assert int(got[at]) == want, (rows, at, scratch is not None)
        if scratch is not None:
            greedy = (temp == 0.0) | (topk == 1)
            first_max = torch.as_tensor(np.argmax(logits.float().cpu().numpy(), axis=-1))
            assert torch.equal(got[greedy], first_max[greedy])
            assert int(cnt.abs().sum()) == 0


def test_default_seed_and_step(dev):
    """seeds = None / steps = None draw as seed 0x5eed at step 0, here on the rows of eight cases at once."""
    names = list(sr.GROUPS["radix"]) + ["topk_v32000_k2", "topk_v32000_k5", "topk_v32000_k50", "topk_tie4"]
    cases = [sr.case(n) for n in names]
    logits = torch.stack([c.row for c in cases]).to(dev)
    temp = torch.tensor([c.temperature for c in cases], device=dev)
    topk = torch.tensor([c.top_k for c in cases], dtype=torch.int32, device=dev)
    topp = torch.tensor([c.top_p for c in cases], device=dev)
    got = ops.sample(logits, temp, topk, topp).cpu()
    seeds = torch.full((len(cases),), 0x5eed, dtype=torch.long, device=dev)
    assert torch.equal(got, ops.sample(logits, temp, topk, topp, seeds, torch.zeros_like(seeds)).cpu())
    assert torch.equal(got, ops.sample(logits, temp, topk, topp, seeds, None).cpu())
    for j, c in enumerate(cases):
        pred = sr.predict(c.row, c.temperature, c.top_k, c.top_p, [0x5eed], [0])
        assert pred.mask[int(got[j])], c.name
        assert int(got[j]) == pred.token[0] or (pred.gap[0] <= sr.DELTA and int(got[j]) == pred.second[0]), c.name


# ------------------------------------------------------------------------------------------------------------
# the decode-step advance

BS, WIDTH, K_WIN = 16, 6, 4


def advance_state(rows, n_real, cnt, g):
    """Positions by row % 4: anywhere; on the last slot of a block (the next slot is the first of another block-table
    entry); on the last slot of the last column (the next slot is -1); one before that (-1 after two steps)."""
    r = torch.arange(rows)
    last_of_block = torch.randint(0, WIDTH - 1, (rows,), generator=g) * BS + BS - 1
    pos = torch.randint(0, WIDTH * BS - 2, (rows,), generator=g)
    pos = torch.where(r % 4 == 1, last_of_block, pos)
    pos = torch.where(r % 4 == 2, torch.full_like(pos, WIDTH * BS - 1), pos)
    pos = torch.where(r % 4 == 3, torch.full_like(pos, WIDTH * BS - 2), pos)
    return {"out": torch.randint(0, 512, (rows,), generator=g), "ids": torch.randint(0, 512, (rows,), generator=g),
            "pos": pos, "ctx": (pos + 1).to(torch.int32), "slots": torch.full((rows,), -7, dtype=torch.long),
            "bt": torch.randint(0, 1000, (rows, WIDTH), generator=g, dtype=torch.int32),
            "step": torch.randint(0, 50, (rows,), generator=g),
            "tokens": torch.full((K_WIN + 3, rows), -1, dtype=torch.long),  # the window is its first K_WIN rows
            "cnt": torch.tensor([cnt], dtype=torch.int32), "n_real": torch.tensor([n_real], dtype=torch.int32)}


def window(state):
    s = dict(state)
    s["tokens"] = state["tokens"][:K_WIN]
    return s


def assert_state(got, want, past_window, what):
    for key, w in want.items():
        assert torch.equal(got[key].cpu(), w), (what, key, got[key].cpu()[:12], w[:12])
    assert bool((past_window.cpu() == -1).all()), (what, "a write past the token window")


def n_reals(rows):
    return sorted({rows, max(rows - 3, 0), 0})


@pytest.mark.parametrize("rows", [1, 8, 32, 128, 300])
def test_decode_advance_against_the_model(dev, rows):
    g = torch.Generator(device="cpu").manual_seed(rows)
    for n_real in n_reals(rows):
        for cnt in (0, K_WIN - 1, K_WIN, K_WIN + 2):
            full = advance_state(rows, n_real, cnt, g)
            want = window(full)
            dfull = {k: v.to(dev) for k, v in full.items()}
            d = window(dfull)
            for launch in range(2):
                want = sr.advance_model(want, rows, BS)
                if launch == 1:  # the second step samples other tokens
                    d["out"].copy_(want["out"])
                ops.decode_advance(d["out"], d["ids"], d["pos"], d["ctx"], d["slots"], d["bt"], d["step"], d["tokens"],
                                   d["cnt"], d["n_real"], rows, BS)
                assert_state(d, want, dfull["tokens"][K_WIN:], (rows, n_real, cnt, launch))
                want["out"] = (want["out"] * 7 + 3) % 512
            if rows >= 4 and n_real == rows:
                assert int(want["slots"][2]) == -1 and int(want["slots"][3]) == -1
                assert int(want["slots"][1]) % BS == 1 and int((want["slots"][:n_real] >= 0).sum()) > 0


@pytest.mark.parametrize("rows", [1, 8, 32])
def test_sample_advance_against_the_model(dev, rows):
    """Greedy rows from the LM head's candidates (ops.linear_tiled_argmax at n = 512, k = 256): the token is the
    first maximum of the logits, and the buffers advance as the model says; the row ticket is zero after every
    launch."""
    n, k, wr, kc = 512, 256, 64, 128
    g = torch.Generator(device="cpu").manual_seed(100 + rows)
    wt = ops.gd_pack_weights((torch.randn(n, k, generator=g) * 0.05).to(torch.bfloat16).to(dev), wr, kc=kc)
    parts = torch.zeros(rows, n // wr, 2, dtype=torch.int32, device=dev)
    temp, topk, topp, seeds, _ = params(dev, 0.0, 0, 1.0, np.arange(rows), np.zeros(rows, dtype=np.int64))
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    for n_real in n_reals(rows):
        for cnt in (0, K_WIN - 1, K_WIN, K_WIN + 2):
            full = advance_state(rows, n_real, cnt, g)
            want = window(full)
            dfull = {kk: v.to(dev) for kk, v in full.items()}
            d = window(dfull)
            for launch in range(2):
                x = torch.randn(rows, k, generator=g).to(torch.bfloat16).to(dev)
                logits = ops.linear_tiled_argmax(x, wt, wr, kc, parts)
                want["out"] = torch.as_tensor(np.argmax(logits.float().cpu().numpy(), axis=-1))
                want = sr.advance_model(want, rows, BS)
                ops.sample_advance(logits, temp, topk, topp, seeds, d["step"], d["out"], parts, d["ids"], d["pos"],
                                   d["ctx"], d["slots"], d["bt"], d["tokens"], d["cnt"], d["n_real"], BS, ticket)
                assert_state(d, want, dfull["tokens"][K_WIN:], (rows, n_real, cnt, launch))
                assert int(ticket.item()) == 0
