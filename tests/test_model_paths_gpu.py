"""Every dense forward path of the model, and the runner's decode step, against the float64 oracle of
tests/model_reference.py.

Each case runs a script (sequences, how they are cut into steps) on one chain of launches of ``CausalLM.forward``
in a sentinel-filled KV pool with scattered block tables, and compares every tap — the final-norm hidden rows, the
residual stream after the last layer, the logits, K and V of every token, layer and kv head — row by row with the
oracle. The tolerance of a case and tap is ``MARGIN`` (2) x the worst row of the bf16 reference path on the same
case, computed here on the CPU. Every slot the script did not write must still hold the sentinel bit for bit, and
the ``src.ops`` entry points are wrapped with counters: a case that falls back to another path fails.

Measured worst GPU row over bf16-reference worst row, per path, is printed by every case (``-s``) and recorded in
tests/README.md.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402
from tests import model_reference as mr  # noqa: E402

CASES = mr.cases()
TINY = [n for n, c in CASES.items() if c.arch == "tiny" and c.world == 1]   # the groups: test_model_paths_tp_moe_gpu.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available()
    return torch.device("cuda:0")


_models = {}


def gpu_model(fold: bool, tiled: bool):
    """llama-tiny on the family's weights, one per variant, with its decode scratch for every row bucket: the fused
    cases all run on the same scratch, one after the other."""
    key = (fold, tiled)
    if key not in _models:
        m = mr.family_model("tiny", "cuda:0", torch.bfloat16, fold)
        m.tiled_decode_weights = tiled
        scratch = m.alloc_decode_scratch(ops.DECODE_GEMM_MAX_M) if fold else None
        if fold:
            assert scratch is not None and sorted(scratch["plans"]) == [32, 64, 128]
            assert bool(m.layers[0].tiled) == tiled
        _models[key] = (m, scratch)
    return _models[key]


def judge(name, taps, tol=None):
    """Print every tap's worst row next to its tolerance, then assert them, the untouched slots and the path."""
    c = CASES[name]
    L = mr.arch_of(c.arch).num_layers
    tol = tol or mr.case_tolerance(c)
    margin = c.opts.get("margin", mr.MARGIN)
    errs = mr.row_errors(taps, mr.oracle_taps(c.arch, c.script), L)
    bad = []
    for tap, e in errs.items():
        worst = float(e.max())
        print(f"{name:28s} {c.path:14s} {tap:7s} worst row {worst:.4f}  tol {tol[tap]:.4f}  "
              f"= {worst / (tol[tap] / margin):.2f} x the bf16 reference's worst row")
        if not worst <= tol[tap]:
            bad.append((tap, worst, tol[tap], int((e > tol[tap]).sum()), int(e.numel())))
    assert not bad, (name, bad)
    assert mr.untouched(taps), name
    for i, (st, counts) in enumerate(zip(c.script.steps, taps.counts)):
        want = mr.expected_counts(mr.step_path(c, st), L)
        got = {n: counts.get(n, 0) for n in mr.COUNTED}
        assert got == want, (name, i, mr.step_path(c, st), {n: (got[n], want[n]) for n in got if got[n] != want[n]})


@pytest.mark.parametrize("name", TINY)
def test_path_matches_the_oracle(dev, name):
    c = CASES[name]
    fused = c.path.startswith("fused")
    m, scratch = gpu_model(c.fold, c.opts.get("tiled", True))
    assert m.norms_folded == c.fold
    m.prefill_gemm_residual = c.opts.get("gemm_residual", True)
    try:
        taps = mr.run_paged(m, c.script, scratch=scratch if fused else None,
                            pre_embedded=c.opts.get("entry") == "pre")
        torch.cuda.synchronize()
    finally:
        m.prefill_gemm_residual = True
    judge(name, taps)


def test_fused_decode_on_llama_mini_with_p13_on_and_off(dev, monkeypatch):
    """llama-mini at two layers, gate/up on the tile with a 13-bit kernel: packed and tile-order weights give every
    tap bit for bit the same, and both are within tolerance of the oracle."""
    # llama-mini's gate/up (2048 x 1024) on the tile with a P13 kernel
    monkeypatch.setitem(ops.DECODE_TILE_CFG, (2048, 1024, ops.MODE_SILU_NORM, 32), (128, 128, 1))
    runs = {}
    for on in (True, False):
        name = f"fused_mini_p13_{'on' if on else 'off'}"
        c = CASES[name]
        monkeypatch.setenv("DIE_P13", "1" if on else "0")
        m = mr.family_model("mini", "cuda:0", torch.bfloat16)
        scratch = m.alloc_decode_scratch(32)
        assert scratch is not None and tuple(m.decode_plan(32)["gate_up"]) == ops.P13_TILE
        if on:
            assert m.p13_stats["packed"] >= 1, m.p13_stats
        else:
            assert m.p13_stats == {"packed": 0, "raw": 0}
        runs[on] = mr.run_paged(m, c.script, scratch=scratch)
        torch.cuda.synchronize()
        judge(name, runs[on])
        del m, scratch
    torch.cuda.empty_cache()
    for tap in ("hidden", "resid", "logits"):
        for a, b in zip(getattr(runs[True], tap), getattr(runs[False], tap)):
            assert torch.equal(a, b), tap
    assert torch.equal(runs[True].pool, runs[False].pool)


# ------------------------------------------------------------------------------------------ the runner's decode step
@pytest.fixture(scope="module")
def engine(dev):
    model = mr.family_model("tiny", "cuda:0", torch.bfloat16)
    cfg = EngineConfig(max_num_seqs=8, max_num_batched_tokens=512, max_latency_ms=0.0, num_kv_blocks=96,
                       graph_batch_sizes=[1, 2, 4, 8], enable_prefix_caching=False)
    eng = LLMEngine(model, cfg, max_model_len=128)
    eng.eos_token_id = None
    eng.runner.capture_graphs()
    assert eng.runner.graph_sizes == [1, 2, 4, 8] and eng.runner.dec_scratch is not None
    yield eng
    del eng
    torch.cuda.empty_cache()


def _requests(eng, prompts, tag):
    """Queue the prompts (greedy, RUNNER_TOKENS each); returns (outputs, block tables), filled as the engine runs."""
    outs, tables = {}, {}

    def on_token(i):
        def cb(seq, tok):
            if len(seq.block_table) >= len(tables.get(i, [])):
                tables[i] = list(seq.block_table)
        return cb

    def on_finish(i):
        def cb(seq):
            outs[i] = list(seq.output_ids)
        return cb

    for i, p in enumerate(prompts):
        eng.add_request(f"{tag}-{i}", p, SamplingParams(max_tokens=mr.RUNNER_TOKENS, temperature=0.0),
                        on_finish=on_finish(i), on_token=on_token(i))
    return outs, tables


@pytest.mark.parametrize("n", sorted(mr.RUNNER_PROMPTS))
def test_engine_decode_windows_match_the_oracle(engine, n):
    """3 and 7 prompts (graph pads 4 and 8) through captured decode windows: emitted tokens, K / V through every
    sequence's block table, and the blocks nobody owns."""
    eng = engine
    prompts = mr.runner_prompts(n)
    torch.cuda.synchronize()
    eng.pool.tensor.fill_(mr.SENTINEL)
    windows = eng.stats.get("decode_windows", 0)
    outs, tables = _requests(eng, prompts, f"gen{n}")
    while eng.has_work():
        eng.step()
    torch.cuda.synchronize()
    assert eng.stats.get("decode_windows", 0) > windows
    outs = [outs[i] for i in range(n)]
    assert [len(o) for o in outs] == [mr.RUNNER_TOKENS] * n
    # the oracle teacher-forced on the emitted tokens; tolerance from the bf16 reference path on the same script
    script = mr.emitted_script(prompts, outs)
    L = mr.arch_of("tiny").num_layers
    tol = mr.tolerance("tiny", script)
    steps = mr.decided_steps(script, tol["logits"])
    under = sum(int((~ok).sum()) for _, ok in steps)
    print(f"{n} prompts: {under} of {n * mr.RUNNER_TOKENS} steps under the judged gap")
    assert under <= 0.10 * n * mr.RUNNER_TOKENS
    for k, (arg, ok) in enumerate(steps):
        for i in range(n):
            assert outs[i][k] == int(arg[i]) or not bool(ok[i]), (k, i, outs[i], int(arg[i]))
    cpu_pool = eng.pool.tensor.cpu()
    got = mr.Taps([], [], [], {name: mr.read_kv(cpu_pool, tables[i], len(toks))
                               for i, (name, toks) in enumerate(script.seqs.items())})
    kv_taps = [f"kv{li}" for li in range(L)]
    for tap, e in mr.row_errors(got, mr.oracle_taps("tiny", script), L, kv_taps).items():
        print(f"runner, {n} prompts      {tap:7s} worst row {float(e.max()):.4f}  tol {tol[tap]:.4f}")
        assert float(e.max()) <= tol[tap], (tap, float(e.max()), tol[tap])
    owned = torch.zeros(cpu_pool.shape[2], dtype=torch.bool)
    owned[torch.tensor(sorted({b for t in tables.values() for b in t}))] = True
    sent = torch.full((), mr.SENTINEL, dtype=cpu_pool.dtype).view(torch.int16)
    assert bool((cpu_pool[:, :, ~owned].view(torch.int16) == sent).all())


def test_graph_replay_equals_the_eager_decode_step(engine):
    """One decode step of 3 sequences padded to 4: the captured graph's logits for the real rows equal the eager
    ``_decode_forward`` on the same inputs, bit for bit."""
    eng, r = engine, engine.runner
    outs, _ = _requests(eng, mr.runner_prompts(3), "replay")
    for _ in range(4):
        seqs = list(eng.scheduler.running)
        if len(seqs) == 3 and all(len(s.output_ids) >= 1 for s in seqs):
            break
        eng.step()
    assert len(seqs) == 3 and r.inflight is None and not outs
    for s in seqs:
        assert eng.blocks.ensure_slots(s, len(s))
    n, pad = 3, r._pad_for(3)
    assert pad == 4 and pad in r.graphs
    t_graph = r.decode(seqs)
    torch.cuda.synchronize()
    lg_graph = r.graph_logits[pad][:n].clone()
    r._exec_decode = lambda n_, pad_, mode=0: r._decode_forward(pad_)   # the same step, launched eagerly
    try:
        t_eager = r.decode(seqs)
        torch.cuda.synchronize()
        lg_eager = r._last_logits[:n].clone()
    finally:
        del r._exec_decode
    assert lg_graph.shape == lg_eager.shape and bool(lg_graph.abs().sum() > 0)
    assert torch.equal(lg_graph, lg_eager)
    assert t_graph == t_eager
