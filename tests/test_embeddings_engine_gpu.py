"""Embedding requests through the engine on the MI355X (llama-mini on the HIP kernels, decode hipGraphs on).

Where the engine's step and an uncached forward run the same kernels on the same shapes (every prompt whole, in
one step) the comparison is exact: last pooling bit for bit, mean pooling within the float32 tolerance of
tests/pool_embed_reference.py against the float64 oracle of those hidden rows. Where chunking or a cached prefix
changes the route by which the last block's KV was computed (other GEMM shapes: a bf16 ulp here and there) the
vectors are compared with the fp32 CPU twin of the model instead, within the relative error tests/test_oracle_gpu.py
allows against that twin (0.03); the measured value is printed."""

import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.models.llama import AttnMetadata  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402
from tests import pool_embed_reference as R  # noqa: E402

TWIN_REL = 0.03


def make(tokens=2048, prefix=True) -> LLMEngine:
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available()
    cfg = EngineConfig(max_num_seqs=8, max_num_batched_tokens=tokens, num_kv_blocks=512, max_latency_ms=0.0,
                       graph_batch_sizes=[1, 2, 4, 8], decode_window=4, use_cuda_graph=True,
                       enable_prefix_caching=prefix, preemption_mode="recompute")
    eng = LLMEngine.from_preset("llama-mini", device="cuda:0", cfg=cfg, max_model_len=1024)
    eng.eos_token_id = None
    assert eng.runner.graphs
    return eng


@pytest.fixture(scope="module")
def engine():
    return make()


@pytest.fixture(scope="module")
def small():
    """The same model (same seed, same weights) with steps of at most 64 tokens: prompts are chunked."""
    return make(tokens=64)


@pytest.fixture(scope="module")
def twin(engine):
    return engine.model.reference_copy("cpu", torch.float32)


@torch.inference_mode()
def uncached_forward(model, ps, keep=None):
    """One ragged prefill forward of the prompts over a pool of its own -> hidden (every row, or the kept rows)."""
    dev = model.device
    lens = [len(p) for p in ps]
    nbps = -(-max(lens) // 16)
    n = len(ps)
    pool = torch.zeros(model.arch.num_layers, 2, n * nbps, model.hkv, 16, model.head_dim, dtype=model.dtype, device=dev)
    bt = torch.arange(n * nbps, dtype=torch.int32).view(n, nbps)
    ids = torch.tensor([t for p in ps for t in p], device=dev)
    pos = torch.cat([torch.arange(L) for L in lens])
    seq_of = torch.cat([torch.full((L,), i) for i, L in enumerate(lens)])
    slots = (bt[seq_of, pos // 16].long() * 16 + pos % 16).to(dev)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    meta = AttnMetadata(True, slots, bt.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), cu.to(dev),
                        max(lens), keep_rows=keep)
    return model.forward(ids, pos.to(dev), meta, pool), cu


def prompts(n, lo=20, hi=200, seed=0):
    rng = random.Random(seed)
    return [[rng.randrange(3, 30000) for _ in range(rng.randrange(lo, hi))] for _ in range(n)]


def run(eng, reqs, hook=None):
    done = {}
    for i, (p, sp) in enumerate(reqs):
        eng.add_request(f"emb-{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    steps = 0
    while eng.has_work():
        eng.step()
        steps += 1
        if hook is not None:
            hook(steps)
    return [done[i] for i in range(len(reqs))]


def twin_rel(twin, p, vec, mode):
    rows, _ = uncached_forward(twin, [p])
    want = R.oracle(rows, mode)
    return float(np.linalg.norm(vec.astype(np.float64) - want) / np.linalg.norm(want))


def test_last_whole_prompts_bit_for_bit(engine, twin):
    """One step of whole prompts, last pooling only: the engine keeps the last rows in the last layer, and an
    uncached forward of the same ragged batch with the same kept rows runs the same kernels on the same shapes."""
    ps = prompts(5, seed=1)
    before = engine.get_stats()["pool_embed_launches"]
    seqs = run(engine, [(p, SamplingParams(pooling="last")) for p in ps])
    assert engine.get_stats()["pool_embed_launches"] == before + 1  # one launch for the step's five segments
    lens = torch.tensor([len(p) for p in ps]).cumsum(0)
    keep = (lens - 1).to(engine.device)
    hidden, _ = uncached_forward(engine.model, ps, keep=keep)
    assert hidden.shape[0] == len(ps)
    segs = torch.tensor([ops.pool_segment(i, 1) for i in range(len(ps))], dtype=torch.int32, device=engine.device)
    want = ops.pool_embed(hidden, segs).cpu().numpy()
    for i, (p, s) in enumerate(zip(ps, seqs)):
        assert s.finish_reason == "embed" and s.output_ids == [] and s.embedding.dtype == np.float32
        assert np.array_equal(s.embedding, want[i]), i
        # and the kernel's normalisation of that row is the oracle's, within the float32 tolerance
        row = hidden[i:i + 1].cpu()
        assert (np.abs(s.embedding.astype(np.float64) - R.oracle(row, "last")) <= R.tolerance(row, "last")).all()
        rel = twin_rel(twin, p, s.embedding, "last")
        print(f"last, whole prompt of {len(p)}: rel err vs the fp32 twin {rel:.4f}")
        assert rel < TWIN_REL


def test_mean_whole_prompts_against_the_oracle(engine, twin):
    ps = prompts(5, seed=2)
    sps = [SamplingParams(pooling="mean"), SamplingParams(pooling="mean", embed_dimensions=64),
           SamplingParams(pooling="mean", embed_normalize=False), SamplingParams(pooling="mean"),
           SamplingParams(pooling="mean", embed_dimensions=64)]
    before = engine.get_stats()["pool_embed_launches"]
    seqs = run(engine, list(zip(ps, sps)))
    assert engine.get_stats()["pool_embed_launches"] == before + 3  # one launch per (dimensions, normalize) group
    hidden, cu = uncached_forward(engine.model, ps)
    for i, (p, sp, s) in enumerate(zip(ps, sps, seqs)):
        rows = hidden[int(cu[i]):int(cu[i + 1])].cpu()
        d, nz = sp.embed_dimensions or 0, sp.embed_normalize
        want, tol = R.oracle(rows, "mean", d, nz), R.tolerance(rows, "mean", d, nz)
        err = np.abs(s.embedding.astype(np.float64) - want)
        print(f"mean, whole prompt of {len(p)}, dims {d}, normalize {nz}: max err {err.max():.3e}, tol {tol.max():.3e}")
        assert s.embedding.shape == want.shape and (err <= tol).all()
    rel = twin_rel(twin, ps[0], seqs[0].embedding, "mean")
    print(f"mean, whole prompt: rel err vs the fp32 twin {rel:.4f}")
    assert rel < TWIN_REL
    assert not engine.runner._pool_slots and sorted(engine.runner._pool_free) == list(range(8))


@pytest.mark.parametrize("mode", ["last", "mean"])
def test_chunked_prefill_against_the_twin(small, twin, mode):
    eng = small
    ps = prompts(3, lo=150, hi=300, seed=3)
    s0 = eng.get_stats()
    seqs = run(eng, [(p, SamplingParams(pooling=mode)) for p in ps])
    assert eng.get_stats()["steps_prefill"] - s0["steps_prefill"] > 3
    for p, s in zip(ps, seqs):
        rel = twin_rel(twin, p, s.embedding, mode)
        print(f"{mode}, prompt of {len(p)} in chunks of <= 64: rel err vs the fp32 twin {rel:.4f}")
        assert s.finish_reason == "embed" and rel < TWIN_REL
    assert not eng.runner._pool_slots


def test_last_after_a_prefix_hit_mean_without_one(engine, twin):
    rng = random.Random(4)
    shared = [rng.randrange(3, 30000) for _ in range(96)]
    a, b = shared + [7, 8, 9], shared + [11, 12, 13, 14, 15]
    run(engine, [(a, SamplingParams(max_tokens=2, ignore_eos=True))])
    s_last, = run(engine, [(b, SamplingParams(pooling="last"))])
    assert s_last.num_prefix_hit == 96
    rel = twin_rel(twin, b, s_last.embedding, "last")
    print(f"last after a 96-token prefix hit: rel err vs the fp32 twin {rel:.4f}")
    assert rel < TWIN_REL
    s_mean, = run(engine, [(b, SamplingParams(pooling="mean"))])
    assert s_mean.num_prefix_hit == 0
    rel = twin_rel(twin, b, s_mean.embedding, "mean")
    print(f"mean of the same prompt (no prefix match): rel err vs the fp32 twin {rel:.4f}")
    assert rel < TWIN_REL


def test_shared_steps_and_decode_windows_keep_the_generated_tokens(engine, twin):
    """Generation requests return the same tokens alone, in a prefill step shared with embedding requests, and when
    an embedding request arrives while their decode windows run."""
    ps = prompts(6, seed=5)
    gen = SamplingParams(max_tokens=24, ignore_eos=True)
    alone = [s.output_ids for s in run(engine, [(p, gen) for p in ps[:3]])]
    w0 = engine.get_stats().get("decode_windows", 0)
    reqs = [(ps[0], gen), (ps[3], SamplingParams(pooling="last")), (ps[1], gen), (ps[2], gen),
            (ps[4], SamplingParams(pooling="last"))]
    seqs = run(engine, reqs)
    assert [seqs[i].output_ids for i in (0, 2, 3)] == alone
    for i in (1, 4):
        rel = twin_rel(twin, reqs[i][0], seqs[i].embedding, "last")
        print(f"last, in a step shared with three generation requests: rel err vs the fp32 twin {rel:.4f}")
        assert rel < TWIN_REL
    assert engine.get_stats().get("decode_windows", 0) > w0
    late = []

    def hook(step):
        if step == 2:
            engine.add_request("late-last", ps[5], SamplingParams(pooling="last"), on_finish=late.append)
        if step == 4:
            engine.add_request("late-mean", ps[4], SamplingParams(pooling="mean"), on_finish=late.append)
    seqs = run(engine, [(p, gen) for p in ps[:3]], hook)
    assert [s.output_ids for s in seqs] == alone
    assert [s.finish_reason for s in late] == ["embed", "embed"]
    for s, p, mode in zip(late, (ps[5], ps[4]), ("last", "mean")):
        rel = twin_rel(twin, p, s.embedding, mode)
        print(f"{mode}, arriving between decode windows: rel err vs the fp32 twin {rel:.4f}")
        assert rel < TWIN_REL


@pytest.mark.parametrize("mode", ["last", "mean"])
def test_recompute_preemption(small, twin, mode):
    eng = small
    p = prompts(1, lo=250, hi=251, seed=6)[0]
    hit = []

    def hook(step):
        if step == 2:
            seq = next(iter(eng.seqs.values()))
            assert 0 < seq.num_computed < len(p)
            eng.scheduler._preempt(seq)
            eng._release_logit_state(seq, preempted=True)
            hit.append(seq.num_computed)
    s, = run(eng, [(p, SamplingParams(pooling=mode))], hook)
    assert hit == [0] and s.num_preemptions == 1 and s.finish_reason == "embed"
    rel = twin_rel(twin, p, s.embedding, mode)
    print(f"{mode} after a recompute preemption: rel err vs the fp32 twin {rel:.4f}")
    assert rel < TWIN_REL
    assert not eng.runner._pool_slots and sorted(eng.runner._pool_free) == list(range(8))


def test_nobody_asks_nothing_is_launched_or_allocated():
    eng = make()
    run(eng, [(p, SamplingParams(max_tokens=6, ignore_eos=True)) for p in prompts(4, seed=7)])
    assert eng.get_stats()["pool_embed_launches"] == 0 and eng.runner.d_pool is None and eng.runner.h_pool is None
    del eng
    torch.cuda.empty_cache()
