"""The engine with kv_cache_dtype="fp8" on the MI355X (llama-tiny): twice the blocks in the same memory, tokens and
chosen-token logprobs against the same model on CPU tensors (the reference ops with the same FP8 cache semantics) by
test_engine_gpu.py's rule (agreement up to the reference's first near-tie), a prefix-cache hit that reads FP8 blocks
through prefill, hipGraph decode windows against single steps, and the refusals."""

import random
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.config import EngineConfig, ModelConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.engine.llm_engine import check_kv_cache_dtype, plan_kv_blocks  # noqa: E402
from src.models.llama import AttnMetadata  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402

STEPS, THR = 10, 0.25


def config(**kw):
    return EngineConfig(max_num_seqs=8, max_num_batched_tokens=512, max_latency_ms=0.0, graph_batch_sizes=[1, 2, 4, 8],
                        **kw)


@pytest.fixture(scope="module")
def engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available()
    eng = LLMEngine.from_preset("llama-tiny", device="cuda:0", cfg=config(num_kv_blocks=512, kv_cache_dtype="fp8"),
                                max_model_len=1024)
    eng.eos_token_id = None
    eng.model.kv_scales = [(0.5, 2.0), (1.0, 0.25)]   # not all ones: a scale lost on the way shows
    return eng


def run(eng, ps, sp):
    done = {}
    for i, p in enumerate(ps):
        eng.add_request(f"kv8-{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    while eng.has_work():
        eng.step()
    return [done[i] for i in range(len(ps))]


@torch.inference_mode()
def cpu_reference(model, prompt, n):
    """Greedy recompute on CPU tensors through an FP8 pool: tokens, top1 - top2 margins, chosen-token logprobs."""
    ids, toks, margins, lps = list(prompt), [], [], []
    nb = (len(prompt) + n + 15) // 16
    pool = torch.zeros(model.arch.num_layers, 2, nb, model.hkv, 16, 128, dtype=torch.uint8)
    for _ in range(n):
        t = len(ids)
        pos = torch.arange(t)
        meta = AttnMetadata(True, pos.clone(), torch.arange(nb, dtype=torch.int32)[None],
                            torch.tensor([t], dtype=torch.int32), torch.tensor([0, t], dtype=torch.int32), t)
        lg = model.compute_logits(model.forward(torch.tensor(ids), pos, meta, pool)[-1:])[0].float()
        top = torch.topk(lg, 2)
        toks.append(int(top.indices[0]))
        margins.append(float(top.values[0] - top.values[1]))
        lps.append(float(torch.log_softmax(lg, -1)[toks[-1]]))
        ids.append(toks[-1])
    return toks, margins, lps


def test_twice_the_blocks_in_the_same_memory(engine):
    n16, n8 = (plan_kv_blocks(engine.arch, engine.model, config(kv_cache_dtype=d), engine.device)
               for d in ("auto", "fp8"))
    assert n8 in (2 * n16, 2 * n16 + 1), (n16, n8)
    assert engine.pool.tensor.element_size() == 1 and engine.pool.nbytes == engine.pool.tensor.numel()


def test_tokens_and_logprobs_match_the_cpu_engine(engine):
    rng = random.Random(0)
    ps = [[rng.randrange(3, 1000) for _ in range(rng.randrange(3, 300))] for _ in range(12)]
    seqs = run(engine, ps, SamplingParams(max_tokens=STEPS, logprobs=0))
    assert engine.runner.graphs, "decode hipGraphs should be captured"
    cpu = engine.model.reference_copy("cpu", torch.float32)
    assert cpu.kv_scales == engine.model.kv_scales
    compared, worst = 0, 0.0
    for p, s in zip(ps, seqs):
        toks, margins, lps = cpu_reference(cpu, p, STEPS)
        for j, (tok, m) in enumerate(zip(toks, margins)):
            if s.output_ids[j] != tok:  # the contexts part here: allowed only at a near-tie of the reference
                assert m < THR, (j, s.output_ids, toks, margins)
                break
            d = abs(s.output_logprobs[j]["logprob"] - lps[j])
            worst, compared = max(worst, d), compared + 1
            assert d <= THR, (j, d)
    print(f"FP8 engine vs CPU tensors: max |delta logprob| {worst:.3e} over {compared} steps")
    assert compared > 0


def test_prefix_hit_reads_fp8_blocks_through_prefill(engine):
    rng = random.Random(1)
    shared = [rng.randrange(3, 1000) for _ in range(400)]
    ps = [shared + [5, 6], shared + [7, 8, 9]]
    hits0 = engine.stats["prefix_hit_tokens"]
    first = engine.generate(ps, SamplingParams(max_tokens=6))
    again = engine.generate(ps, SamplingParams(max_tokens=6))
    assert engine.stats["prefix_hit_tokens"] > hits0 and first == again


def test_graph_windows_match_single_steps(engine, monkeypatch):
    rng = random.Random(2)
    ps = [[rng.randrange(3, 1000) for _ in range(rng.randrange(3, 200))] for _ in range(5)]
    windows = engine.generate(ps, SamplingParams(max_tokens=STEPS))
    monkeypatch.setattr(engine, "_decode_window", lambda seqs: 1)
    monkeypatch.setattr(engine.runner, "graphs", {})   # eager single steps
    assert engine.generate(ps, SamplingParams(max_tokens=STEPS)) == windows


def test_refusals(engine):
    from src.engine.backend import LLMBackend

    fp8 = config(num_kv_blocks=64, kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="MoE"):
        LLMEngine.from_preset("mixtral-tiny", device="cuda:0", cfg=fp8, max_model_len=256, capture=False)
    with pytest.raises(ValueError, match="tensor-parallel"):
        check_kv_cache_dtype(fp8, SimpleNamespace(tp=SimpleNamespace(enabled=True)))
    for kw, what in ((dict(tp_size=2), "tensor-parallel"), (dict(role="prefill"), "disaggregated"),
                     (dict(role="decode"), "disaggregated")):
        with pytest.raises(ValueError, match=what):
            LLMBackend(ModelConfig("m", "", arch="llama", preset="llama-tiny", kv_cache_dtype="fp8", **kw))
    with pytest.raises(ValueError, match="export"):
        engine.add_request("kv8-export", [5, 6, 7], SamplingParams(max_tokens=1), export_kv=True)
    with pytest.raises(ValueError, match="auto / fp8"):
        plan_kv_blocks(engine.arch, engine.model, config(kv_cache_dtype="int4"), engine.device)
