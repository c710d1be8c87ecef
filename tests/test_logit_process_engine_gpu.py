"""Penalties and logit_bias through the engine on the MI355X: the processed decode graphs (windows of 4, a
continuation queued behind each), the eager prefill launch, slots, mixed batches, logprobs of the processed row.

The requests of the recompute comparison are built so that the oracle's arithmetic, not the random model, decides
their tokens: three or four tokens absent from the prompt get biases near +100 a few units apart, and
repetition_penalty = 10 divides a generated token's value (and the model's share of it) by ten, after which
frequency_penalty takes 2 per occurrence. The processed values then form ladders whose rungs are at least 0.4
apart (10 - 2c, 9.3 - 2c, 8.6 - 2c, ...), the model's logits (|z| below about 3.5 for llama-mini) move a rung by
z / 10, and only around step 10 do the rungs come down to the unbiased tokens. So the reference's first near-tie
(processed margin below 0.25, the threshold of tests/test_engine_gpu.py) cannot come before step 6, which the
test asserts. A step that forgot to count the latest token picks the same token twice and fails at once."""

import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402

from tests.logit_process_reference import agree_until_near_tie, greedy_reference_processed  # noqa: E402

STEPS = 12
MARGIN = 0.25
VOCAB = 32000
BIASED = list(range(31000, 31016, 2))       # eight ids no prompt holds (the prompts draw below 30000)
LADDERS = (dict(logit_bias={31001: 100, 31003: 93, 31005: 86}, repetition_penalty=10, frequency_penalty=2.0),
           dict(logit_bias={31101: 100, 31103: 96, 31105: 91, 31107: 87}, repetition_penalty=10, frequency_penalty=2.0),
           dict(logit_bias={31201: 100, 31203: 94, 31205: 87}, repetition_penalty=10, frequency_penalty=2.0,
                presence_penalty=0.5))


def make(graphs: bool) -> LLMEngine:
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available()
    cfg = EngineConfig(max_num_seqs=8, max_num_batched_tokens=512, num_kv_blocks=512, max_latency_ms=0.0,
                       graph_batch_sizes=[1, 2, 4, 8], decode_window=4, use_cuda_graph=graphs)
    eng = LLMEngine.from_preset("llama-mini", device="cuda:0", cfg=cfg, max_model_len=1024)
    eng.eos_token_id = None
    return eng


@pytest.fixture(scope="module")
def engine():
    eng = make(True)
    assert eng.runner.graphs and set(eng.runner.graphs_proc) == set(eng.runner.graphs)
    return eng


def prompts(n, seed=0):
    rng = random.Random(seed)
    return [[rng.randrange(3, 30000) for _ in range(rng.randrange(3, 200))] for _ in range(n)]


def run(eng, ps, sps):
    done = {}
    for i, (p, sp) in enumerate(zip(ps, sps)):
        eng.add_request(f"pen-{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    while eng.has_work():
        eng.step()
    return [done[i] for i in range(len(ps))]


def all_slots_free(eng):
    r = eng.runner
    return not r._pen_slots and sorted(r._pen_free) == list(range(eng.cfg.max_num_seqs))


@pytest.fixture(scope="module")
def ladder_runs(engine):
    """(prompts, sampling parameters, the graph engine's tokens, stats before and after): shared by the tests."""
    ps = prompts(len(LADDERS), seed=1)
    sps = [SamplingParams(max_tokens=STEPS, **kw) for kw in LADDERS]
    st0 = engine.get_stats()
    outs = [s.output_ids for s in run(engine, ps, sps)]
    return ps, sps, outs, st0, engine.get_stats()


def test_bias_forces_a_token_across_windows_and_continuations(engine):
    st0 = engine.get_stats()
    out = run(engine, prompts(1), [SamplingParams(max_tokens=STEPS, logit_bias={12345: 100})])[0].output_ids
    st1 = engine.get_stats()
    assert out == [12345] * STEPS
    # a window of 4 and continuations queued behind it: the steps ran on the processed graphs
    assert st1.get("queued_windows", 0) > st0.get("queued_windows", 0)
    assert st1["logit_process_launches"] - st0["logit_process_launches"] >= STEPS
    assert all_slots_free(engine)


def test_repetition_penalty_gives_eight_distinct_tokens(engine):
    sp = SamplingParams(max_tokens=STEPS, logit_bias={t: 100 for t in BIASED}, repetition_penalty=50)
    out = run(engine, prompts(1, seed=2), [sp])[0].output_ids
    # +100 lifts the eight far above the rest; a generated one falls to about 2 — a latest token that was not
    # counted (the window's first step, a continuation's first step) would come twice
    assert sorted(out[:8]) == BIASED, out
    assert all_slots_free(engine)


def test_ladders_agree_with_the_no_cache_oracle_recompute(engine, ladder_runs):
    ps, sps, outs, st0, st1 = ladder_runs
    assert st1.get("queued_windows", 0) > st0.get("queued_windows", 0)
    for p, kw, o in zip(ps, LADDERS, outs):
        want, margins = greedy_reference_processed(engine.model, p, STEPS, rp=kw["repetition_penalty"],
                                                   freq=kw["frequency_penalty"], pres=kw.get("presence_penalty", 0.0),
                                                   bias=kw["logit_bias"])
        first = agree_until_near_tie(o, want, margins, MARGIN)
        print(f"ladder {sorted(kw['logit_bias'])}: compared {first} steps, margins {[round(m, 2) for m in margins]}")
        assert first >= 6, (first, margins)        # a badly chosen request fails loudly: it cannot shrink the check
        assert len(set(o[:len(kw["logit_bias"])])) == len(kw["logit_bias"])
    assert all_slots_free(engine)


def test_eager_decode_gives_the_same_tokens(ladder_runs):
    ps, sps, outs, _, _ = ladder_runs
    eager = make(False)
    assert not eager.runner.graphs and not eager.runner.graphs_proc
    assert [s.output_ids for s in run(eager, ps, sps)] == outs
    assert all_slots_free(eager)


def test_plain_requests_keep_their_tokens_and_their_graphs(engine):
    ps = prompts(4, seed=3)
    n0 = engine.get_stats()["logit_process_launches"]
    alone = engine.generate(ps, SamplingParams(max_tokens=STEPS))
    assert engine.get_stats()["logit_process_launches"] == n0      # no row asked: the raw graphs, nothing else
    sps = [SamplingParams(max_tokens=STEPS), SamplingParams(max_tokens=STEPS, **LADDERS[0]),
           SamplingParams(max_tokens=STEPS), SamplingParams(max_tokens=STEPS, logit_bias={777: 100})]
    outs = [s.output_ids for s in run(engine, ps, sps)]
    assert engine.get_stats()["logit_process_launches"] > n0
    assert outs[0] == alone[0] and outs[2] == alone[2]
    assert outs[3] == [777] * STEPS and len(set(outs[1][:3])) == 3
    assert all_slots_free(engine)


def test_logprobs_are_those_of_the_processed_row(engine):
    sp = SamplingParams(max_tokens=STEPS, logit_bias={4242: 100}, logprobs=0)
    s = run(engine, prompts(1, seed=4), [sp])[0]
    assert s.output_ids == [4242] * STEPS and len(s.output_logprobs) == STEPS
    for e in s.output_logprobs:      # +100 on one token: it holds all the mass of the processed distribution
        assert e["rank"] == 0 and -1e-3 <= e["logprob"] <= 0.0
    assert all_slots_free(engine)
