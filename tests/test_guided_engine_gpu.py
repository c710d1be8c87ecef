"""Constrained decoding through the engine on the MI355X: the guided decode graphs (LM head -> ops.logit_process ->
ops.token_guide -> the sampling tail) in windows of 4 with a continuation queued behind each, the eager prefill
launch, slots and arena regions, batches that mix plain, penalised and guided rows.

Nothing here depends on what the random model prefers: a forced choice has one legal token per step, and a
sampled regex output is checked against the pattern, not against particular tokens."""

import random
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.preproc import ByteTokenizer, SamplingParams  # noqa: E402

EOS = 2
PATTERN = "(ab|cd){4}x"                     # nine tokens and EOS: two windows and a continuation
STEPS = 10                                  # every row of the mixed batch ends in the same step (see mixed_requests)
TAIL = [31010 + i for i in range(7)]
TOK = ByteTokenizer(32000)


def make(graphs: bool) -> LLMEngine:
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available()
    cfg = EngineConfig(max_num_seqs=8, max_num_batched_tokens=512, num_kv_blocks=512, max_latency_ms=0.0,
                       graph_batch_sizes=[1, 2, 4, 8], decode_window=4, use_cuda_graph=graphs)
    eng = LLMEngine.from_preset("llama-mini", device="cuda:0", cfg=cfg, max_model_len=1024)
    eng.eos_token_id = EOS
    return eng


@pytest.fixture(scope="module")
def engine():
    eng = make(True)
    r = eng.runner
    assert r.graphs and set(r.graphs_guided) == set(r.graphs) == set(r.graphs_proc)
    return eng


def prompts(n, seed=0):
    rng = random.Random(seed)
    return [[rng.randrange(3, 30000) for _ in range(rng.randrange(3, 200))] for _ in range(n)]


def run(eng, ps, sps):
    done = {}
    for i, (p, sp) in enumerate(zip(ps, sps)):
        eng.add_request(f"guide-{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    while eng.has_work():
        eng.step()
    return [done[i] for i in range(len(ps))]


def all_free(eng):
    r = eng.runner
    return (not r._guide_slots and not r._guide_refs and sorted(r._guide_free) == list(range(eng.cfg.max_num_seqs))
            and all(reg["refs"] == 0 for reg in r._guide_regions.values())
            and not r._pen_slots and sorted(r._pen_free) == list(range(eng.cfg.max_num_seqs)))


def mixed_requests():
    """Plain, penalised and guided rows in one batch (sampled regex rows with several seeds, a choice of two).
    Every row generates exactly STEPS tokens, so the batch keeps its shape to the end and the plain rows can be
    compared with a run of the same shape in which nobody is guided."""
    sps = [SamplingParams(max_tokens=STEPS, ignore_eos=True),
           SamplingParams(max_tokens=STEPS, guided_regex=PATTERN, temperature=1.0, seed=11),
           SamplingParams(max_tokens=STEPS, ignore_eos=True, logit_bias={777: 100}),
           SamplingParams(max_tokens=STEPS, guided_regex=PATTERN, temperature=1.0, seed=12, repetition_penalty=1.3),
           SamplingParams(max_tokens=STEPS, ignore_eos=True),
           SamplingParams(max_tokens=STEPS, guided_regex=PATTERN, temperature=0.7, seed=13, logprobs=2),
           SamplingParams(max_tokens=STEPS, guided_choice=[[31001, 5] + TAIL, [31001, 6] + TAIL], logit_bias={6: 100})]
    return prompts(len(sps), seed=3), sps


@pytest.fixture(scope="module")
def mixed_runs(engine):
    ps, sps = mixed_requests()
    # the prompts' full blocks enter the prefix cache here, so that this run and the all-plain run that
    # test_plain_rows_keep_their_tokens_and_their_graphs compares it with prefill the same rows
    engine.generate(ps, SamplingParams(max_tokens=1, ignore_eos=True))
    st0 = engine.get_stats()
    seqs = run(engine, ps, sps)
    return ps, sps, seqs, st0, engine.get_stats()


def test_a_forced_choice_crosses_windows_and_continuations(engine):
    choice = [31000 + 7 * i for i in range(11)]
    st0 = engine.get_stats()
    s = run(engine, prompts(1), [SamplingParams(max_tokens=32, guided_choice=[choice])])[0]
    st1 = engine.get_stats()
    assert s.output_ids == choice + [EOS] and s.finish_reason == "stop"
    assert st1.get("queued_windows", 0) > st0.get("queued_windows", 0)
    assert st1["token_guide_launches"] - st0["token_guide_launches"] >= len(choice) + 1
    assert st1.get("guide_errors", 0) == 0 and all_free(engine)


def test_sampled_regex_outputs_match_in_a_mixed_batch(engine, mixed_runs):
    ps, sps, seqs, st0, st1 = mixed_runs
    assert st1["token_guide_launches"] > st0["token_guide_launches"]
    assert st1.get("queued_windows", 0) > st0.get("queued_windows", 0)
    for i in (1, 3, 5):
        s = seqs[i]
        assert s.output_ids[-1] == EOS and s.finish_reason == "stop", s.output_ids
        assert re.fullmatch(PATTERN, TOK.decode(s.output_ids[:-1])), s.output_ids
    assert seqs[2].output_ids == [777] * STEPS
    assert seqs[6].output_ids == [31001, 6] + TAIL + [EOS]  # the bias chooses among the ALLOWED tokens
    # the logprobs of a guided row are those of the masked row: the sampled token is one of at most two allowed
    for tok, e in zip(seqs[5].output_ids, seqs[5].output_logprobs):
        assert e["logprob"] > float("-inf") and e["rank"] in (0, 1) and tok in e["top_ids"]
    assert st1.get("guide_errors", 0) == 0 and all_free(engine)


def test_plain_rows_keep_their_tokens_and_their_graphs(engine, mixed_runs):
    ps, sps, seqs, _, _ = mixed_runs
    n0 = engine.get_stats()["token_guide_launches"]
    alone = engine.generate(ps, SamplingParams(max_tokens=STEPS, ignore_eos=True))
    assert engine.get_stats()["token_guide_launches"] == n0   # no row asked: the raw graphs, nothing else
    for i in (0, 4):
        print(f"plain row {i}: mixed {seqs[i].output_ids} alone {alone[i]}")
    assert seqs[0].output_ids == alone[0] and seqs[4].output_ids == alone[4]


def decisive_requests():
    """Requests whose every token is decided by the guide, or by a bias of 50 against logits below about 3.5 in
    magnitude among the tokens the guide allows: the same in any engine, whatever its GEMM tiles do to the last
    bit of a logit (a sampled row's draw, or a plain row's near-tie, may differ between a padded graph batch and
    an eager one of another size; that is not what this compares)."""
    a, c = TOK.encode("a", add_bos=False)[0], TOK.encode("c", add_bos=False)[0]
    sps = [SamplingParams(max_tokens=32, guided_choice=[[31000 + 7 * i for i in range(11)]]),
           SamplingParams(max_tokens=STEPS, guided_regex=PATTERN, logit_bias={c: 50}),
           SamplingParams(max_tokens=STEPS, guided_regex=PATTERN, logit_bias={a: 50}, logprobs=1),
           SamplingParams(max_tokens=STEPS, allowed_token_ids=[100, 200, 300], logit_bias={200: 50}, ignore_eos=True),
           SamplingParams(max_tokens=STEPS, guided_choice=[[31001, 5, 31002], [31001, 6]], logit_bias={5: 50}),
           SamplingParams(max_tokens=STEPS, ignore_eos=True, logit_bias={777: 100})]
    want = [[31000 + 7 * i for i in range(11)] + [EOS], TOK.encode("cdcdcdcdx", add_bos=False) + [EOS],
            TOK.encode("ababababx", add_bos=False) + [EOS], [200] * STEPS, [31001, 5, 31002, EOS], [777] * STEPS]
    return prompts(len(sps), seed=5), sps, want


def test_an_eager_engine_gives_the_same_tokens(engine):
    ps, sps, want = decisive_requests()
    st0 = engine.get_stats()
    graph = [s.output_ids for s in run(engine, ps, sps)]
    assert engine.get_stats().get("queued_windows", 0) > st0.get("queued_windows", 0)
    eager = make(False)
    assert not eager.runner.graphs and not eager.runner.graphs_guided
    got = [s.output_ids for s in run(eager, ps, sps)]
    assert got == graph == want
    assert all_free(eager) and all_free(engine)
