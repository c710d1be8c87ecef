"""JSON mode through the engine on the MI355X: the JSON decode graphs (LM head -> ops.logit_process ->
ops.token_guide -> ops.byte_guide -> ops.json_guide -> the sampling tail; a set of their own, replayed only by
batches with a JSON row) in windows of 4 with a continuation queued
behind each, the eager prefill launch, slots and regions, and batches that mix plain, penalised, CSR-guided,
byte-guided and JSON rows. engine.token_bytes is a seeded 32,000-entry table: all 256 single bytes, '{"k":' and
tokens of 2..8 bytes rich in JSON punctuation.

Nothing here depends on what the random model prefers: a sampled row's bytes are checked against the recogniser of
tests/json_guide_reference.py, a steered row is decided by biases of 100 / 60 / 30 among the tokens the guide
allows, against logits below about 3.5 in magnitude."""

import json
import random
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.guided import JsonGuide  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402

from tests import json_guide_reference as oracle  # noqa: E402

EOS = 2
VOCAB = 32000
TABLE = oracle.engine_table(VOCAB)
KEY = oracle.ENGINE_KEY
STEPS = 10
UPPER = r"[A-D]{9}"                         # no multi-byte token has a capital: exactly nine tokens and EOS
TAIL = [31010 + i for i in range(7)]


def b(ch: str) -> int:
    return 3 + ord(ch)


BIAS = {KEY: 100.0, b("0"): 60.0, b("}"): 30.0}      # ranks '{"k":' above '0' above '}'


def steered_ids(bias=BIAS, limit=200):
    """The recogniser simulating "the highest-biased allowed token"."""
    order = sorted(bias, key=lambda t: -bias[t])
    cfg, out = oracle.START, []
    while len(out) < limit:
        if cfg[0] == "done":
            return out + [EOS]
        tok = next(t for t in order if oracle.token_feed(cfg, t, TABLE) is not None)
        out.append(tok)
        cfg = oracle.token_feed(cfg, tok, TABLE)
    raise AssertionError("the steered document does not end")


def make(graphs: bool, blocks: int = 512, seqs: int = 8) -> LLMEngine:
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available()
    cfg = EngineConfig(max_num_seqs=seqs, max_num_batched_tokens=512, num_kv_blocks=blocks, max_latency_ms=0.0,
                       graph_batch_sizes=[1, 2, 4, 8], decode_window=4, use_cuda_graph=graphs,
                       enable_prefix_caching=True, preemption_mode="auto")
    eng = LLMEngine.from_preset("llama-mini", device="cuda:0", cfg=cfg, max_model_len=1024)
    eng.eos_token_id = EOS
    eng.token_bytes = TABLE
    return eng


@pytest.fixture(scope="module")
def engine():
    eng = make(True)
    r = eng.runner
    assert r.graphs and set(r.graphs_guided) == set(r.graphs) == set(r.graphs_proc) == set(r.graphs_json)
    return eng


def prompts(n, seed=0):
    rng = random.Random(seed)
    return [[rng.randrange(3, 30000) for _ in range(rng.randrange(3, 200))] for _ in range(n)]


def run(eng, ps, sps):
    done = {}
    for i, (p, sp) in enumerate(zip(ps, sps)):
        eng.add_request(f"jguide-{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    while eng.has_work():
        eng.step()
    return [done[i] for i in range(len(ps))]


def all_free(eng):
    r = eng.runner
    return (not r._guide_slots and not r._guide_refs and sorted(r._guide_free) == list(range(eng.cfg.max_num_seqs))
            and all(reg["refs"] == 0 for reg in r._guide_regions.values())
            and set(r._guide_lru) == set(r._guide_regions)
            and r.guide_arena_states_used() == sum(g["auto"].n_states for g in r._guide_regions.values() if "st" in g)
            and not r._pen_slots and sorted(r._pen_free) == list(range(eng.cfg.max_num_seqs)))


def check_steered(seq):
    want = steered_ids()
    assert want == [KEY] * 32 + [b("0")] + [b("}")] * 32 + [EOS] and len(want) == 66
    assert seq.output_ids == want and seq.finish_reason == "stop", seq.output_ids
    doc, depth = json.loads(oracle.spell(TABLE, seq.output_ids[:-1])), 0
    while isinstance(doc, dict):
        doc, depth = doc["k"], depth + 1
    assert depth == 32 and doc == 0


def test_the_steered_document_reaches_the_cap_across_windows_and_continuations(engine):
    assert isinstance(engine._compile_guide(SamplingParams(guided_json_object=True)), JsonGuide)
    st0 = engine.get_stats()
    sp = SamplingParams(max_tokens=80, guided_json_object=True, logit_bias=BIAS)
    ps = prompts(2, seed=1)
    seqs = run(engine, ps, [sp, sp])
    st1 = engine.get_stats()
    for s in seqs:
        check_steered(s)
    assert st1.get("queued_windows", 0) > st0.get("queued_windows", 0)
    assert st1["json_guide_launches"] - st0["json_guide_launches"] >= 64
    assert st1.get("guide_errors", 0) == 0 and all_free(engine)


def test_sampled_rows_are_legal_prefixes_and_finished_ones_parse(engine):
    sps = [SamplingParams(max_tokens=40, guided_json_object=True, temperature=1.0, seed=s) for s in range(6)]
    seqs = run(engine, prompts(6, seed=2), sps)
    for s in seqs:
        ids = s.output_ids
        body = ids[:-1] if ids[-1] == EOS else ids
        text = oracle.spell(TABLE, body)
        print(len(ids), s.finish_reason, text)
        assert EOS not in body and oracle.accepts_prefix(text), (ids, text)
        if ids[-1] == EOS:
            assert s.finish_reason == "stop" and isinstance(json.loads(text), dict)
        else:
            assert s.finish_reason == "length" and len(ids) == 40
    assert engine.get_stats().get("guide_errors", 0) == 0 and all_free(engine)


def mixed_requests(with_json: bool):
    """Plain, penalised, CSR-guided and byte-guided rows and, behind them, two JSON rows (one sampled, one steered to
    '{', '}', EOS) — or, without JSON, two plain rows on the same prompts in their place, so that the prefill step
    and every decode step have the same shape for the other rows in both runs."""
    sps = [SamplingParams(max_tokens=STEPS, ignore_eos=True),
           SamplingParams(max_tokens=STEPS, guided_regex=UPPER, temperature=1.0, seed=11),
           SamplingParams(max_tokens=STEPS, ignore_eos=True, logit_bias={777: 100}),
           SamplingParams(max_tokens=STEPS, ignore_eos=True, repetition_penalty=1.3),
           SamplingParams(max_tokens=STEPS, guided_choice=[[31001, 5] + TAIL, [31001, 6] + TAIL], logit_bias={6: 100})]
    if not with_json:
        sps += [SamplingParams(max_tokens=STEPS, ignore_eos=True), SamplingParams(max_tokens=STEPS, ignore_eos=True)]
    else:
        sps += [SamplingParams(max_tokens=STEPS, guided_json_object=True, temperature=1.0, seed=12),
                SamplingParams(max_tokens=STEPS, guided_json_object=True, logit_bias={b("{"): 90, b("}"): 80},
                               logprobs=2)]
    return prompts(7, seed=3), sps


def test_a_mixed_batch_keeps_its_other_rows_and_frees_everything(engine):
    ps, sps = mixed_requests(True)
    engine.generate(ps, SamplingParams(max_tokens=1, ignore_eos=True))     # the prompts' blocks enter the prefix cache
    st0 = engine.get_stats()
    seqs = run(engine, ps, sps)
    st1 = engine.get_stats()
    assert re.fullmatch(UPPER.encode(), oracle.spell(TABLE, seqs[1].output_ids[:-1])) and seqs[1].output_ids[-1] == EOS
    assert seqs[2].output_ids == [777] * STEPS
    assert seqs[4].output_ids == [31001, 6] + TAIL + [EOS]
    assert seqs[6].output_ids == [b("{"), b("}"), EOS]                     # the shortest document
    for e in seqs[6].output_logprobs:                                      # the logprobs of the masked row
        assert e["logprob"] > float("-inf")
    body = [t for t in seqs[5].output_ids if t != EOS]
    assert oracle.accepts_prefix(oracle.spell(TABLE, body))
    d_tok = st1["token_guide_launches"] - st0["token_guide_launches"]
    d_byte = st1["byte_guide_launches"] - st0["byte_guide_launches"]
    d_json = st1["json_guide_launches"] - st0["json_guide_launches"]
    # every step is guided; the steps with a JSON row replay the set with the ops.json_guide launch
    assert d_tok == d_byte >= STEPS and 0 < d_json <= d_byte
    assert st1.get("guide_errors", 0) == 0 and all_free(engine)
    # the same requests without the JSON rows: the other rows' tokens are the same
    ps2, sps2 = mixed_requests(False)
    seqs2 = run(engine, ps2, sps2)
    for i in range(5):
        print(f"row {i}: with json {seqs[i].output_ids} without {seqs2[i].output_ids}")
        assert seqs[i].output_ids == seqs2[i].output_ids, i
    st2 = engine.get_stats()
    assert st2["json_guide_launches"] == st1["json_guide_launches"]        # guided, no JSON row: the guided set of old
    assert st2["byte_guide_launches"] - st1["byte_guide_launches"] >= STEPS
    engine.generate(ps, SamplingParams(max_tokens=STEPS, ignore_eos=True))
    st3 = engine.get_stats()
    assert st3["json_guide_launches"] == st2["json_guide_launches"]        # no row asked: the raw graphs, nothing else
    assert st3["byte_guide_launches"] == st2["byte_guide_launches"] and all_free(engine)


def test_an_eager_engine_gives_the_same_steered_tokens(engine):
    sp = SamplingParams(max_tokens=80, guided_json_object=True, logit_bias=BIAS)
    ps = prompts(1, seed=5)
    graph = run(engine, ps, [sp])[0]
    eager = make(False)
    assert not eager.runner.graphs and not eager.runner.graphs_guided and not eager.runner.graphs_json
    got = run(eager, ps, [sp])[0]
    check_steered(graph)
    check_steered(got)
    assert eager.get_stats()["json_guide_launches"] > 0
    assert all_free(eager) and all_free(engine)
