"""Structured outputs (guided_json) through the engine on the MI355X: the schema decode graphs (... -> ops.byte_guide
-> ops.json_guide -> ops.schema_guide -> the sampling tail; a fifth set, replayed only by batches with a schema row)
in windows of 4 with a continuation queued behind each, the eager path, slots and arena regions, the launch counters
of every graph set, and a batch that mixes plain, penalised, CSR-guided, byte-guided, JSON and schema rows.
engine.token_bytes is the seeded 32,000-entry table of tests/json_guide_reference.py: all 256 single bytes and
tokens of 2..8 bytes rich in JSON punctuation.

Nothing here depends on what the random model prefers: a sampled row's bytes are checked against the simulator and
the validator of tests/schema_guide_reference.py, a steered row is decided by biases of 100 / 60 / 50 among the
tokens the guide allows, against logits below about 3.5 in magnitude."""

import json
import random
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import guided, ops  # noqa: E402
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402

from tests import json_guide_reference as json_oracle  # noqa: E402
from tests import schema_guide_reference as oracle  # noqa: E402

EOS = 2
VOCAB = 32000
TABLE = json_oracle.engine_table(VOCAB)
STEPS = 10
UPPER = r"[A-D]{9}"                         # no multi-byte token has a capital: exactly nine tokens and EOS
NEST = {"type": "object", "properties": {"n": {"anyOf": [{"$ref": "#"}, {"type": "null"}]}}, "required": ["n"]}
POINT = {"type": "object", "properties": {"x": {"type": "integer"}, "tag": {"enum": ["a", "b"]},
                                          "meta": {"type": "object"}}, "required": ["x"]}


def b(ch: str) -> int:
    return 3 + ord(ch)


# '{' above everything: the document nests to the depth cap, then null, then the closing braces
BIAS = {**{b(ch): 50.0 for ch in '":ul}'}, b("{"): 100.0, b("n"): 60.0}


def steered_ids(schema, bias, limit=400):
    """The simulator playing "the highest-biased allowed token"."""
    trans, accept = guided.schema_to_pda(schema)
    order = sorted(bias, key=lambda t: -bias[t])
    state, stack, out = 0, [], []
    while len(out) < limit:
        if accept[state] and not stack:
            return out + [EOS]
        for tok in order:
            r = oracle.feed(trans, len(trans), state, stack, TABLE[tok])
            if r not in (oracle.DEAD, oracle.BAD):
                break
        else:
            raise AssertionError("no biased token is allowed")
        out.append(tok)
        state, stack = r
    raise AssertionError("the steered document does not end")


def spell(ids):
    return b"".join(TABLE[t] for t in ids)


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
    assert r.graphs and set(r.graphs) == set(r.graphs_proc) == set(r.graphs_guided) == set(r.graphs_json) == \
        set(r.graphs_schema)
    assert r.schema_guide_launches == 0 and r.json_guide_launches == 0       # capture served no request
    return eng


def prompts(n, seed=0):
    rng = random.Random(seed)
    return [[rng.randrange(3, 30000) for _ in range(rng.randrange(3, 200))] for _ in range(n)]


def run(eng, ps, sps):
    done = {}
    for i, (p, sp) in enumerate(zip(ps, sps)):
        eng.add_request(f"sguide-{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    while eng.has_work():
        eng.step()
    return [done[i] for i in range(len(ps))]


def all_free(eng):
    r = eng.runner
    return (not r._guide_slots and not r._guide_refs and sorted(r._guide_free) == list(range(eng.cfg.max_num_seqs))
            and all(reg["refs"] == 0 for reg in r._guide_regions.values())
            and set(r._guide_lru) == set(r._guide_regions)
            and r._sguide_st.used == sum(g["auto"].n_states for g in r._guide_regions.values() if "sg" in g)
            and not r._pen_slots and sorted(r._pen_free) == list(range(eng.cfg.max_num_seqs)))


def check_output(seq, schema, max_tokens):
    ids = seq.output_ids
    body = spell(ids[:-1] if ids[-1] == EOS else ids)
    trans, accept = guided.schema_to_pda(schema)
    oracle.text_config(trans, len(trans), body)                   # asserts that no byte dies
    if ids[-1] == EOS:
        assert seq.finish_reason == "stop" and oracle.accepts(trans, accept, body)
        assert oracle.validate(json.loads(body.decode("utf-8")), schema), body
    else:
        assert seq.finish_reason == "length" and len(ids) == max_tokens


def check_steered(seq):
    want = steered_ids(NEST, BIAS)
    text = spell(want[:-1]).decode()
    assert text == '{"n":' * 32 + "null" + "}" * 32 and len(want) == 32 * 5 + 4 + 32 + 1
    assert seq.output_ids == want and seq.finish_reason == "stop", spell(seq.output_ids[:-1])
    assert oracle.validate(json.loads(text), NEST)


def test_the_steered_document_reaches_the_cap_across_windows_and_continuations(engine):
    assert isinstance(engine._compile_guide(SamplingParams(guided_json=NEST)), guided.SchemaGuide)
    st0 = engine.get_stats()
    sp = SamplingParams(max_tokens=260, guided_json=NEST, logit_bias=BIAS)
    seqs = run(engine, prompts(2, seed=1), [sp, sp])
    st1 = engine.get_stats()
    for s in seqs:
        check_steered(s)
    assert st1.get("queued_windows", 0) > st0.get("queued_windows", 0)
    assert st1["schema_guide_launches"] - st0["schema_guide_launches"] >= 196
    assert st1.get("guide_errors", 0) == 0 and all_free(engine)


def test_sampled_rows_validate_or_are_legal_prefixes(engine):
    schemas = [POINT, NEST, POINT, NEST, {"type": "array", "items": {"type": ["integer", "null"]}, "maxItems": 4}, {}]
    sps = [SamplingParams(max_tokens=40, guided_json=s, temperature=1.0, seed=i) for i, s in enumerate(schemas)]
    seqs = run(engine, prompts(6, seed=2), sps)
    for seq, s in zip(seqs, schemas):
        print(len(seq.output_ids), seq.finish_reason, spell([t for t in seq.output_ids if t != EOS]))
        check_output(seq, s, 40)
    assert engine.get_stats().get("guide_errors", 0) == 0 and all_free(engine)
    assert len([g for g in engine.runner._guide_regions.values() if "sg" in g]) >= 4


def mixed_requests(with_schema: bool):
    """Plain, penalised, CSR-guided, byte-guided and JSON rows and, behind them, two schema rows (one sampled, one
    steered) — or, without them, two plain rows on the same prompts in their place, so that every step has the same
    shape for the other rows in both runs."""
    sps = [SamplingParams(max_tokens=STEPS, ignore_eos=True),
           SamplingParams(max_tokens=STEPS, guided_regex=UPPER, temperature=1.0, seed=11),
           SamplingParams(max_tokens=STEPS, ignore_eos=True, logit_bias={777: 100}),
           SamplingParams(max_tokens=STEPS, ignore_eos=True, repetition_penalty=1.3),
           SamplingParams(max_tokens=STEPS, guided_json_object=True, logit_bias={b("{"): 90, b("}"): 80})]
    if not with_schema:
        sps += [SamplingParams(max_tokens=STEPS, ignore_eos=True), SamplingParams(max_tokens=STEPS, ignore_eos=True)]
    else:
        sps += [SamplingParams(max_tokens=STEPS, guided_json=POINT, temperature=1.0, seed=12),
                SamplingParams(max_tokens=STEPS, guided_json=NEST, logprobs=2,
                               logit_bias={**BIAS, b("{"): 55.0})]            # 'n' above '{': {"n":null}
    return prompts(7, seed=3), sps


def test_a_mixed_batch_keeps_its_other_rows_and_only_schema_batches_launch_the_op(engine):
    ps, sps = mixed_requests(True)
    engine.generate(ps, SamplingParams(max_tokens=1, ignore_eos=True))     # the prompts' blocks enter the prefix cache
    st0 = engine.get_stats()
    seqs = run(engine, ps, sps)
    st1 = engine.get_stats()
    assert re.fullmatch(UPPER.encode(), spell(seqs[1].output_ids[:-1])) and seqs[1].output_ids[-1] == EOS
    assert seqs[2].output_ids == [777] * STEPS
    assert seqs[4].output_ids == [b("{"), b("}"), EOS]
    # ten single-byte tokens, the whole budget: the document is complete, EOS would have been the eleventh
    assert spell(seqs[6].output_ids) == b'{"n":null}' and seqs[6].finish_reason == "length"
    for e in seqs[6].output_logprobs:                                      # the logprobs of the masked row
        assert e["logprob"] > float("-inf")
    check_output(seqs[5], POINT, STEPS)
    d = {k: st1[k] - st0[k] for k in ("token_guide_launches", "byte_guide_launches", "json_guide_launches",
                                      "schema_guide_launches", "logit_process_launches")}
    # every step is guided; the steps with a schema row replay the set with the ops.schema_guide launch
    assert d["token_guide_launches"] == d["byte_guide_launches"] >= STEPS
    assert 0 < d["schema_guide_launches"] <= d["byte_guide_launches"]
    assert 0 < d["json_guide_launches"] <= d["byte_guide_launches"]
    assert st1.get("guide_errors", 0) == 0 and all_free(engine)
    # the same requests without the schema rows: the other rows' tokens are the same, the plain row included
    ps2, sps2 = mixed_requests(False)
    seqs2 = run(engine, ps2, sps2)
    for i in range(5):
        print(f"row {i}: with schema rows {seqs[i].output_ids} without {seqs2[i].output_ids}")
        assert seqs[i].output_ids == seqs2[i].output_ids, i
    st2 = engine.get_stats()
    assert st2["schema_guide_launches"] == st1["schema_guide_launches"]    # a JSON batch: the JSON set of old
    assert st2["json_guide_launches"] > st1["json_guide_launches"]
    # the plain row of the mixed batch equals its solo run, which replays the raw graphs
    solo = run(engine, [ps[0]], [sps[0]])[0]
    print(f"row 0 alone: {solo.output_ids}")
    assert seqs[0].output_ids == solo.output_ids and len(solo.output_ids) == STEPS
    st2 = engine.get_stats()
    # guided without JSON, processed and raw batches: their own counters move as before, the schema counter never
    run(engine, ps[:2], [sps[1], sps[1]])
    st3 = engine.get_stats()
    assert st3["byte_guide_launches"] - st2["byte_guide_launches"] >= STEPS
    assert st3["json_guide_launches"] == st2["json_guide_launches"]
    run(engine, ps[:2], [sps[2], sps[3]])
    st4 = engine.get_stats()
    assert st4["logit_process_launches"] - st3["logit_process_launches"] >= STEPS
    assert st4["token_guide_launches"] == st3["token_guide_launches"]
    engine.generate(ps, SamplingParams(max_tokens=STEPS, ignore_eos=True))
    st5 = engine.get_stats()
    for k in d:
        assert st5[k] == st4[k], k                                         # no row asked: the raw graphs, nothing else
    assert st5["schema_guide_launches"] == st1["schema_guide_launches"] and all_free(engine)


def test_an_eager_engine_gives_the_same_steered_tokens(engine):
    sp = SamplingParams(max_tokens=260, guided_json=NEST, logit_bias=BIAS)
    ps = prompts(1, seed=5)
    graph = run(engine, ps, [sp])[0]
    eager = make(False)
    assert not eager.runner.graphs and not eager.runner.graphs_json and not eager.runner.graphs_schema
    got = run(eager, ps, [sp])[0]
    check_steered(graph)
    check_steered(got)
    assert eager.get_stats()["schema_guide_launches"] > 0 and eager.get_stats().get("guide_errors", 0) == 0
    assert all_free(eager) and all_free(engine)
