"""guided_regex over a multi-byte vocabulary through the engine on the MI355X: the guided decode graphs (LM head ->
ops.logit_process -> ops.token_guide -> ops.byte_guide -> the sampling tail) in windows of 4 with a continuation
queued behind each, the eager prefill launch, slots and arena regions, batches that mix plain, penalised,
CSR-guided and byte-guided rows. engine.token_bytes is a seeded 32,000-entry table with tokens of 1..8 bytes.

Nothing here depends on what the random model prefers: a sampled row's bytes are checked against the pattern, a
decisive row is decided by a bias of 50 among the tokens the guide allows."""

import random
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from src import ops  # noqa: E402
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.guided import ByteGuide  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402

from tests import byte_guide_reference as oracle  # noqa: E402

EOS = 2
VOCAB = 32000
TABLE = oracle.engine_table(VOCAB)
PATTERN = r"([a-d]{1,3} ){5}\d{2}"          # 17..27 bytes: several windows whatever tokens spell them
UPPER = r"[A-D]{9}"                         # no multi-byte token has a capital: exactly nine tokens and EOS
STEPS = 10                                  # every row of the mixed batch ends in the same step (see mixed_requests)
WIDE = r"[a-z ]{0,200}"                     # beyond the CSR form's edge cap on this table
TAIL = [31010 + i for i in range(7)]


def b(ch: str) -> int:
    return 3 + ord(ch)


def make(graphs: bool, blocks: int = 512, seqs: int = 8) -> LLMEngine:
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available()
    cfg = EngineConfig(max_num_seqs=seqs, max_num_batched_tokens=512, num_kv_blocks=blocks, max_latency_ms=0.0,
                       graph_batch_sizes=[1, 2, 4, 8], decode_window=4, use_cuda_graph=graphs,
                       enable_prefix_caching=blocks >= 512, preemption_mode="auto" if blocks >= 512 else "recompute")
    eng = LLMEngine.from_preset("llama-mini", device="cuda:0", cfg=cfg, max_model_len=1024)
    eng.eos_token_id = EOS
    eng.token_bytes = TABLE
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
        eng.add_request(f"bguide-{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
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


def test_sampled_rows_match_across_windows_and_continuations(engine):
    st0 = engine.get_stats()
    sps = [SamplingParams(max_tokens=40, guided_regex=PATTERN, temperature=1.0, seed=s) for s in range(6)]
    seqs = run(engine, prompts(6, seed=1), sps)
    st1 = engine.get_stats()
    multi = 0
    for s in seqs:
        assert s.output_ids[-1] == EOS and s.finish_reason == "stop", s.output_ids
        text = oracle.spell(TABLE, s.output_ids[:-1])
        print(len(s.output_ids), text)
        assert re.fullmatch(PATTERN.encode(), text), (s.output_ids, text)
        multi += sum(len(TABLE[t]) > 1 for t in s.output_ids[:-1])
    assert multi > 0                                        # 60-odd draws among sets that are mostly multi-byte
    assert st1.get("queued_windows", 0) > st0.get("queued_windows", 0)
    assert st1["byte_guide_launches"] - st0["byte_guide_launches"] >= 8
    assert st1.get("guide_errors", 0) == 0 and all_free(engine)


def test_a_pattern_over_the_edge_cap_is_admitted_and_matches(engine):
    guide = engine._compile_guide(SamplingParams(guided_regex=WIDE))
    assert isinstance(guide, ByteGuide) and guide.n_states == 201
    sps = [SamplingParams(max_tokens=12, guided_regex=WIDE, temperature=1.0, seed=s) for s in (1, 2)]
    for s in run(engine, prompts(2, seed=2), sps):
        body = s.output_ids[:-1] if s.output_ids[-1] == EOS else s.output_ids
        assert EOS not in body and re.fullmatch(WIDE.encode(), oracle.spell(TABLE, body)), s.output_ids
    assert engine.get_stats().get("guide_errors", 0) == 0 and all_free(engine)


def mixed_requests():
    """Plain, penalised, CSR-guided and byte-guided rows in one batch. Every row generates exactly STEPS tokens, so
    the batch keeps its shape to the end and the plain rows can be compared with a run of the same shape in which
    nobody is guided."""
    sps = [SamplingParams(max_tokens=STEPS, ignore_eos=True),
           SamplingParams(max_tokens=STEPS, guided_regex=UPPER, temperature=1.0, seed=11),
           SamplingParams(max_tokens=STEPS, ignore_eos=True, logit_bias={777: 100}),
           SamplingParams(max_tokens=STEPS, guided_regex=UPPER, temperature=1.0, seed=12, repetition_penalty=1.3),
           SamplingParams(max_tokens=STEPS, ignore_eos=True),
           SamplingParams(max_tokens=STEPS, guided_regex=UPPER, temperature=0.7, seed=13, logprobs=2),
           SamplingParams(max_tokens=STEPS, guided_choice=[[31001, 5] + TAIL, [31001, 6] + TAIL], logit_bias={6: 100})]
    return prompts(len(sps), seed=3), sps


def test_a_mixed_batch_keeps_its_plain_rows_and_its_graphs(engine):
    ps, sps = mixed_requests()
    engine.generate(ps, SamplingParams(max_tokens=1, ignore_eos=True))     # the prompts' blocks enter the prefix cache
    st0 = engine.get_stats()
    seqs = run(engine, ps, sps)
    st1 = engine.get_stats()
    for i in (1, 3, 5):
        s = seqs[i]
        assert s.output_ids[-1] == EOS and s.finish_reason == "stop", s.output_ids
        assert re.fullmatch(UPPER.encode(), oracle.spell(TABLE, s.output_ids[:-1])), s.output_ids
    assert seqs[2].output_ids == [777] * STEPS
    assert seqs[6].output_ids == [31001, 6] + TAIL + [EOS]
    for tok, e in zip(seqs[5].output_ids, seqs[5].output_logprobs):        # the logprobs of the masked row
        assert e["logprob"] > float("-inf") and e["rank"] in (0, 1, 2, 3)  # one of at most four allowed tokens
    d_tok = st1["token_guide_launches"] - st0["token_guide_launches"]
    d_byte = st1["byte_guide_launches"] - st0["byte_guide_launches"]
    assert d_tok == d_byte >= STEPS                                        # the guided set: both launches, every step
    assert st1.get("guide_errors", 0) == 0 and all_free(engine)
    alone = engine.generate(ps, SamplingParams(max_tokens=STEPS, ignore_eos=True))
    st2 = engine.get_stats()
    assert st2["byte_guide_launches"] == st1["byte_guide_launches"]        # no row asked: the raw graphs, nothing else
    assert st2["token_guide_launches"] == st1["token_guide_launches"]
    for i in (0, 4):
        print(f"plain row {i}: mixed {seqs[i].output_ids} alone {alone[i]}")
    assert seqs[0].output_ids == alone[0] and seqs[4].output_ids == alone[4]


def test_a_preempted_and_recomputed_row_continues_legally():
    eng = make(False, blocks=12, seqs=4)
    pattern = r"([A-D]\d){14}x"                             # capitals: one byte per token, 28 or 29 tokens and EOS
    ps = [p[:40] for p in prompts(4, seed=3)]
    sps = [SamplingParams(max_tokens=30, guided_regex=pattern, temperature=1.0, seed=s) for s in range(4)]
    seqs = run(eng, ps, sps)
    assert eng.scheduler.num_preemptions > 0
    for s in seqs:
        assert len(s.output_ids) in (29, 30) and s.output_ids[-1] == EOS    # the last digit and 'x' may be one token
        assert re.fullmatch(pattern.encode(), oracle.spell(TABLE, s.output_ids[:-1]))
    assert eng.get_stats().get("guide_errors", 0) == 0 and all_free(eng)


def decisive_requests():
    """Requests whose every token is decided by the guide, or by a bias of 50 against logits below about 3.5 in
    magnitude among the tokens the guide allows: the same in any engine, whatever its GEMM tiles do to the last
    bit of a logit."""
    ab, cd = oracle.ENGINE_AB, oracle.ENGINE_CD
    sps = [SamplingParams(max_tokens=STEPS, guided_regex="(ab|cd){4}x", logit_bias={b("c"): 50, b("d"): 50}),
           SamplingParams(max_tokens=STEPS, guided_regex="(ab|cd){4}x", logit_bias={ab: 50}, logprobs=1),
           SamplingParams(max_tokens=STEPS, guided_regex="(ab|cd){4}x", logit_bias={cd: 50, b("a"): 25}),
           SamplingParams(max_tokens=STEPS, guided_choice=[[31001, 5, 31002], [31001, 6]], logit_bias={5: 50}),
           SamplingParams(max_tokens=STEPS, allowed_token_ids=[100, 200, 300], logit_bias={200: 50}, ignore_eos=True),
           SamplingParams(max_tokens=STEPS, ignore_eos=True, logit_bias={777: 100})]
    want = [[b("c"), b("d")] * 4 + [b("x"), EOS], [ab] * 4 + [b("x"), EOS], [cd] * 4 + [b("x"), EOS],
            [31001, 5, 31002, EOS], [200] * STEPS, [777] * STEPS]
    return prompts(len(sps), seed=5), sps, want


def test_an_eager_engine_gives_the_same_tokens(engine):
    ps, sps, want = decisive_requests()
    graph = [s.output_ids for s in run(engine, ps, sps)]
    eager = make(False)
    assert not eager.runner.graphs and not eager.runner.graphs_guided
    got = [s.output_ids for s in run(eager, ps, sps)]
    assert got == graph == want
    assert eager.get_stats()["byte_guide_launches"] > 0
    assert all_free(eager) and all_free(engine)
