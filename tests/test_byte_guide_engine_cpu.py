"""guided_regex over a multi-byte vocabulary through a CPU engine (reference.byte_guide_rows stands in for the
kernel) and through the serving path: an LLMBackend whose tokenizer is a ByteLevel BPE trained in memory and loaded
from a directory. Today's forms (allowed_token_ids, guided_choice, guided_regex on the byte-level table) keep their
CSR automaton beside it."""

import asyncio
import random
import re

import pytest

from src import ops
from src.config import ModelConfig
from src.engine.backend import LLMBackend
from src.guided import ByteGuide
from src.preproc import SamplingParams

from tests import byte_guide_reference as oracle
from tests.test_byte_guide_reference_cpu import bytelevel_tokenizer
from tests.test_engine_cpu import make_engine, prompts

EOS = 2
VOCAB = 1024          # llama-tiny
PATTERN = r"[a-d]{2,5}( \d{1,3}){1,2}"
WIDE = r"[a-z ]{0,200}"                         # 201 states; the CSR form needs an edge per state and allowed token


def byte_engine(**kw):
    eng = make_engine(**kw)
    eng.eos_token_id = EOS
    eng.token_bytes = oracle.engine_table(eng.arch.vocab_size)
    return eng


def run(eng, ps, sps):
    done = {}
    for i, (p, sp) in enumerate(zip(ps, sps)):
        eng.add_request(f"b{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    while eng.has_work():
        eng.step()
    return [done[i] for i in range(len(ps))]


def all_free(eng):
    r = eng.runner
    return (not r._guide_slots and not r._guide_refs and sorted(r._guide_free) == list(range(eng.cfg.max_num_seqs))
            and all(reg["refs"] == 0 for reg in r._guide_regions.values()))


def test_sampled_rows_match_beside_plain_and_csr_rows():
    eng = byte_engine(max_num_seqs=8, budget=256)
    table = eng.token_bytes
    sps = [SamplingParams(max_tokens=16, ignore_eos=True),
           SamplingParams(max_tokens=16, guided_regex=PATTERN, temperature=1.0, seed=1),
           SamplingParams(max_tokens=16, guided_choice=[[700, 701, 702], [700, 705]]),
           SamplingParams(max_tokens=16, guided_regex=PATTERN, temperature=1.0, seed=2, repetition_penalty=1.2),
           SamplingParams(max_tokens=16, guided_regex=PATTERN),
           SamplingParams(max_tokens=16, allowed_token_ids=[9, 10], ignore_eos=True)]
    ps = prompts(len(sps), seed=1)
    seqs = run(eng, ps, sps)
    for i in (1, 3, 4):
        s = seqs[i]
        assert s.output_ids[-1] == EOS and s.finish_reason == "stop", s.output_ids
        assert re.fullmatch(PATTERN.encode(), oracle.spell(table, s.output_ids[:-1])), s.output_ids
    assert seqs[2].output_ids in ([700, 701, 702, EOS], [700, 705, EOS])
    assert set(seqs[5].output_ids) <= {9, 10} and len(seqs[5].output_ids) == 16
    st = eng.get_stats()
    assert st["byte_guide_launches"] == st["token_guide_launches"] > 0 and st.get("guide_errors", 0) == 0
    r = eng.runner
    kinds = sorted("st" in reg for reg in r._guide_regions.values())
    assert kinds == [False, False, True]                    # one byte region shared by three rows, two CSR regions
    assert r.guide_arena_states_used() == next(reg["auto"].n_states for reg in r._guide_regions.values() if "st" in reg)
    assert all_free(eng)
    # the plain row is what it is without any guided neighbour
    alone = make_engine(max_num_seqs=8, budget=256)
    assert alone.generate([ps[0]], SamplingParams(max_tokens=16))[0] == seqs[0].output_ids
    assert alone.get_stats()["byte_guide_launches"] == 0 and alone.runner.d_bguide is None


def test_a_pattern_over_the_edge_cap_is_admitted_and_matches():
    eng = byte_engine()
    guide = eng._compile_guide(SamplingParams(guided_regex=WIDE))
    assert isinstance(guide, ByteGuide) and guide.n_states == 201
    s = run(eng, prompts(1), [SamplingParams(max_tokens=12, guided_regex=WIDE, temperature=1.0, seed=3)])[0]
    body = s.output_ids[:-1] if s.output_ids[-1] == EOS else s.output_ids
    assert re.fullmatch(WIDE.encode(), oracle.spell(eng.token_bytes, body)), s.output_ids
    assert len(oracle.spell(eng.token_bytes, body)) > 0 or s.output_ids == [EOS]
    assert all_free(eng)


def test_a_preempted_and_recomputed_row_continues_legally():
    ps = [p[:40] for p in prompts(4, seed=3)]
    pattern = r"([a-d]\d){14}x"                              # 29 bytes: up to 29 tokens and EOS
    eng = byte_engine(blocks=12, max_num_seqs=4, budget=256, prefix=False)
    table = [b if b is None or len(b) == 1 else None for b in eng.token_bytes]
    table[1000] = b"a1"                                      # one multi-byte token keeps the table multi-byte; the
    eng.token_bytes = table                                  # rows stay long enough to run out of KV blocks
    sps = [SamplingParams(max_tokens=30, guided_regex=pattern, temperature=1.0, seed=s) for s in range(4)]
    seqs = run(eng, ps, sps)
    assert eng.scheduler.num_preemptions > 0
    for s in seqs:
        assert s.output_ids[-1] == EOS and re.fullmatch(pattern.encode(), oracle.spell(table, s.output_ids[:-1]))
    assert all_free(eng)


def test_the_state_arena_fills_frees_and_shares(monkeypatch):
    monkeypatch.setattr(ops, "GUIDE_BYTE_STATE_ARENA", 24)   # read when the runner allocates its tables
    eng = byte_engine(max_num_seqs=8)
    pats = [r"%s{9}" % c for c in "abcd"]                    # 10 states each
    p = prompts(1)[0]
    for pat in pats[:2]:
        eng.add_request(f"a-{pat}", p, SamplingParams(max_tokens=4, guided_regex=pat))
    eng.add_request("a-again", p, SamplingParams(max_tokens=4, guided_regex=pats[0]))     # shares a region
    assert eng.runner.guide_arena_states_used() == 20
    with pytest.raises(ValueError, match="arena is full"):
        eng.add_request("a-full", p, SamplingParams(max_tokens=4, guided_regex=pats[2]))
    while eng.has_work():
        eng.step()
    assert all_free(eng) and eng.runner.guide_arena_states_used() == 20      # kept until their room is needed
    eng.add_request("a-evicts", p, SamplingParams(max_tokens=4, guided_regex=pats[3]))
    assert eng.runner.guide_arena_states_used() == 20
    while eng.has_work():
        eng.step()
    assert all_free(eng)


def test_serving_a_text_request_with_a_trained_bpe_tokenizer(tmp_path):
    tok = bytelevel_tokenizer()
    tok.save_pretrained(str(tmp_path))
    cfg = ModelConfig(model_name="mini", model_path=str(tmp_path), arch="llama", preset="llama-mini", max_batch_size=4,
                      max_model_len=256, max_num_batched_tokens=128, num_kv_blocks=128, use_cuda_graph=False,
                      max_latency_ms=1.0, overrides={"device": "cpu"})
    backend = LLMBackend(cfg)
    try:
        assert type(backend.tokenizer).__name__ != "ByteTokenizer" and backend.engine.token_bytes is not None
        assert backend.engine.eos_token_id == tok.eos_token_id
        pattern = r"[a-z]{2,6} \d{1,3}"

        async def main():
            out = await backend.predict({"prompt": "hello there", "max_tokens": 24, "guided_regex": pattern,
                                         "temperature": 1.0, "seed": 4})
            with pytest.raises(ValueError, match="single-byte token"):
                # the trainer's alphabet has every byte: drop one from the engine's table to meet the refusal
                table = list(backend.engine.token_bytes)
                table[table.index(b"7")] = None
                backend.engine.token_bytes = table
                await backend.predict({"prompt": "hello", "max_tokens": 8, "guided_regex": r"\d+"})
            return out

        out = asyncio.run(main())
        assert out["finish_reason"] == "stop" and out["token_ids"][-1] == tok.eos_token_id
        assert re.fullmatch(pattern, out["text"].replace(tok.eos_token, "")), out["text"]
        assert re.fullmatch(pattern, tok.decode(out["token_ids"][:-1]))
        assert backend.engine.get_stats()["byte_guide_launches"] > 0
    finally:
        backend.close()
