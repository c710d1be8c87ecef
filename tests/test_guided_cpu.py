"""Constrained decoding off the GPU: the request surface, the host compiler (src/guided.py; Python's re is the
oracle of the regex subset), the CPU reference of ops.token_guide against the numpy oracle bit for bit (corrupted
tables included: those never run on a GPU), the CPU engine end to end and the OpenAI gateway."""

import asyncio
import itertools
import random
import re

import aiohttp
import numpy as np
import pytest
import torch
from aiohttp import web

from src import guided, ops
from src.coordinator import Coordinator
from src.engine.disagg import sampling_to_dict
from src.http_server import Gateway
from src.ops import reference as ref
from src.preproc import ByteTokenizer, SamplingParams, normalize_request
from src.worker import Worker

from tests import token_guide_reference as oracle
from tests.test_engine_cpu import make_engine, prompts
from tests.test_http_gateway_cpu import llm_cfg

EOS = 2
VOCAB = 1024          # llama-tiny
TOK = ByteTokenizer(VOCAB)


def ids(text):
    return TOK.encode(text, add_bos=False)


# ------------------------------------------------------------------ request surface
def test_defaults_guide_nothing():
    sp = SamplingParams()
    assert (sp.allowed_token_ids, sp.guided_choice, sp.guided_regex) == (None, None, None) and not sp.guided
    for kw in ({"allowed_token_ids": [5, 9]}, {"guided_choice": [[5, 6], [7]]}, {"guided_regex": "a+"}):
        assert SamplingParams(**kw).guided


def test_field_validation():
    assert SamplingParams(allowed_token_ids=(9, 5)).allowed_token_ids == [9, 5]
    assert SamplingParams(guided_choice=[[5, 6], [7], [5, 6]]).guided_choice == [[5, 6], [7]]      # duplicates removed
    assert len(SamplingParams(guided_choice=[[i] for i in range(1024)]).guided_choice) == 1024
    bads = ({"allowed_token_ids": []}, {"allowed_token_ids": [5, 5]}, {"allowed_token_ids": [-1]},
            {"allowed_token_ids": [1.5]}, {"allowed_token_ids": [True]}, {"allowed_token_ids": "5"},
            {"allowed_token_ids": 5}, {"guided_choice": []}, {"guided_choice": [[]]}, {"guided_choice": [[5], []]},
            {"guided_choice": [5, 6]}, {"guided_choice": [["a"]]}, {"guided_choice": "yes"},
            {"guided_choice": [[-3]]}, {"guided_choice": [[i] for i in range(1025)]},
            {"guided_choice": [list(range(40000)), list(range(1, 40000))]},                       # > 65,536 tokens
            {"guided_regex": ""}, {"guided_regex": 5}, {"guided_regex": ["a"]},
            {"allowed_token_ids": [5], "guided_regex": "a"}, {"guided_choice": [[5]], "guided_regex": "a"},
            {"allowed_token_ids": [5], "guided_choice": [[5]]},
            {"guided_choice": [[5]], "ignore_eos": True}, {"guided_regex": "a", "ignore_eos": True})
    for bad in bads:
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    assert SamplingParams(allowed_token_ids=[5], ignore_eos=True).guided     # no end-of-sequence logic there


def test_normalize_request_and_the_disaggregation_dict_round_trip():
    gi = normalize_request({"prompt_token_ids": [5, 6], "guided_choice": ["yes", [9, 10], "no", "yes"]}, TOK)
    assert gi.sampling.guided_choice == [ids("yes"), [9, 10], ids("no")] and ids("yes") == [124, 104, 118]
    for kw in ({"allowed_token_ids": [7, 300]}, {"guided_choice": [[5, 6], [7]]}, {"guided_regex": "(ab|cd)+x"}, {}):
        sp = normalize_request(dict({"prompt_token_ids": [5]}, **kw), TOK).sampling
        assert SamplingParams(**sampling_to_dict(sp)) == sp and sp.guided == bool(kw)
    for bad in ({"allowed_token_ids": [VOCAB]}, {"guided_choice": [[5, VOCAB]]}, {"guided_choice": [""]},
                {"guided_regex": "a("}, {"guided_regex": "a", "allowed_token_ids": [4]}):
        with pytest.raises(ValueError):
            normalize_request(dict({"prompt_token_ids": [5]}, **bad), TOK)


# ------------------------------------------------------------------ the compiler
def reachable(a: guided.Automaton):
    seen, stack = {0}, [0]
    while stack:
        for n in a.edges(stack.pop())[1].tolist():
            if n not in seen:
                seen.add(n)
                stack.append(n)
    return seen


def check_form(a: guided.Automaton):
    assert a.row_ptr[0] == 0 and a.row_ptr[-1] == a.n_edges and a.row_ptr.dtype == np.int32
    for s in reachable(a):
        toks, nxt = a.edges(s)
        assert len(toks) >= 1, f"state {s} is a dead end"
        assert (np.diff(toks) > 0).all() and ((0 <= nxt) & (nxt < a.n_states)).all()


def accepts(a: guided.Automaton, tokens) -> bool:
    """The automaton allows `tokens` and then EOS."""
    try:
        s = guided.walk(a, 0, tokens)
    except ValueError:
        return False
    return EOS in a.edges(s)[0].tolist()


PATTERNS = ["ab", "a*", "(ab|cd){4}x", "a+b?", "[a-c]+d", "[^a]b", "a{2,3}", "a{2,}b", ".a", "(a|b)*c", r"\d+|a",
            "a|", "(a*)*b", "[]a]+", "a{0,2}", "(ab)?c", r"[a\-c]+", r"\w\s?", "x(b|c){1,2}", "a.*d", r"[^\d]c*",
            r"\Sb|\Wd"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_regex_dfa_agrees_with_python_re(pattern):
    trans, accept = guided.regex_to_dfa(pattern)
    rng = random.Random(pattern)
    words = ["".join(w) for n in range(6) for w in itertools.product("abcd", repeat=n)]
    words += ["".join(rng.choice("abcdx -1_\n") for _ in range(rng.randrange(1, 12))) for _ in range(300)]
    for w in words:
        assert guided.dfa_accepts(trans, accept, w.encode()) == bool(re.fullmatch(pattern, w)), (pattern, w)
    a = guided.compile_regex(pattern, guided.byte_table(VOCAB), EOS, VOCAB)
    check_form(a)
    for w in words[::7]:
        assert accepts(a, ids(w)) == bool(re.fullmatch(pattern, w)), (pattern, w)


def test_non_ascii_literals_are_their_utf8_bytes():
    a = guided.compile_regex("é+", guided.byte_table(VOCAB), EOS, VOCAB)
    assert accepts(a, ids("éé")) and not accepts(a, ids("é")[:1]) and not accepts(a, ids("e"))


@pytest.mark.parametrize("pattern,pos", [("^a", 0), ("ab$", 2), ("a*?", 2), ("a+?", 2), ("(?i)a", 0), ("(?=a)b", 0),
                                         ("(?<!a)b", 0), (r"(a)\1", 3), (r"a\b", 1), ("a**", 2), ("a{2", 1),
                                         ("[a-", 0), ("(ab", 0), ("ab)", 2), ("*a", 0), (r"\pL", 0), ("[z-a]", 1),
                                         ("(?P<n>a)", 0), ("a{3,2}", 1), ("[[:alpha:]]", 1)])
def test_unsupported_syntax_names_its_position(pattern, pos):
    with pytest.raises(ValueError, match=f"position {pos}$"):
        guided.parse_regex(pattern)
    with pytest.raises(ValueError, match="position"):
        SamplingParams(guided_regex=pattern)


def test_choice_tries_accept_exactly_the_choices():
    choices = [[5, 6, 7], [5, 6], [9], [5, 8, 7], [300, 5]]
    a = guided.compile_choice(choices, EOS, VOCAB)
    check_form(a)
    alphabet = [5, 6, 7, 8, 9, 300]
    for n in range(4):
        for w in itertools.product(alphabet, repeat=n):
            assert accepts(a, list(w)) == (list(w) in choices), w
    sink = guided.walk(a, 0, [9, EOS])
    assert a.edges(sink)[0].tolist() == [EOS] and guided.walk(a, sink, [EOS, EOS]) == sink   # windows run past the end
    one = guided.compile_allowed([9, 3, 700], VOCAB)
    check_form(one)
    assert one.n_states == 1 and one.edges(0)[0].tolist() == [3, 9, 700] and guided.walk(one, 0, [700, 3, 3]) == 0


def test_compile_refusals_and_the_cache():
    table = guided.byte_table(VOCAB)
    sp = SamplingParams
    for kw, eos, tb in (({"allowed_token_ids": [VOCAB]}, EOS, table), ({"guided_choice": [[5, VOCAB + 3]]}, EOS, table),
                        ({"guided_choice": [[5]]}, None, table), ({"guided_regex": "a"}, None, table),
                        ({"guided_regex": "a"}, EOS, None), ({"guided_choice": [[5, EOS]]}, EOS, table),
                        ({"guided_regex": "a{1024}" * 17}, EOS, table),                    # 17,409 states
                        ({"guided_regex": ".{1000}.{1000}.{100}"}, EOS, table),             # 2,102 x 127 edges
                        ({"guided_regex": "a{17000}"}, EOS, table),
                        ({"guided_regex": "\x01"}, EOS, [None] * VOCAB)):                 # matches nothing producible
        with pytest.raises(ValueError):
            guided.compile_guide(sp(**kw), VOCAB, eos, tb)
    with pytest.raises(ValueError, match="states"):                                        # 16,385 trie states
        guided.compile_choice([list(range(3, 3 + 900))] + [[1000 - i] + list(range(3, 800)) for i in range(20)], EOS)
    a = guided.compile_guide(sp(guided_regex="(ab|cd){4}x"), VOCAB, EOS, table)
    assert guided.compile_guide(sp(guided_regex="(ab|cd){4}x"), VOCAB, EOS, table) is a     # the LRU
    b = guided.compile_guide(sp(guided_choice=[[7], [5, 6]]), VOCAB, EOS, table)
    assert guided.compile_guide(sp(guided_choice=[[5, 6], [7], [5, 6]]), VOCAB, EOS, table) is b   # canonical spec
    assert guided.GUIDE_MAX_STATES == ops.GUIDE_MAX_STATES == 16384
    assert guided.GUIDE_MAX_EDGES == ops.GUIDE_MAX_EDGES == 262144


def test_first_fit_free_list():
    ff = guided.FirstFit(100)
    a, b, c = ff.alloc(30), ff.alloc(30), ff.alloc(30)
    assert (a, b, c) == (0, 30, 60) and ff.alloc(20) is None and ff.used == 90
    ff.release(b, 30)
    assert ff.alloc(40) is None and ff.alloc(10) == 30
    ff.release(a, 30)
    ff.release(30, 10)
    ff.release(c, 30)
    assert ff.free == [[0, 100]] and ff.used == 0


# ------------------------------------------------------------------ the reference op against the oracle
def tensors(case, rows, stride):
    vocab = case["vocab"]
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = case["bits"][:rows]
    t = torch.from_numpy(buf.view(np.int16)).view(torch.bfloat16)
    return {"logits": t, "slot": torch.tensor(oracle.ROW_SLOT[:rows], dtype=torch.int32),
            "desc": torch.from_numpy(case["desc"].copy()), "rowptr": torch.from_numpy(case["rowptr"].copy()),
            "edges": torch.from_numpy(case["edges"].copy()), "cur": torch.from_numpy(case["cur"].copy()),
            "err": torch.zeros(oracle.SLOTS, dtype=torch.int32)}


def as_bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("with_lm", [False, True], ids=["no_lm_part", "lm_part"])
@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("vocab", [1024, 8200])
def test_reference_op_equals_the_oracle_bit_for_bit(vocab, rows, with_advance, with_lm):
    case = oracle.build_case(vocab)
    stride = vocab + 8
    want, w_cur, w_err, w_lm = oracle.run_oracle(case, rows, stride, with_advance, with_lm)
    t = tensors(case, rows, stride)
    lm = torch.from_numpy(oracle.start_lm(rows).view(np.int32).copy()) if with_lm else None
    out = ops.token_guide(t["logits"][:, :vocab], t["slot"], t["desc"], t["rowptr"], t["edges"], t["cur"], t["err"],
                          advance_ids=torch.from_numpy(case["advance"][:rows]) if with_advance else None, lm_part=lm)
    assert out.data_ptr() == t["logits"].data_ptr()                       # in place
    assert np.array_equal(as_bits(t["logits"]), want)
    assert np.array_equal(t["cur"].numpy(), w_cur) and np.array_equal(t["err"].numpy(), w_err)
    if with_lm:
        assert np.array_equal(lm.numpy().view(np.uint32), w_lm)
        if rows == 5:
            assert np.array_equal(w_lm[1], oracle.start_lm(5)[1])         # slot -1: candidates left alone
            assert (w_lm[[0, 2, 3, 4], 1:, 1] == oracle.NO_INDEX).all()
    if rows == 5:
        assert np.array_equal(want[1], np.concatenate([case["bits"][1], np.full(8, 0x447A, np.uint16)]))
        assert w_err.tolist() == [0, 0, ops.GUIDE_ERR_NO_EDGE if with_advance else 0, 0, 0, 0, 0]
        assert w_cur.tolist() == ([3, 4, 2, 1, 4, 4, 2] if with_advance else case["cur"].tolist())
        allowed = (want[:, :vocab] != oracle.NINF_BF16).sum(1).tolist()
        n_many = len(case["many"])
        # (row 4 holds one -inf of its own among the allowed entries; row 1 is untouched)
        assert [allowed[0], allowed[2], allowed[3], allowed[4]] == \
            ([2, vocab, n_many, n_many - 1] if with_advance else [1, 2, vocab, n_many - 1])


CORRUPTIONS = {
    "state_base < 0": lambda t: t["desc"].__setitem__((3, 0), -1),
    "n_states = 0": lambda t: t["desc"].__setitem__((3, 1), 0),
    "row pointers beyond the arena": lambda t: t["desc"].__setitem__((3, 1), 2 ** 30),
    "state_base beyond the arena": lambda t: t["desc"].__setitem__((3, 0), 2 ** 31 - 1),
    "edge_base < 0": lambda t: t["desc"].__setitem__((3, 2), -5),
    "edges beyond the arena": lambda t: t["desc"].__setitem__((3, 3), t["edges"].shape[0]),
    "n_edges < 0": lambda t: t["desc"].__setitem__((3, 3), -1),
    "state >= n_states": lambda t: t["cur"].__setitem__(3, 5),
    "state < 0": lambda t: t["cur"].__setitem__(3, -1),
    "row pointer descends": lambda t: t["rowptr"].__setitem__(oracle.STATE_BASE + 1, -1),
    "row pointer beyond n_edges": lambda t: t["rowptr"].__setitem__(oracle.STATE_BASE + 1, 2 ** 30),
    "next state out of range": lambda t: t["edges"].__setitem__((oracle.EDGE_BASE, 1), 5),
    "edge token = vocab": lambda t: t["edges"].__setitem__((oracle.EDGE_BASE + 1, 0), 1024),
    "edge token < 0": lambda t: t["edges"].__setitem__((oracle.EDGE_BASE + 2, 0), -1),
}


@pytest.mark.parametrize("what", sorted(CORRUPTIONS))
def test_corrupted_tables_leave_the_row_untouched_and_set_err(what):
    """Row 0 (slot 3, state 0, advancing over token 7 into state 1) with one table entry broken: reference and
    oracle agree, the row's bytes, the candidates and the state stay, err carries GUIDE_ERR_TABLE."""
    vocab = 1024
    case = oracle.build_case(vocab)
    t = tensors(case, 5, vocab)
    CORRUPTIONS[what](t)
    before, cur0 = as_bits(t["logits"]).copy(), t["cur"].clone()
    o = {k: v.numpy().copy() for k, v in t.items() if k not in ("logits", "slot")}
    o_bits, o_lm = before.copy(), oracle.start_lm(5)
    oracle.token_guide(o_bits, oracle.ROW_SLOT, o["desc"], o["rowptr"], o["edges"], o["cur"], o["err"], vocab,
                       advance=case["advance"], lm=o_lm)
    lm = torch.from_numpy(oracle.start_lm(5).view(np.int32).copy())
    ops.token_guide(t["logits"], t["slot"], t["desc"], t["rowptr"], t["edges"], t["cur"], t["err"],
                    advance_ids=torch.from_numpy(case["advance"]), lm_part=lm)
    assert np.array_equal(as_bits(t["logits"]), o_bits) and np.array_equal(lm.numpy().view(np.uint32), o_lm)
    assert np.array_equal(t["cur"].numpy(), o["cur"]) and np.array_equal(t["err"].numpy(), o["err"])
    assert int(t["err"][3]) & ops.GUIDE_ERR_TABLE and int(t["cur"][3]) == int(cur0[3])
    assert np.array_equal(as_bits(t["logits"])[0], before[0]) and np.array_equal(o_lm[0], oracle.start_lm(5)[0])
    assert not np.array_equal(as_bits(t["logits"])[4], before[4])          # a healthy row was still guided


# ------------------------------------------------------------------ the CPU engine
def guided_engine(**kw):
    eng = make_engine(**kw)
    eng.eos_token_id = EOS
    return eng


def run(eng, ps, sps):
    done = {}
    for i, (p, sp) in enumerate(zip(ps, sps)):
        eng.add_request(f"g{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    while eng.has_work():
        eng.step()
    return [done[i] for i in range(len(ps))]


def all_free(eng):
    r = eng.runner
    return (not r._guide_slots and not r._guide_refs and sorted(r._guide_free) == list(range(eng.cfg.max_num_seqs))
            and all(reg["refs"] == 0 for reg in r._guide_regions.values())
            and set(r._guide_lru) == set(r._guide_regions))


def test_a_single_choice_is_forced_and_stops():
    eng = guided_engine()
    choice = [700, 5, 5, 901, 33, 64, 12]
    s = run(eng, prompts(1), [SamplingParams(max_tokens=32, guided_choice=[choice])])[0]
    assert s.output_ids == choice + [EOS] and s.finish_reason == "stop"
    assert eng.get_stats()["token_guide_launches"] >= len(choice) + 1
    assert eng.get_stats()["guide_arena_edges_used"] == len(choice) + 2 and all_free(eng)


def test_allowed_token_ids_bar_everything_else():
    eng = guided_engine()
    allowed = [17, 400, 999, 3]
    sps = [SamplingParams(max_tokens=12, allowed_token_ids=allowed, temperature=1.0, seed=s) for s in range(3)]
    for s in run(eng, prompts(3, seed=5), sps):
        assert len(s.output_ids) == 12 and set(s.output_ids) <= set(allowed) and s.finish_reason == "length"
    assert all_free(eng)


def test_a_bias_cannot_lift_a_barred_token():
    eng = guided_engine()
    a, b = ids("a")[0], ids("b")[0]
    s = run(eng, prompts(1, seed=1), [SamplingParams(max_tokens=8, guided_regex="ab", logit_bias={b: 100})])[0]
    assert s.output_ids == [a, b, EOS] and s.finish_reason == "stop"


def test_sampled_regex_outputs_fully_match():
    eng = guided_engine()
    pattern = "(ab|cd){4}x"
    sps = [SamplingParams(max_tokens=16, guided_regex=pattern, temperature=1.0, seed=s) for s in range(6)]
    seqs = run(eng, prompts(6, seed=2), sps)
    texts = set()
    for s in seqs:
        assert s.output_ids[-1] == EOS and s.finish_reason == "stop"
        text = TOK.decode(s.output_ids[:-1])
        assert re.fullmatch(pattern, text), text
        texts.add(text)
    assert len(texts) > 1                                   # sampled, not one forced string
    assert len(eng.runner._guide_regions) == 1 and all_free(eng)


def test_plain_neighbours_keep_their_tokens_and_an_engine_that_never_saw_a_guide_allocates_nothing():
    ps = prompts(3, seed=3)
    alone = make_engine().generate(ps, SamplingParams(max_tokens=8))
    eng = guided_engine()
    eng.eos_token_id = None                                 # as `alone`: allowed_token_ids needs no EOS
    sps = [SamplingParams(max_tokens=8), SamplingParams(max_tokens=8, allowed_token_ids=[5, 6]),
           SamplingParams(max_tokens=8)]
    outs = [s.output_ids for s in run(eng, ps, sps)]
    assert outs[0] == alone[0] and outs[2] == alone[2] and set(outs[1]) <= {5, 6}
    plain = make_engine()
    plain.generate(ps, SamplingParams(max_tokens=4))
    assert plain.get_stats()["token_guide_launches"] == 0 and plain.runner.d_guide is None
    assert plain.get_stats()["guide_arena_edges_used"] == 0


def test_a_preempted_and_recomputed_sequence_continues_legally():
    ps = [p[:40] for p in prompts(4, seed=3)]
    pattern = "(ab|cd){14}x"                                # 29 tokens and EOS
    eng = guided_engine(blocks=12, max_num_seqs=4, budget=256, prefix=False)
    sps = [SamplingParams(max_tokens=30, guided_regex=pattern, temperature=1.0, seed=s) for s in range(4)]
    seqs = run(eng, ps, sps)
    assert eng.scheduler.num_preemptions > 0
    for s in seqs:
        assert len(s.output_ids) == 30 and s.output_ids[-1] == EOS
        assert re.fullmatch(pattern, TOK.decode(s.output_ids[:-1]))
    assert all_free(eng)


def test_the_arena_fills_frees_and_shares(monkeypatch):
    monkeypatch.setattr(ops, "GUIDE_EDGE_ARENA", 40)        # read when the runner allocates its tables
    eng = guided_engine(max_num_seqs=8)
    lists = [list(range(100 * k + 3, 100 * k + 19)) for k in range(4)]          # 16 edges each
    p = prompts(1)[0]
    done = []
    for k in (0, 1):
        eng.add_request(f"a{k}", p, SamplingParams(max_tokens=4, allowed_token_ids=lists[k]), on_finish=done.append)
    assert eng.get_stats()["guide_arena_edges_used"] == 32
    with pytest.raises(ValueError, match="arena is full"):
        eng.add_request("a2", p, SamplingParams(max_tokens=4, allowed_token_ids=lists[2]))
    assert "a2" not in eng.seqs and len(eng.seqs) == 2
    while eng.has_work():
        eng.step()
    assert len(done) == 2 and all(set(s.output_ids) <= set(lists[i]) for i, s in enumerate(done)) and all_free(eng)
    # the finished requests' regions stay until their room is needed: the third spec now evicts the oldest
    eight = run(eng, [p] * 8, [SamplingParams(max_tokens=4, allowed_token_ids=lists[2]) for _ in range(8)])
    assert all(set(s.output_ids) <= set(lists[2]) for s in eight)
    assert tuple(lists[0]) not in [k[1] for k in eng.runner._guide_regions]
    assert sum(k[1] == tuple(lists[2]) for k in eng.runner._guide_regions) == 1     # one region for the eight
    assert eng.get_stats()["guide_arena_edges_used"] == 32 and all_free(eng)


def test_engine_refusals():
    eng = guided_engine()
    p = [5, 6, 7]
    for kw in ({"allowed_token_ids": [VOCAB]}, {"guided_choice": [[5, VOCAB]]}, {"guided_choice": [[5, EOS]]}):
        with pytest.raises(ValueError):
            eng.add_request("v", p, SamplingParams(max_tokens=2, **kw))
    eng.token_bytes = None                                  # as LLMBackend leaves it for an HF tokenizer
    with pytest.raises(ValueError, match="byte table"):
        eng.add_request("b", p, SamplingParams(max_tokens=2, guided_regex="a"))
    eng.add_request("c", p, SamplingParams(max_tokens=2, guided_choice=[[9]]))        # choices need no table
    eng.eos_token_id = None
    for kw in ({"guided_choice": [[5]]}, {"guided_regex": "a"}):
        with pytest.raises(ValueError, match="end-of-sequence"):
            eng.add_request("e", p, SamplingParams(max_tokens=2, **kw))
    eng.add_request("a", p, SamplingParams(max_tokens=2, allowed_token_ids=[9]))
    eng.runner.supports_token_guide = False                 # as TPModelRunner declares
    for kw in ({"allowed_token_ids": [5]}, {"guided_choice": [[5]]}, {"guided_regex": "a"}):
        with pytest.raises(ValueError, match="not supported on a tensor-parallel engine"):
            eng.add_request("t", p, SamplingParams(max_tokens=2, **kw))
    eng.add_request("ok", p, SamplingParams(max_tokens=2))
    from src.parallel.tp_runner import TPModelRunner
    assert TPModelRunner.supports_token_guide is False
    assert sorted(eng.seqs) == ["a", "c", "ok"]


def test_a_device_side_error_fails_that_request_only():
    eng = guided_engine()
    ps = [[5, 6, 7], [8, 9, 10]]                            # one prefill step, then decode steps only
    done = {}
    eng.add_request("bad", ps[0], SamplingParams(max_tokens=6, allowed_token_ids=[5, 6]),
                    on_finish=lambda s: done.__setitem__("bad", s))
    eng.add_request("good", ps[1], SamplingParams(max_tokens=6, allowed_token_ids=[8, 9]),
                    on_finish=lambda s: done.__setitem__("good", s))
    eng.step()                                              # prefill: both have slots now
    slot = eng.runner._guide_slots[eng.seqs["bad"].seq_id]
    with torch.inference_mode():                            # the tables are the runner's inference tensors
        eng.runner.d_guide[0][slot, 1] = 0                  # n_states = 0: a table no step may follow
    while eng.has_work():
        eng.step()
    assert done["bad"].finish_reason == "error" and len(done["bad"].output_ids) < 6
    assert done["good"].finish_reason == "length" and set(done["good"].output_ids) <= {8, 9}
    assert eng.get_stats()["guide_errors"] == 1 and all_free(eng)


# ------------------------------------------------------------------ worker, coordinator, gateway
def test_gateway_passes_the_fields_and_rejects_bad_values():
    async def main():
        w = Worker("h0", host="127.0.0.1", install_signal_handlers=False)
        assert w.load_model(llm_cfg())
        wport = await w.start()
        coord = Coordinator(port=0, max_batch_size=4, max_latency_ms=2)
        cport = await coord.start()
        await coord.add_static_worker(f"127.0.0.1:{wport}")
        runner = web.AppRunner(Gateway(f"127.0.0.1:{cport}").app())
        await runner.setup()
        site = web.TCPSite(runner, "127.0.0.1", 0)
        await site.start()
        base = f"http://127.0.0.1:{site._server.sockets[0].getsockname()[1]}"
        body = {"model": "tiny", "prompt": "hello world", "max_tokens": 12, "cache": False}
        chat = {"model": "tiny", "messages": [{"role": "user", "content": "hi"}], "max_tokens": 12, "cache": False}
        async with aiohttp.ClientSession() as s:
            async with s.post(base + "/v1/completions", json=dict(body, guided_choice=["yes", "no"])) as r:
                assert r.status == 200
                ch = (await r.json())["choices"][0]
                assert ch["token_ids"] in (ids("yes") + [EOS], ids("no") + [EOS]) and ch["finish_reason"] == "stop"
                assert ch["text"] in ("yes", "no")
            async with s.post(base + "/v1/chat/completions",
                              json=dict(chat, guided_regex="(ab|cd){2}", temperature=1.0, seed=3)) as r:
                assert r.status == 200
                ch = (await r.json())["choices"][0]
                assert re.fullmatch("(ab|cd){2}", TOK.decode(ch["token_ids"][:-1])) and ch["token_ids"][-1] == EOS
            async with s.post(base + "/v1/completions",
                              json=dict(body, allowed_token_ids=[300, 301], ignore_eos=True, logprobs=3)) as r:
                assert r.status == 200
                ch = (await r.json())["choices"][0]
                assert len(ch["token_ids"]) == 12 and set(ch["token_ids"]) <= {300, 301}
                for top in ch["logprobs"]["top_logprobs"]:     # two allowed tokens, the third is barred: -inf
                    assert sorted(top.values())[0] == -9999.0 and len(top) == 3
            bads = ({"allowed_token_ids": []}, {"allowed_token_ids": [5, 5]}, {"allowed_token_ids": "5"},
                    {"guided_choice": []}, {"guided_choice": [""]}, {"guided_choice": [[]]}, {"guided_choice": "yes"},
                    {"guided_regex": "^a"}, {"guided_regex": "a*?"}, {"guided_regex": ""}, {"guided_regex": 7},
                    {"guided_regex": "a", "guided_choice": ["a"]}, {"guided_regex": "a", "ignore_eos": True},
                    {"guided_choice": ["a"], "ignore_eos": True})
            for bad in bads:
                async with s.post(base + "/v1/completions", json=dict(body, **bad)) as r:
                    assert r.status == 400, bad
                async with s.post(base + "/v1/chat/completions", json=dict(chat, **bad)) as r:
                    assert r.status == 400, bad
            # an engine whose runner keeps no such state (tensor parallel) refuses: the worker's error is a 400
            w.models["tiny"].engine.runner.supports_token_guide = False
            async with s.post(base + "/v1/completions", json=dict(body, guided_choice=["yes"])) as r:
                assert r.status == 400 and "tensor-parallel" in (await r.json())["error"]["message"]
            async with s.post(base + "/v1/completions", json=body) as r:
                assert r.status == 200
        await runner.cleanup()
        await coord.stop()
        await w.shutdown()
    asyncio.run(main())
