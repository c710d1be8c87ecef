"""JSON mode (guided_json_object, response_format {"type": "json_object"}) from the request surface down to a CPU
engine: SamplingParams validation, the gateway's mappings and 400s, the engine's refusals, a document steered by
logit_bias through reference.json_guide_rows with and without a preemption in the middle, and a disaggregated import
that resumes mid-document."""

import asyncio
import json
import random

import aiohttp
import pytest
from aiohttp import web

from src import guided
from src.coordinator import Coordinator
from src.engine.disagg import sampling_to_dict
from src.http_server import Gateway
from src.parallel.kv_transfer import KVPacket
from src.preproc import ByteTokenizer, SamplingParams, normalize_request
from src.worker import Worker

from tests import json_guide_reference as oracle
from tests.test_engine_cpu import make_engine, prompts
from tests.test_http_gateway_cpu import llm_cfg

EOS = 2
TOK = ByteTokenizer(1024)


def b(ch: str) -> int:
    return 3 + ord(ch)


# ------------------------------------------------------------------ request surface
def test_the_field_is_validated_and_is_one_of_the_guided_fields():
    assert not SamplingParams().guided_json_object and not SamplingParams().guided
    assert SamplingParams(guided_json_object=True).guided
    assert not SamplingParams(guided_json_object=False).guided
    bads = ({"guided_json_object": 1}, {"guided_json_object": "true"}, {"guided_json_object": None},
            {"guided_json_object": True, "allowed_token_ids": [5]}, {"guided_json_object": True, "guided_choice": [[5]]},
            {"guided_json_object": True, "guided_regex": "a"}, {"guided_json_object": True, "ignore_eos": True},
            {"guided_json_object": True, "pooling": "last"}, {"guided_json_object": True, "pooling": "mean"})
    for bad in bads:
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    SamplingParams(guided_json_object=False, guided_regex="a")          # off: the field takes no part


def test_normalize_request_and_the_disaggregation_dict_carry_it():
    sp = normalize_request({"prompt_token_ids": [5, 6], "guided_json_object": True}, TOK).sampling
    assert sp.guided_json_object is True and sp.guided
    assert SamplingParams(**sampling_to_dict(sp)) == sp
    assert sampling_to_dict(SamplingParams())["guided_json_object"] is False
    with pytest.raises(ValueError):
        normalize_request({"prompt_token_ids": [5], "guided_json_object": True, "guided_regex": "a"}, TOK)


# ------------------------------------------------------------------ compile-time refusals
def test_compile_refusals():
    table = guided.byte_table(1024)
    sp = SamplingParams(guided_json_object=True)
    g = guided.compile_guide(sp, 1024, EOS, table)
    assert isinstance(g, guided.JsonGuide) and g.key[0] == "json_object" and g.eos == EOS
    assert guided.compile_guide(sp, 1024, EOS, table) is g                # the cache
    with pytest.raises(ValueError, match="end-of-sequence"):
        guided.compile_guide(sp, 1024, None, table)
    with pytest.raises(ValueError, match="byte table"):
        guided.compile_guide(sp, 1024, EOS, None)
    # a needed byte without a single-byte token: the error names it
    for ch in ('"', "}", "7", "\\"):
        short = list(table)
        short[b(ch)] = None
        with pytest.raises(ValueError, match="0x%02X" % ord(ch)):
            guided.compile_guide(sp, 1024, EOS, short)
    # a byte only EOS spells does not count
    only_eos = list(table)
    only_eos[b("{")] = None
    only_eos[EOS] = b"{"
    with pytest.raises(ValueError, match="0x7B"):
        guided.compile_guide(sp, 1024, EOS, only_eos)
    # a control byte is on no transition: it is not needed
    no_ctl = list(table)
    no_ctl[3 + 0x0A] = None
    assert isinstance(guided.compile_guide(sp, 1024, EOS, no_ctl), guided.JsonGuide)


def json_engine(**kw):
    eng = make_engine(**kw)
    eng.eos_token_id = EOS
    eng.token_bytes = guided.byte_table(eng.arch.vocab_size)
    return eng


def test_engine_refusals():
    eng = json_engine()
    p = [5, 6, 7]
    sp = SamplingParams(max_tokens=2, guided_json_object=True)
    eng.token_bytes = None
    with pytest.raises(ValueError, match="byte table"):
        eng.add_request("b", p, sp)
    eng.token_bytes = guided.byte_table(eng.arch.vocab_size)
    eng.eos_token_id = None
    with pytest.raises(ValueError, match="end-of-sequence"):
        eng.add_request("e", p, sp)
    eng.eos_token_id = EOS
    eng.runner.supports_token_guide = False                 # as TPModelRunner declares
    with pytest.raises(ValueError, match="guided_json_object are not supported on a tensor-parallel engine"):
        eng.add_request("t", p, sp)
    eng.runner.supports_token_guide = True
    eng.add_request("ok", p, sp)
    assert sorted(eng.seqs) == ["ok"]


# ------------------------------------------------------------------ a CPU engine, steered
MINI_VOCAB = 32000
MINI_TABLE = oracle.engine_table(MINI_VOCAB)
KEY, ZERO, CLOSE = oracle.ENGINE_KEY, b("0"), b("}")
BIAS = {KEY: 100.0, ZERO: 60.0, CLOSE: 30.0}     # ranks '{"k":' above '0' above '}', far above any logit


def steered_ids(table=MINI_TABLE, bias=BIAS, eos=EOS, limit=200):
    """The recogniser simulating "the highest-biased allowed token": what a steered request must generate."""
    order = sorted(bias, key=lambda t: -bias[t])
    cfg, out = oracle.START, []
    while len(out) < limit:
        if cfg[0] == "done":
            return out + [eos]
        tok = next(t for t in order if oracle.token_feed(cfg, t, table) is not None)
        out.append(tok)
        cfg = oracle.token_feed(cfg, tok, table)
    raise AssertionError("the steered document does not end")


def mini_engine(**kw):
    eng = make_engine(preset="llama-mini", **kw)
    eng.eos_token_id = EOS
    eng.token_bytes = MINI_TABLE
    return eng


def run(eng, ps, sps):
    done = {}
    for i, (p, sp) in enumerate(zip(ps, sps)):
        eng.add_request(f"j{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    while eng.has_work():
        eng.step()
    return [done[i] for i in range(len(ps))]


def all_free(eng):
    r = eng.runner
    return (not r._guide_slots and not r._guide_refs and sorted(r._guide_free) == list(range(eng.cfg.max_num_seqs))
            and all(reg["refs"] == 0 for reg in r._guide_regions.values())
            and set(r._guide_lru) == set(r._guide_regions))


def test_the_steered_document_reaches_the_cap_and_closes():
    want = steered_ids()
    assert want == [KEY] * 32 + [ZERO] + [CLOSE] * 32 + [EOS] and len(want) == 66
    doc = json.loads(oracle.spell(MINI_TABLE, want[:-1]))
    depth = 0
    while isinstance(doc, dict):
        doc, depth = doc["k"], depth + 1
    assert depth == 32 and doc == 0


def test_a_steered_run_straight_and_with_a_preemption_gives_the_same_tokens():
    want = steered_ids()
    sp = SamplingParams(max_tokens=80, guided_json_object=True, logit_bias=BIAS)
    ps = [p[:40] for p in prompts(3, seed=4)]
    straight = mini_engine(max_num_seqs=4, budget=256)
    a = run(straight, ps[:1], [sp])[0]
    assert a.output_ids == want and a.finish_reason == "stop"
    st = straight.get_stats()
    assert st["json_guide_launches"] > 0 and st.get("guide_errors", 0) == 0 and all_free(straight)
    regs = list(straight.runner._guide_regions.values())
    assert len(regs) == 1 and "js" in regs[0] and "st" not in regs[0] and "rp" not in regs[0]
    assert straight.runner.guide_arena_states_used() == 0 and straight.get_stats()["guide_arena_edges_used"] == 0
    # three such rows in 12 KV blocks: someone is preempted mid-document and recomputed
    tight = mini_engine(blocks=12, max_num_seqs=4, budget=256, prefix=False)
    seqs = run(tight, ps, [sp] * 3)
    assert tight.scheduler.num_preemptions > 0
    for s in seqs:
        assert s.output_ids == want and s.finish_reason == "stop"
    assert tight.get_stats().get("guide_errors", 0) == 0 and all_free(tight)


def test_sampled_rows_are_legal_prefixes_beside_other_guides():
    eng = mini_engine(max_num_seqs=8, budget=256)
    sps = [SamplingParams(max_tokens=24, guided_json_object=True, temperature=1.0, seed=1),
           SamplingParams(max_tokens=24, ignore_eos=True),
           SamplingParams(max_tokens=24, guided_json_object=True, temperature=1.0, seed=2, repetition_penalty=1.2),
           SamplingParams(max_tokens=24, guided_regex=r"[a-d]{2,5} \d{1,3}", temperature=1.0, seed=3),
           SamplingParams(max_tokens=24, guided_choice=[[700, 701], [705]]),
           SamplingParams(max_tokens=24, guided_json_object=True, logprobs=2)]
    ps = prompts(len(sps), seed=6)
    seqs = run(eng, ps, sps)
    for i in (0, 2, 5):
        ids = seqs[i].output_ids
        body = ids[:-1] if ids[-1] == EOS else ids
        assert EOS not in body and oracle.accepts_prefix(oracle.spell(MINI_TABLE, body)), ids
        if ids[-1] == EOS:
            assert isinstance(json.loads(oracle.spell(MINI_TABLE, body)), dict) and seqs[i].finish_reason == "stop"
    for e in seqs[5].output_logprobs:                       # the logprobs of the masked row
        assert e["logprob"] > float("-inf")
    assert seqs[4].output_ids in ([700, 701, EOS], [705, EOS])
    st = eng.get_stats()
    # ops.json_guide is launched only in steps that hold a JSON row, the other two in every guided step
    assert 0 < st["json_guide_launches"] <= st["byte_guide_launches"] == st["token_guide_launches"]
    assert st.get("guide_errors", 0) == 0 and all_free(eng)
    alone = mini_engine(max_num_seqs=8, budget=256)
    assert alone.generate([ps[1]], SamplingParams(max_tokens=24, ignore_eos=True))[0] == seqs[1].output_ids
    assert alone.get_stats()["json_guide_launches"] == 0 and alone.runner.d_jguide is None
    run(alone, ps[3:5], sps[3:5])                           # guided, but nobody in JSON mode: no such launch
    st = alone.get_stats()
    assert st["json_guide_launches"] == 0 and st["byte_guide_launches"] > 0


def test_the_byte_table_cannot_change_under_a_running_json_request():
    eng = mini_engine()
    sp = SamplingParams(max_tokens=4, guided_json_object=True)
    eng.add_request("a", [5, 6, 7], sp)
    eng.token_bytes = list(MINI_TABLE)                       # another table object
    with pytest.raises(ValueError, match="byte table changed"):
        eng.add_request("b", [5, 6, 7], sp)
    while eng.has_work():
        eng.step()
    eng.add_request("c", [5, 6, 7], sp)                      # nobody walks the old one any more
    while eng.has_work():
        eng.step()
    assert all_free(eng)


def test_a_disaggregated_import_resumes_mid_document():
    want = steered_ids()
    sp = SamplingParams(max_tokens=80, guided_json_object=True, logit_bias=BIAS)
    p = prompts(1, seed=7)[0][:40]
    pre = mini_engine(max_num_seqs=4, budget=256)
    got = {}
    pre.add_request("kv", p, SamplingParams(**dict(sampling_to_dict(sp), max_tokens=1)), export_kv=True,
                    on_finish=lambda s: got.setdefault("s", s))
    while pre.has_work():
        pre.step()
    first = got["s"]
    assert first.output_ids == want[:1]                      # '{"k":': the document is open
    dec = mini_engine(max_num_seqs=4, budget=256)
    done = {}
    dec.add_imported(KVPacket("kv", p, first.output_ids[0], first.kv_export, 16, sampling_to_dict(sp)),
                     SamplingParams(**sampling_to_dict(sp)), on_finish=lambda s: done.setdefault("s", s))
    while dec.has_work():
        dec.step()
    assert done["s"].output_ids == want and done["s"].finish_reason == "stop"
    assert dec.get_stats().get("guide_errors", 0) == 0 and all_free(dec) and all_free(pre)
    # a first token the grammar cannot start with: the device reports it at the first step, that request fails
    bad = {}
    dec.add_imported(KVPacket("kv2", p, CLOSE, first.kv_export, 16, sampling_to_dict(sp)),
                     SamplingParams(**dict(sampling_to_dict(sp), max_tokens=8)),
                     on_finish=lambda s: bad.setdefault("s", s))
    while dec.has_work():
        dec.step()
    assert bad["s"].finish_reason == "error" and dec.get_stats()["guide_errors"] == 1 and all_free(dec)


# ------------------------------------------------------------------ worker, coordinator, gateway
def test_gateway_maps_response_format_and_rejects_bad_values():
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
        # '}' is worth more than anything else: the shortest document
        steer = {"logit_bias": {str(b("{")): 100, str(b("}")): 90}}
        launches = lambda: w.models["tiny"].engine.get_stats()["json_guide_launches"]
        async with aiohttp.ClientSession() as s:
            for url, req in (("/v1/completions", body), ("/v1/chat/completions", chat)):
                n0 = launches()
                async with s.post(base + url, json=dict(req, response_format={"type": "json_object"}, **steer)) as r:
                    assert r.status == 200
                    ch = (await r.json())["choices"][0]
                    assert ch["token_ids"] == [b("{"), b("}"), EOS] and ch["finish_reason"] == "stop"
                    text = ch["text"] if "text" in ch else ch["message"]["content"]
                    assert json.loads(text[:2]) == {}
                assert launches() > n0
                async with s.post(base + url, json=dict(req, guided_json_object=True, temperature=1.0, seed=5)) as r:
                    assert r.status == 200
                    ch = (await r.json())["choices"][0]
                    ids = ch["token_ids"]
                    data = bytes(t - 3 for t in (ids[:-1] if ids[-1] == EOS else ids))
                    assert oracle.accepts_prefix(data), data
                    assert ch["finish_reason"] == ("stop" if ids[-1] == EOS else "length")
                n1 = launches()
                async with s.post(base + url, json=dict(req, response_format={"type": "text"})) as r:
                    assert r.status == 200
                assert launches() == n1                      # "text" does nothing
            bads = ({"response_format": {"type": "json_schema", "json_schema": {}}}, {"response_format": {"type": "xml"}},
                    {"response_format": "json_object"}, {"response_format": {}}, {"response_format": {"type": 5}},
                    {"response_format": ["json_object"]},
                    {"response_format": {"type": "json_object"}, "allowed_token_ids": [5]},
                    {"response_format": {"type": "json_object"}, "guided_choice": ["a"]},
                    {"response_format": {"type": "json_object"}, "guided_regex": "a"},
                    {"response_format": {"type": "json_object"}, "ignore_eos": True},
                    {"guided_json_object": "yes"}, {"guided_json_object": True, "guided_regex": "a"})
            for bad in bads:
                for url, req in (("/v1/completions", body), ("/v1/chat/completions", chat)):
                    async with s.post(base + url, json=dict(req, **bad)) as r:
                        assert r.status == 400, bad
                        msg = (await r.json())["error"]["message"]
                    t = bad.get("response_format")
                    if isinstance(t, dict) and t.get("type") in ("json_schema", "xml"):
                        assert t["type"] in msg                  # the 400 names the type
            # an engine whose runner keeps no such state (tensor parallel) refuses: the worker's error is a 400
            w.models["tiny"].engine.runner.supports_token_guide = False
            async with s.post(base + "/v1/completions", json=dict(body, response_format={"type": "json_object"})) as r:
                assert r.status == 400
                msg = (await r.json())["error"]["message"]
                assert "tensor-parallel" in msg and "guided_json_object" in msg
            async with s.post(base + "/v1/completions", json=body) as r:
                assert r.status == 200
        await runner.cleanup()
        await coord.stop()
        await w.shutdown()
    asyncio.run(main())
