"""guided_json from the request surface down to a CPU engine on the host fallback (reference.schema_guide_rows): the
outputs validate or are legal prefixes, a mixed batch gives every row the tokens it gets alone, a preempted row is
rebuilt by guided.walk_schema, the launch counters show that a batch without a schema row never calls the op, the
disaggregation dict carries the field, and the gateway maps response_format {"type": "json_schema"} and refuses what
it must."""

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
from src.preproc import ByteTokenizer, SamplingParams, normalize_request
from src.worker import Worker

from tests import schema_guide_reference as oracle
from tests.test_engine_cpu import make_engine, prompts
from tests.test_http_gateway_cpu import llm_cfg

EOS = 2
TOK = ByteTokenizer(1024)
POINT = {"type": "object", "properties": {"x": {"type": "integer"}, "tag": {"enum": ["a", "b"]}}, "required": ["x"]}
LIST = {"type": "object", "properties": {"v": {"type": "boolean"}, "next": {"anyOf": [{"$ref": "#"}, {"type": "null"}]}},
        "required": ["v", "next"]}
META = {"type": "object", "properties": {"id": {"type": "string", "maxLength": 2}, "meta": {"type": "object"}},
        "required": ["id", "meta"]}


def b(ch: str) -> int:
    return 3 + ord(ch)


def engine(**kw):
    eng = make_engine(**kw)
    eng.eos_token_id = EOS
    eng.token_bytes = guided.byte_table(eng.arch.vocab_size)
    return eng


def run(eng, ps, sps):
    done = {}
    for i, (p, sp) in enumerate(zip(ps, sps)):
        eng.add_request(f"s{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    while eng.has_work():
        eng.step()
    return [done[i] for i in range(len(ps))]


def all_free(eng):
    r = eng.runner
    return (not r._guide_slots and not r._guide_refs and sorted(r._guide_free) == list(range(eng.cfg.max_num_seqs))
            and all(reg["refs"] == 0 for reg in r._guide_regions.values())
            and set(r._guide_lru) == set(r._guide_regions))


def check_output(seq, schema):
    """A finished document parses and validates; one cut off by max_tokens is a prefix the guide still reads."""
    ids = seq.output_ids
    body = bytes(t - 3 for t in (ids[:-1] if ids[-1] == EOS else ids))
    trans, accept = guided.schema_to_pda(schema)
    if ids[-1] == EOS:
        assert seq.finish_reason == "stop"
        assert oracle.validate(json.loads(body.decode("utf-8")), schema), body
        assert oracle.accepts(trans, accept, body)
    else:
        assert seq.finish_reason == "length"
        oracle.text_config(trans, len(trans), body)     # asserts that no byte dies


def test_the_request_surface_carries_the_field():
    sp = normalize_request({"prompt_token_ids": [5, 6], "guided_json": POINT}, TOK).sampling
    assert sp.guided_json == POINT and sp.guided
    wire = sampling_to_dict(sp)
    assert isinstance(wire["guided_json"], str) and SamplingParams(**wire) == sp
    assert list(SamplingParams(**wire).guided_json["properties"]) == ["x", "tag"]      # the declared order travels
    assert sampling_to_dict(SamplingParams())["guided_json"] is None
    with pytest.raises(ValueError, match="at most one"):
        normalize_request({"prompt_token_ids": [5], "guided_json": POINT, "guided_json_object": True}, TOK)
    with pytest.raises(ValueError, match="minimum"):
        normalize_request({"prompt_token_ids": [5], "guided_json": {"type": "integer", "minimum": 1}}, TOK)


def test_engine_refusals():
    eng = engine()
    p = [5, 6, 7]
    sp = SamplingParams(max_tokens=2, guided_json=POINT)
    eng.token_bytes = None
    with pytest.raises(ValueError, match="byte table"):
        eng.add_request("b", p, sp)
    eng.token_bytes = guided.byte_table(eng.arch.vocab_size)
    eng.eos_token_id = None
    with pytest.raises(ValueError, match="end-of-sequence"):
        eng.add_request("e", p, sp)
    eng.eos_token_id = EOS
    eng.runner.supports_token_guide = False                 # as TPModelRunner declares
    with pytest.raises(ValueError, match="guided_json / guided_json_object are not supported on a tensor-parallel engine"):
        eng.add_request("t", p, sp)
    eng.runner.supports_token_guide = True
    eng.add_request("ok", p, sp)
    assert sorted(eng.seqs) == ["ok"]


def test_greedy_and_sampled_outputs_validate_and_share_regions():
    eng = engine(max_num_seqs=8, budget=256)
    schemas = [POINT, LIST, META, POINT, LIST, META]
    sps = [SamplingParams(max_tokens=48, guided_json=s, **({} if i < 3 else {"temperature": 1.0, "seed": i}))
           for i, s in enumerate(schemas)]
    seqs = run(eng, prompts(len(sps), seed=3), sps)
    for seq, s in zip(seqs, schemas):
        check_output(seq, s)
    assert any(s.output_ids[-1] == EOS for s in seqs)
    st = eng.get_stats()
    assert st["schema_guide_launches"] > 0 and st.get("guide_errors", 0) == 0 and all_free(eng)
    regs = list(eng.runner._guide_regions.values())
    assert len(regs) == 3 and all("sg" in r for r in regs)                 # one region per distinct schema
    assert eng.runner._sguide_st.used == sum(r["auto"].n_states for r in regs)
    # the same runs with a logit_bias towards '}' and ']' close early: every one is a complete document
    bias = {str(b("}")): 40.0, str(b('"')): 20.0, str(b("n")): 10.0}
    seqs = run(eng, prompts(3, seed=5), [SamplingParams(max_tokens=64, guided_json=s, logit_bias=bias)
                                         for s in (POINT, LIST, META)])
    for seq, s in zip(seqs, (POINT, LIST, META)):
        check_output(seq, s)
        assert seq.output_ids[-1] == EOS


def test_a_mixed_batch_gives_each_row_its_solo_tokens_and_only_schema_batches_launch_the_op():
    sps = [SamplingParams(max_tokens=20, guided_json=LIST, temperature=1.0, seed=1),
           SamplingParams(max_tokens=20, guided_json_object=True, temperature=1.0, seed=2),
           SamplingParams(max_tokens=20, guided_regex=r"[a-d]{2,5} \d{1,3}", temperature=1.0, seed=3),
           SamplingParams(max_tokens=20, ignore_eos=True),
           SamplingParams(max_tokens=20, guided_json=POINT, logprobs=2)]
    ps = prompts(len(sps), seed=8)
    eng = engine(max_num_seqs=8, budget=256)
    solo = []
    for i, (p, sp) in enumerate(zip(ps, sps)):
        n0 = eng.get_stats()["schema_guide_launches"]
        solo.append(run(eng, [p], [sp])[0])
        moved = eng.get_stats()["schema_guide_launches"] - n0
        assert (moved > 0) == (sp.guided_json is not None), i               # no schema row: the op is never called
    st = eng.get_stats()
    assert st["json_guide_launches"] > 0 and st["byte_guide_launches"] > 0 and st["token_guide_launches"] > 0
    mixed = run(engine(max_num_seqs=8, budget=256), ps, sps)
    for a, m in zip(solo, mixed):
        assert a.output_ids == m.output_ids and a.finish_reason == m.finish_reason
    check_output(mixed[0], LIST)
    check_output(mixed[4], POINT)
    # logprobs of a schema row are those of the masked row: a sampled token is never barred
    assert len(mixed[4].output_logprobs) == len(mixed[4].output_ids)
    for e in mixed[4].output_logprobs:
        assert e["logprob"] > float("-inf")


def test_a_preempted_row_is_rebuilt_from_its_tokens():
    bias = {str(b("{")): 30.0, str(b("t")): 5.0}       # keeps the list nesting: a long document
    sp = SamplingParams(max_tokens=90, guided_json=LIST, logit_bias=bias)
    ps = [p[:40] for p in prompts(3, seed=4)]
    straight = run(engine(max_num_seqs=4, budget=256), ps, [sp] * 3)
    tight = engine(blocks=12, max_num_seqs=4, budget=256, prefix=False)
    seqs = run(tight, ps, [sp] * 3)
    assert tight.scheduler.num_preemptions > 0
    for a, s in zip(straight, seqs):
        assert a.output_ids == s.output_ids
        check_output(s, LIST)
    assert tight.get_stats().get("guide_errors", 0) == 0 and all_free(tight)


def test_gateway_maps_json_schema_and_rejects_bad_values():
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
        body = {"model": "tiny", "prompt": "hello world", "max_tokens": 24, "cache": False}
        chat = {"model": "tiny", "messages": [{"role": "user", "content": "hi"}], "max_tokens": 24, "cache": False}
        fmt = {"type": "json_schema", "json_schema": {"name": "point", "strict": True, "description": "d",
                                                      "schema": POINT}}
        steer = {"logit_bias": {str(b("}")): 90, str(b("1")): 50}}
        launches = lambda: w.models["tiny"].engine.get_stats()["schema_guide_launches"]
        trans, accept = guided.schema_to_pda(POINT)
        async with aiohttp.ClientSession() as s:
            for url, req in (("/v1/completions", body), ("/v1/chat/completions", chat)):
                n0 = launches()
                async with s.post(base + url, json=dict(req, response_format=fmt, **steer)) as r:
                    assert r.status == 200, await r.text()
                    ch = (await r.json())["choices"][0]
                    assert ch["finish_reason"] == "stop" and ch["token_ids"][-1] == EOS
                    text = bytes(t - 3 for t in ch["token_ids"][:-1]).decode("utf-8")
                    assert oracle.validate(json.loads(text), POINT)
                assert launches() > n0
                for spelled in ({"guided_json": POINT}, {"guided_json": json.dumps(POINT)},
                                {"response_format": {"type": "json_schema", "json_schema": {"schema": POINT}}}):
                    async with s.post(base + url, json=dict(req, temperature=1.0, seed=5, **spelled)) as r:
                        assert r.status == 200, await r.text()
                        ids = (await r.json())["choices"][0]["token_ids"]
                        data = bytes(t - 3 for t in (ids[:-1] if ids[-1] == EOS else ids))
                        oracle.text_config(trans, len(trans), data)
                n1 = launches()
                async with s.post(base + url, json=dict(req, response_format={"type": "json_object"})) as r:
                    assert r.status == 200
                assert launches() == n1                      # JSON mode does not launch the schema op
            bads = ({"response_format": {"type": "json_schema"}},
                    {"response_format": {"type": "json_schema", "json_schema": {}}},
                    {"response_format": {"type": "json_schema", "json_schema": "x"}},
                    {"response_format": {"type": "json_schema", "json_schema": {"schema": "x"}}},
                    {"response_format": {"type": "json_schema", "json_schema": {"name": 5, "schema": POINT}}},
                    {"response_format": {"type": "json_schema", "json_schema": {"schema": {"type": "int"}}}},
                    {"response_format": {"type": "json_schema", "json_schema": {"schema": {"oneOf": [{}]}}}},
                    {"response_format": fmt, "guided_json": POINT}, {"response_format": fmt, "guided_regex": "a"},
                    {"response_format": fmt, "allowed_token_ids": [5]}, {"response_format": fmt, "guided_choice": ["a"]},
                    {"response_format": fmt, "guided_json_object": True}, {"response_format": fmt, "ignore_eos": True},
                    {"guided_json": "{"}, {"guided_json": 5}, {"guided_json": [POINT]},
                    {"guided_json": {"type": "object", "properties": {"s": {"$ref": "#"}}, "required": ["s"]}},
                    {"guided_json": POINT, "guided_regex": "a"}, {"guided_json": POINT, "guided_json_object": True},
                    {"guided_json": POINT, "response_format": {"type": "json_object"}})
            for bad in bads:
                for url, req in (("/v1/completions", body), ("/v1/chat/completions", chat)):
                    async with s.post(base + url, json=dict(req, **bad)) as r:
                        assert r.status == 400, bad
                        msg = (await r.json())["error"]["message"]
                    js = (bad.get("response_format") or {}).get("json_schema", 0)
                    if "response_format" in bad and len(bad) == 1 and not (isinstance(js, dict) and
                                                                          isinstance(js.get("schema"), dict)):
                        assert "json_schema" in msg          # a malformed member: the 400 names it
            async with s.post(base + "/v1/completions",
                              json=dict(body, guided_json={"type": "integer", "minimum": 0})) as r:
                assert r.status == 400 and "minimum" in (await r.json())["error"]["message"]
            # an engine whose runner keeps no such state (tensor parallel) refuses: the worker's error is a 400
            w.models["tiny"].engine.runner.supports_token_guide = False
            async with s.post(base + "/v1/completions", json=dict(body, response_format=fmt)) as r:
                assert r.status == 400
                msg = (await r.json())["error"]["message"]
                assert "tensor-parallel" in msg and "guided_json" in msg
            async with s.post(base + "/v1/completions", json=body) as r:
                assert r.status == 200
        await runner.cleanup()
        await coord.stop()
        await w.shutdown()

    asyncio.run(main())
