"""Per-token logprobs off the GPU: the request surface, the reference op's tie order, the CPU engine end to end
(alignment, streaming, preemption, prompt logprobs), the disaggregation packet, and the OpenAI gateway's layouts."""

import asyncio
import json
import math
import types

import aiohttp
import pytest
import torch
from aiohttp import web

from src.client import InferenceClient
from src.coordinator import Coordinator
from src.engine.disagg import sampling_to_dict
from src.http_server import Gateway, render_logprobs
from src.ops import reference as ref
from src.parallel.kv_transfer import KVPacket, packet_from_wire, packet_meta, packet_to_wire
from src.postproc import LOGPROB_FLOOR, logprobs_block
from src.preproc import SamplingParams, normalize_request
from src.worker import Worker

from tests.logprobs_reference import all_rows_logits
from tests.test_engine_cpu import make_engine, prompts
from tests.test_http_gateway_cpu import llm_cfg


# ------------------------------------------------------------------ request surface
def test_sampling_params_validation():
    assert SamplingParams().logprobs is None and SamplingParams().prompt_logprobs is None
    assert SamplingParams(logprobs=0).logprobs == 0 and SamplingParams(prompt_logprobs=20).prompt_logprobs == 20
    for bad in (-1, 21, 1.5, True, "3"):
        with pytest.raises(ValueError):
            SamplingParams(logprobs=bad)
        with pytest.raises(ValueError):
            SamplingParams(prompt_logprobs=bad)


def test_normalize_request_and_disagg_dict_carry_the_fields():
    gi = normalize_request({"prompt_token_ids": [5, 6, 7], "logprobs": 4, "prompt_logprobs": 0})
    assert gi.sampling.logprobs == 4 and gi.sampling.prompt_logprobs == 0
    assert normalize_request({"prompt_token_ids": [5]}).sampling.logprobs is None
    with pytest.raises(ValueError):
        normalize_request({"prompt_token_ids": [5], "logprobs": 21})
    d = sampling_to_dict(gi.sampling)
    assert d["logprobs"] == 4 and d["prompt_logprobs"] == 0
    assert SamplingParams(**d) == gi.sampling


# ------------------------------------------------------------------ the reference op
def test_reference_tie_order_on_integer_rows():
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-3, 4, (4, 1000), generator=g).to(torch.bfloat16)
    t = torch.tensor([0, 999, 1000, -1])
    lp, rank, top_lp, top_id = ref.token_logprobs(x, t, 20)
    lsm = torch.log_softmax(x.double(), -1)
    for r in range(4):
        # larger logit first, then lower id: the first 20 ids holding the maximum, ascending
        assert torch.equal(top_id[r].long(), (x[r].float() == 3).nonzero()[:20, 0])
        assert torch.allclose(top_lp[r].double(), lsm[r, top_id[r].long()], atol=1e-6)
    for r in (0, 1):
        z, i = x[r].float(), int(t[r])
        assert int(rank[r]) == int((z > z[i]).sum() + (z[:i] == z[i]).sum())
        assert abs(float(lp[r]) - float(lsm[r, i])) < 1e-6
    assert lp[2] == -math.inf and rank[2] == 1000 and lp[3] == -math.inf and rank[3] == 1000
    assert ref.token_logprobs(x, t, 0)[2].shape == (4, 0)
    with pytest.raises(ValueError):
        ref.token_logprobs(x, t, 21)


# ------------------------------------------------------------------ the CPU engine
def run(eng, ps, sps, on_token=None):
    done = {}
    for i, (p, sp) in enumerate(zip(ps, sps)):
        eng.add_request(f"r{i}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s), on_token=on_token)
    while eng.has_work():
        eng.step()
    return [done[i] for i in range(len(ps))]


def check_greedy_entries(seq, n):
    assert len(seq.output_logprobs) == len(seq.output_ids)
    for tok, e in zip(seq.output_ids, seq.output_logprobs):
        assert e["rank"] == 0 and e["logprob"] <= 0.0
        assert len(e["top_ids"]) == n and len(e["top_logprobs"]) == n
        assert n == 0 or (e["top_ids"][0] == tok and e["top_logprobs"][0] == e["logprob"])
        assert all(a >= b for a, b in zip(e["top_logprobs"], e["top_logprobs"][1:]))
        assert sum(math.exp(v) for v in e["top_logprobs"]) <= 1 + 1e-4


def test_cpu_engine_logprobs_align_with_tokens():
    ps = prompts(5)
    plain = make_engine().generate(ps, SamplingParams(max_tokens=6))
    eng = make_engine()
    before = eng.get_stats()["logprob_launches"]
    sps = [SamplingParams(max_tokens=6, logprobs=(3, None, 0, None, 20)[i]) for i in range(5)]
    seqs = run(eng, ps, sps)
    assert [s.output_ids for s in seqs] == plain          # asking for logprobs changes no token
    for s, sp in zip(seqs, sps):
        if sp.logprobs is None:
            assert s.output_logprobs == []
        else:
            check_greedy_entries(s, sp.logprobs)
    assert eng.get_stats()["logprob_launches"] > before
    # the entries are the raw distribution of an independent no-cache recompute
    s = seqs[0]
    want = torch.log_softmax(all_rows_logits(eng.model, ps[0] + s.output_ids).double(), -1)
    for j, (tok, e) in enumerate(zip(s.output_ids, s.output_logprobs)):
        row = want[len(ps[0]) - 1 + j]
        assert abs(e["logprob"] - float(row[tok])) < 1e-3 and e["top_ids"][0] == int(row.argmax())
    again = run(make_engine(), [ps[0]], [SamplingParams(max_tokens=6, logprobs=3)])[0]
    assert again.output_ids == s.output_ids
    for a, b in zip(again.output_logprobs, s.output_logprobs):   # alone or in a batch
        assert a["top_ids"] == b["top_ids"] and abs(a["logprob"] - b["logprob"]) < 1e-3


def test_cpu_engine_untouched_default():
    eng = make_engine()
    eng.generate(prompts(3), SamplingParams(max_tokens=4))
    assert eng.get_stats()["logprob_launches"] == 0


def test_on_token_gets_the_entry_as_optional_third_argument():
    two, three = [], []
    eng = make_engine()
    run(eng, prompts(1), [SamplingParams(max_tokens=4, logprobs=2)], on_token=lambda s, t: two.append(t))
    s = run(eng, prompts(1), [SamplingParams(max_tokens=4, logprobs=2)],
            on_token=lambda s, t, e=None: three.append((t, e)))[0]
    assert two == s.output_ids
    assert [t for t, _ in three] == s.output_ids and [e for _, e in three] == s.output_logprobs


def test_recompute_preemption_keeps_entries_aligned():
    ps = [p[:40] for p in prompts(4, seed=3)]
    plain = make_engine(blocks=12, max_num_seqs=4, budget=256, prefix=False).generate(ps, SamplingParams(max_tokens=30))
    eng = make_engine(blocks=12, max_num_seqs=4, budget=256, prefix=False)
    seqs = run(eng, ps, [SamplingParams(max_tokens=30, logprobs=2) for _ in ps])
    assert eng.scheduler.num_preemptions > 0
    for s, want in zip(seqs, plain):
        assert s.output_ids == want and len(s.output_ids) == 30
        check_greedy_entries(s, 2)


def test_prompt_logprobs_on_the_cpu_engine():
    eng = make_engine(budget=64)          # a 150-token prompt: three chunks
    p = prompts(1, seed=5)[0]
    p = (p * 4)[:150]
    s = run(eng, [p], [SamplingParams(max_tokens=3, prompt_logprobs=3)])[0]
    out = s.prompt_logprobs_out
    assert len(out) == 150 and out[0] is None and all(e is not None for e in out[1:])
    # one eager no-cache forward of the whole prompt
    want = torch.log_softmax(all_rows_logits(eng.model, p).double(), -1)
    for pos in (1, 63, 64, 65, 127, 128, 149):     # the chunk boundaries at 64 and 128 among them
        e = out[pos]
        assert abs(e["logprob"] - float(want[pos - 1, p[pos]])) < 1e-3
        assert e["top_ids"][0] == int(want[pos - 1].argmax()) and len(e["top_ids"]) == 3
    hits = eng.stats["prefix_hit_tokens"]
    again = run(eng, [p], [SamplingParams(max_tokens=3, prompt_logprobs=3)])[0]
    assert eng.stats["prefix_hit_tokens"] == hits            # every position computed again
    assert len(again.prompt_logprobs_out) == 150 and again.prompt_logprobs_out[1:] == out[1:]
    assert again.output_ids == s.output_ids


def test_prompt_logprobs_rejected_under_tp_and_on_the_disaggregated_prefill_path():
    eng = make_engine()
    with pytest.raises(ValueError, match="prompt_logprobs"):
        eng.add_request("d", [5, 6, 7], SamplingParams(max_tokens=2, prompt_logprobs=1), export_kv=True)
    eng.model.tp = types.SimpleNamespace(enabled=True)
    with pytest.raises(ValueError, match="prompt_logprobs"):
        eng.add_request("t", [5, 6, 7], SamplingParams(max_tokens=2, prompt_logprobs=1))
    assert not eng.has_work()


# ------------------------------------------------------------------ transport
def test_kv_packet_wire_round_trip_with_first_logprobs():
    first = {"logprob": -0.5, "rank": 0, "top_ids": [9, 4], "top_logprobs": [-0.5, -math.inf]}
    kv = torch.zeros(2, 4, 8, dtype=torch.bfloat16)
    p = KVPacket("r", [1, 2, 3], 9, kv, 16, {"max_tokens": 4, "logprobs": 2}, first_logprobs=first)
    wire = packet_to_wire(p)
    json.dumps({k: v for k, v in wire.items() if k != "kv"})          # valid JSON: -inf was floored
    back = packet_from_wire(wire)
    assert back.first_logprobs == dict(first, top_logprobs=[-0.5, LOGPROB_FLOOR])
    assert packet_meta(p)["first_logprobs"] == back.first_logprobs
    assert packet_from_wire(packet_to_wire(KVPacket("r", [1], 9, kv, 16))).first_logprobs is None


def test_cache_keys_differ_with_and_without_logprobs():
    plain = {"prompt": "hello", "max_tokens": 4}
    keys = {Coordinator._cache_key("m", "1", x) for x in
            (plain, dict(plain, logprobs=0), dict(plain, logprobs=5), dict(plain, prompt_logprobs=5))}
    assert len(keys) == 4


def test_non_finite_values_are_floored_in_outputs():
    blk = logprobs_block([None, {"logprob": -math.inf, "rank": 7, "top_ids": [1, 2],
                                 "top_logprobs": [-0.25, math.nan]}])
    assert blk == {"token_logprobs": [None, LOGPROB_FLOOR], "ranks": [None, 7], "top_token_ids": [None, [1, 2]],
                   "top_logprobs": [None, [-0.25, LOGPROB_FLOOR]]}
    assert LOGPROB_FLOOR == -9999.0
    json.loads(json.dumps(blk, allow_nan=False))
    comp = render_logprobs(dict(blk, tokens=["a", "bc"], top_tokens=[None, ["x", "y"]]), chat=False)
    assert comp["token_logprobs"] == [None, -9999.0] and comp["top_logprobs"] == [None, {"x": -0.25, "y": -9999.0}]
    assert comp["text_offset"] == [0, 1] and comp["tokens"] == ["a", "bc"]


# ------------------------------------------------------------------ worker, coordinator, gateway
async def sse(session, url, body):
    chunks = []
    async with session.post(url, json=body) as r:
        assert r.status == 200
        async for line in r.content:
            line = line.decode().strip()
            if line.startswith("data: ") and line[6:] != "[DONE]":
                chunks.append(json.loads(line[6:]))
    return chunks


def test_gateway_and_streaming_layouts():
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
        client = InferenceClient(f"127.0.0.1:{cport}")
        inp = {"prompt": "hello world", "max_tokens": 6, "ignore_eos": True}
        # RPC: final output and streamed frames
        rpc = (await client.infer("tiny", dict(inp, logprobs=3, prompt_logprobs=1), cache=False))["outputs"]
        plain = (await client.infer("tiny", inp, cache=False))["outputs"]
        assert "logprobs" not in plain and "prompt_logprobs" not in plain
        assert rpc["token_ids"] == plain["token_ids"]
        lp = rpc["logprobs"]
        assert set(lp) == {"token_logprobs", "ranks", "top_token_ids", "top_logprobs", "tokens", "top_tokens"}
        assert all(len(lp[k]) == 6 for k in lp) and lp["ranks"] == [0] * 6
        assert [r[0] for r in lp["top_token_ids"]] == rpc["token_ids"] and all(len(r) == 3 for r in lp["top_tokens"])
        pl = rpc["prompt_logprobs"]
        assert len(pl["token_logprobs"]) == rpc["num_prompt_tokens"] and pl["token_logprobs"][0] is None
        assert pl["top_token_ids"][0] is None and all(len(r) == 1 for r in pl["top_token_ids"][1:])
        ids_only = (await client.infer("tiny", dict(inp, logprobs=0, return_text=False), cache=False))["outputs"]
        assert set(ids_only["logprobs"]) == {"token_logprobs", "ranks", "top_token_ids", "top_logprobs"}
        assert ids_only["logprobs"]["token_logprobs"] == lp["token_logprobs"]
        toks, vals = [], []
        async for frame in client.infer_stream("tiny", dict(inp, logprobs=3)):
            if frame.get("done") is False:
                d = frame["delta_logprobs"]
                assert len(d["token_logprobs"]) == len(frame["delta_token_ids"]) == len(d["tokens"])
                assert [r[0] for r in d["top_token_ids"]] == frame["delta_token_ids"]
                toks += frame["delta_token_ids"]
                vals += d["token_logprobs"]
        assert toks == rpc["token_ids"] and vals == lp["token_logprobs"]
        async for frame in client.infer_stream("tiny", inp):
            assert "delta_logprobs" not in frame
        async with aiohttp.ClientSession() as s:
            body = dict(inp, model="tiny")
            async with s.post(base + "/v1/completions", json=body) as r:
                assert (await r.json())["choices"][0]["logprobs"] is None
            async with s.post(base + "/v1/completions", json=dict(body, logprobs=3, echo=True)) as r:
                assert r.status == 200
                ch = (await r.json())["choices"][0]
            c = ch["logprobs"]
            assert set(c) == {"tokens", "token_logprobs", "top_logprobs", "text_offset", "top_token_ids"}
            assert c["token_logprobs"] == lp["token_logprobs"] and c["tokens"] == lp["tokens"]
            assert c["top_token_ids"] == lp["top_token_ids"] and c["text_offset"][0] == 0
            for i, d in enumerate(c["top_logprobs"]):
                assert 1 <= len(d) <= 3 and d[lp["top_tokens"][i][0]] == lp["token_logprobs"][i]
            assert ch["prompt_logprobs"]["token_logprobs"][0] is None
            assert len(ch["prompt_logprobs"]["tokens"]) == rpc["num_prompt_tokens"]
            chat = {"model": "tiny", "messages": [{"role": "user", "content": "hi"}], "max_tokens": 4,
                    "ignore_eos": True}
            async with s.post(base + "/v1/chat/completions", json=dict(chat, logprobs=True, top_logprobs=2)) as r:
                assert r.status == 200
                cc = (await r.json())["choices"][0]
            content = cc["logprobs"]["content"]
            assert len(content) == 4
            for e in content:
                assert set(e) == {"token", "logprob", "bytes", "top_logprobs"} and len(e["top_logprobs"]) == 2
                assert e["bytes"] == list(e["token"].encode()) and e["top_logprobs"][0]["logprob"] == e["logprob"]
                assert set(e["top_logprobs"][0]) == {"token", "logprob", "bytes"}
            async with s.post(base + "/v1/chat/completions", json=dict(chat, logprobs=True)) as r:
                assert [e["top_logprobs"] for e in (await r.json())["choices"][0]["logprobs"]["content"]] == [[]] * 4
            async with s.post(base + "/v1/chat/completions", json=chat) as r:
                assert (await r.json())["choices"][0]["logprobs"] is None
            # server-sent events: the same layouts for each delta
            chunks = await sse(s, base + "/v1/completions", dict(body, logprobs=3, stream=True))
            got = [v for ck in chunks for v in ((ck["choices"][0].get("logprobs") or {}).get("token_logprobs") or [])]
            assert got == lp["token_logprobs"]
            for ck in chunks:
                ch0 = ck["choices"][0]
                if ch0["token_ids"]:
                    assert len(ch0["logprobs"]["tokens"]) == len(ch0["token_ids"])
            chunks = await sse(s, base + "/v1/chat/completions", dict(chat, logprobs=True, top_logprobs=2, stream=True))
            got = [e["logprob"] for ck in chunks for e in ((ck["choices"][0].get("logprobs") or {}).get("content") or [])]
            assert got == [e["logprob"] for e in content]
            chunks = await sse(s, base + "/v1/completions", dict(body, stream=True))
            assert all(ck["choices"][0].get("logprobs") is None for ck in chunks)
            # out of range: 400
            for bad in (dict(body, logprobs=21), dict(body, logprobs=-1), dict(body, logprobs=True)):
                async with s.post(base + "/v1/completions", json=bad) as r:
                    assert r.status == 400
            for bad in (dict(chat, logprobs=True, top_logprobs=21), dict(chat, top_logprobs=2), dict(chat, logprobs=3)):
                async with s.post(base + "/v1/chat/completions", json=bad) as r:
                    assert r.status == 400
        client.close()
        await runner.cleanup()
        await coord.stop()
        await w.shutdown()
    asyncio.run(main())
