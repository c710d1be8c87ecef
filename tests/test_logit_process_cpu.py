"""Penalties and logit_bias off the GPU: the request surface, the oracle's hand cases, the CPU engine end to end
(forcing, distinct tokens, agreement with a no-cache recompute, mixed batches, the tensor-parallel refusal) and
the OpenAI gateway."""

import asyncio
import math

import aiohttp
import pytest
import torch
from aiohttp import web

from src.coordinator import Coordinator
from src.engine.disagg import sampling_to_dict
from src.http_server import Gateway
from src.ops import reference as ref
from src.preproc import SamplingParams, normalize_request
from src.worker import Worker

from tests.logit_process_reference import greedy_reference_processed, inv_f32, logit_process
from tests.test_engine_cpu import make_engine, prompts
from tests.test_http_gateway_cpu import llm_cfg


# ------------------------------------------------------------------ request surface
def test_defaults_process_nothing():
    sp = SamplingParams()
    assert (sp.presence_penalty, sp.frequency_penalty, sp.repetition_penalty, sp.logit_bias) == (0.0, 0.0, 1.0, None)
    assert not sp.processes_logits and sp.greedy
    assert not SamplingParams(logit_bias={}).processes_logits
    for kw in ({"presence_penalty": 0.5}, {"frequency_penalty": -1}, {"repetition_penalty": 1.1},
               {"logit_bias": {7: -1.0}}):
        sp = SamplingParams(**kw)
        assert sp.processes_logits and sp.greedy


@pytest.mark.parametrize("name", ["presence_penalty", "frequency_penalty"])
def test_additive_penalty_validation(name):
    assert getattr(SamplingParams(**{name: 2}), name) == 2.0
    assert getattr(SamplingParams(**{name: -2.0}), name) == -2.0
    for bad in (2.01, -2.5, math.nan, math.inf, True, "1", None):
        with pytest.raises(ValueError):
            SamplingParams(**{name: bad})


def test_repetition_penalty_validation():
    assert SamplingParams(repetition_penalty=50).repetition_penalty == 50.0
    assert SamplingParams(repetition_penalty=0.5).processes_logits
    for bad in (0, 0.0, -1.2, math.nan, math.inf, False, "1.1", None):
        with pytest.raises(ValueError):
            SamplingParams(repetition_penalty=bad)


def test_logit_bias_validation():
    sp = SamplingParams(logit_bias={"5": 1, 9: -100, " 12 ": 100.0})
    assert sp.logit_bias == {5: 1.0, 9: -100.0, 12: 100.0}
    assert len(SamplingParams(logit_bias={i: 0.5 for i in range(300)}).logit_bias) == 300
    for bad in ({i: 0.5 for i in range(301)}, {5: 100.5}, {5: -101}, {5: math.nan}, {5: True}, {5: "1"}, {5: None},
                {-1: 1.0}, {"x": 1.0}, {1.5: 1.0}, {True: 1.0}, {"5": 1.0, 5: 2.0}, [5, 1.0], "5"):
        with pytest.raises(ValueError):
            SamplingParams(logit_bias=bad)


def test_normalize_request_round_trip_through_the_disaggregation_dict():
    gi = normalize_request({"prompt_token_ids": [5, 6, 7], "presence_penalty": 0.5, "frequency_penalty": -0.25,
                            "repetition_penalty": 1.3, "logit_bias": {"17": 4, "200": -100}})
    sp = gi.sampling
    assert (sp.presence_penalty, sp.frequency_penalty, sp.repetition_penalty) == (0.5, -0.25, 1.3)
    assert sp.logit_bias == {17: 4.0, 200: -100.0} and sp.processes_logits
    d = sampling_to_dict(sp)
    assert all(isinstance(k, str) for k in d["logit_bias"])     # a JSON / msgpack map needs string keys
    assert SamplingParams(**d) == sp
    plain = normalize_request({"prompt_token_ids": [5]}).sampling
    assert SamplingParams(**sampling_to_dict(plain)) == plain and not plain.processes_logits
    with pytest.raises(ValueError, match="logit_bias"):         # the ByteTokenizer's vocabulary: 128256
        normalize_request({"prompt_token_ids": [5], "logit_bias": {"128256": 1.0}})
    with pytest.raises(ValueError):
        normalize_request({"prompt_token_ids": [5], "presence_penalty": 3})


# ------------------------------------------------------------------ the oracle
def _one(z, in_prompt, count, rp=1.0, freq=0.0, pres=0.0, bias=None):
    args = (torch.tensor([z], dtype=torch.bfloat16), torch.tensor([in_prompt]), torch.tensor([count]), rp, inv_f32(rp),
            freq, pres, None if bias is None else torch.tensor([bias], dtype=torch.float32))
    a, b = logit_process(*args), ref.logit_process(*args)
    assert a.dtype == torch.bfloat16 and torch.equal(a.view(torch.int16), b.view(torch.int16))
    return float(a[0])


def test_oracle_hand_cases():
    # repetition penalty: a positive logit is divided, a negative one multiplied — only for tokens seen
    assert _one(3.0, False, 1, rp=2.0) == 1.5
    assert _one(-3.0, False, 1, rp=2.0) == -6.0
    assert _one(3.0, False, 0, rp=2.0) == 3.0 and _one(-3.0, False, 0, rp=2.0) == -3.0
    # a prompt-only token: the repetition penalty applies, frequency and presence do not
    assert _one(3.0, True, 0, rp=2.0, freq=1.0, pres=0.5) == 1.5
    assert _one(-3.0, True, 0, rp=2.0, freq=1.0, pres=0.5) == -6.0
    # counts 0 / 1 / 3 under frequency and presence
    assert _one(4.0, False, 0, freq=0.5, pres=0.25) == 4.0
    assert _one(4.0, False, 1, freq=0.5, pres=0.25) == 3.25
    assert _one(4.0, False, 3, freq=0.5, pres=0.25) == 2.25
    # the order: bias, repetition, frequency, presence — (1 + 3) / 2 - 3 * 0.5 - 0.25
    assert _one(1.0, True, 3, rp=2.0, freq=0.5, pres=0.25, bias=3.0) == 0.25
    # the sign test is on the biased value: (1 - 3) * 2
    assert _one(1.0, True, 0, rp=2.0, bias=-3.0) == -4.0
    # one rounding, at the end: 1 + 2^-9 is kept in fp32 and only then rounded (to 1.0 in bf16), the count saturates
    assert _one(1.0, False, 0, bias=2.0 ** -9) == 1.0
    assert _one(0.0, False, 40000, freq=1.0) == -32768.0        # 32767 in fp32, rounded to bf16 once
    # inv_rp is fp32(1 / rp), a multiplication: 3 * fp32(1/3) is not 1 in fp32 but rounds to it in bf16
    assert _one(3.0, True, 0, rp=3.0) == 1.0


# ------------------------------------------------------------------ the CPU engine
def run(eng, ps, sps):
    done = {}
    for i, (p, sp) in enumerate(zip(ps, sps)):
        eng.add_request(f"r{i}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    while eng.has_work():
        eng.step()
    return [list(done[i].output_ids) for i in range(len(ps))]


def absent(ps, n, vocab=1024):
    """The n lowest token ids (above the special ones) that occur in none of the prompts; llama-tiny: 1024 ids."""
    used = {t for p in ps for t in p}
    ids = [t for t in range(3, vocab) if t not in used][:n]
    assert len(ids) == n
    return ids


def test_bias_forces_a_token_at_every_step():
    eng = make_engine()
    p = prompts(1)[0]
    out = run(eng, [p], [SamplingParams(max_tokens=10, logit_bias={777: 100})])[0]
    assert out == [777] * 10
    assert eng.get_stats()["logit_process_launches"] >= 10
    assert not eng.runner._pen_slots and len(eng.runner._pen_free) == eng.cfg.max_num_seqs


def test_repetition_penalty_walks_through_the_biased_set():
    eng = make_engine()
    p = prompts(1, seed=1)[0]
    ids = absent([p], 8)
    out = run(eng, [p], [SamplingParams(max_tokens=8, logit_bias={t: 100 for t in ids}, repetition_penalty=50)])[0]
    # +100 puts the eight far above everything else; once generated, a token falls to about 2: never twice
    assert sorted(out) == ids


def test_frequency_penalty_agrees_with_the_no_cache_oracle_loop():
    # the tiny model's logits lie within +-1.5: a small bias ladder makes three tokens compete, so that the
    # counts (0, 1, 2, ...) decide every step; fp32 on the CPU is exact enough for token equality, as in
    # tests/test_engine_cpu.py
    eng = make_engine()
    ps = prompts(3, seed=2)
    n = 10
    a, b, c = absent(ps, 3)
    bias = {a: 6.0, b: 5.0, c: 4.0}
    outs = run(eng, ps, [SamplingParams(max_tokens=n, frequency_penalty=1.5, logit_bias=bias) for _ in ps])
    for p, o in zip(ps, outs):
        want, _ = greedy_reference_processed(eng.model, p, n, freq=1.5, bias=bias)
        assert o == want
        assert len(set(o)) >= 3 and max(o.count(t) for t in set(o)) >= 2       # repeats: counts above 1 were used
    assert run(eng, ps[:1], [SamplingParams(max_tokens=n, logit_bias=bias)])[0] == [a] * n


def test_plain_requests_are_untouched_by_penalised_neighbours():
    ps = prompts(4, seed=3)
    alone = make_engine().generate(ps, SamplingParams(max_tokens=8))
    eng = make_engine()
    sps = [SamplingParams(max_tokens=8), SamplingParams(max_tokens=8, frequency_penalty=2.0, repetition_penalty=1.5),
           SamplingParams(max_tokens=8), SamplingParams(max_tokens=8, logit_bias={5: 100})]
    outs = run(eng, ps, sps)
    assert outs[0] == alone[0] and outs[2] == alone[2]
    assert outs[3] == [5] * 8
    # and an engine that never saw the fields launches nothing and allocates nothing
    plain = make_engine()
    plain.generate(ps, SamplingParams(max_tokens=4))
    assert plain.get_stats()["logit_process_launches"] == 0 and plain.runner.d_pen is None


def test_recompute_preemption_keeps_prompt_bits_and_counts():
    ps = [p[:40] for p in prompts(4, seed=3)]
    ids = absent(ps, 30)
    sp = dict(max_tokens=30, logit_bias={t: 100 for t in ids}, repetition_penalty=50)
    eng = make_engine(blocks=12, max_num_seqs=4, budget=256, prefix=False)
    outs = run(eng, ps, [SamplingParams(**sp) for _ in ps])
    assert eng.scheduler.num_preemptions > 0
    for o in outs:   # thirty biased tokens, thirty steps: a recompute that lost the counts would repeat one
        assert sorted(o) == ids
    assert not eng.runner._pen_slots


def test_disaggregated_prefill_and_decode_equal_one_engine():
    """The prefill worker applies the fields to the first token; the decode worker builds its slot from the
    imported lists (the first token is its first decode step's input: counted by that step, not by the build)."""
    from src.engine.async_engine import AsyncLLMEngine
    from src.engine.disagg import DisaggregatedServer
    from tests.test_disagg_cpu import PROMPTS, eng

    ids = absent(PROMPTS, 8)
    sp = dict(max_tokens=8, logit_bias={t: 100 for t in ids}, repetition_penalty=50)
    expect = run(eng(), PROMPTS, [SamplingParams(**sp) for _ in PROMPTS])
    assert all(sorted(o) == ids for o in expect)
    srv = DisaggregatedServer(AsyncLLMEngine(eng()), AsyncLLMEngine(eng()))

    async def main():
        srv.start()
        seqs = await asyncio.wait_for(asyncio.gather(*(srv.generate(p, SamplingParams(**sp)) for p in PROMPTS)), 60)
        srv.stop()
        return seqs

    assert [s.output_ids for s in asyncio.run(main())] == expect


def test_a_runner_without_the_state_refuses():
    eng = make_engine()
    eng.runner.supports_logit_processing = False     # as TPModelRunner declares
    for kw in ({"presence_penalty": 0.1}, {"frequency_penalty": 0.1}, {"repetition_penalty": 1.1},
               {"logit_bias": {5: 1.0}}):
        with pytest.raises(ValueError, match="tensor-parallel"):
            eng.add_request("t", [5, 6, 7], SamplingParams(max_tokens=2, **kw))
    assert not eng.has_work()
    eng.add_request("ok", [5, 6, 7], SamplingParams(max_tokens=2))    # plain requests still run
    from src.parallel.tp_runner import TPModelRunner
    assert TPModelRunner.supports_logit_processing is False
    with pytest.raises(ValueError, match="logit_bias"):
        make_engine().add_request("b", [5, 6, 7], SamplingParams(max_tokens=2, logit_bias={10 ** 7: 1.0}))


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
        body = {"model": "tiny", "prompt": "hello world", "max_tokens": 6, "ignore_eos": True}
        chat = {"model": "tiny", "messages": [{"role": "user", "content": "hi"}], "max_tokens": 6, "ignore_eos": True}
        eight = {str(t): 100 for t in range(300, 316, 2)}
        async with aiohttp.ClientSession() as s:
            async with s.post(base + "/v1/completions", json=dict(body, logit_bias={"123": 100})) as r:
                assert r.status == 200
                assert (await r.json())["choices"][0]["token_ids"] == [123] * 6
            async with s.post(base + "/v1/chat/completions", json=dict(chat, logit_bias={"123": 100})) as r:
                assert r.status == 200
                assert (await r.json())["choices"][0]["token_ids"] == [123] * 6
            # the penalty reaches the engine: without it the +100 set's best token simply repeats (below)
            async with s.post(base + "/v1/completions", json=dict(body, logit_bias=eight, repetition_penalty=50)) as r:
                assert r.status == 200
                ids = (await r.json())["choices"][0]["token_ids"]
            assert len(set(ids)) == 6 and set(ids) <= {int(t) for t in eight}
            async with s.post(base + "/v1/chat/completions",
                              json=dict(chat, presence_penalty=2, frequency_penalty=-2.0)) as r:
                assert r.status == 200 and len((await r.json())["choices"][0]["token_ids"]) == 6
            async with s.post(base + "/v1/completions", json=dict(body, logit_bias=eight)) as r:
                ids = (await r.json())["choices"][0]["token_ids"]
                assert len(set(ids)) < 6 and set(ids) <= {int(t) for t in eight}
            bads = ({"presence_penalty": 2.5}, {"frequency_penalty": -3}, {"frequency_penalty": "1"},
                    {"repetition_penalty": 0}, {"repetition_penalty": -1}, {"logit_bias": {"5": 101}},
                    {"logit_bias": {"five": 1}}, {"logit_bias": [5, 1]}, {"logit_bias": {str(i): 1 for i in range(301)}})
            for bad in bads:
                async with s.post(base + "/v1/completions", json=dict(body, **bad)) as r:
                    assert r.status == 400, bad
                async with s.post(base + "/v1/chat/completions", json=dict(chat, **bad)) as r:
                    assert r.status == 400, bad
            # an engine whose runner keeps no such state (tensor parallel) refuses: the worker's error is a 400
            w.models["tiny"].engine.runner.supports_logit_processing = False
            async with s.post(base + "/v1/completions", json=dict(body, repetition_penalty=1.5, cache=False)) as r:
                assert r.status == 400 and "tensor-parallel" in (await r.json())["error"]["message"]
            async with s.post(base + "/v1/completions", json=dict(body, cache=False)) as r:
                assert r.status == 200
        await runner.cleanup()
        await coord.stop()
        await w.shutdown()
    asyncio.run(main())
