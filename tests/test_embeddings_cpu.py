"""Embedding requests (SamplingParams.pooling) on the CPU ops with llama-tiny: the engine's vectors against the
float64 oracle (tests/pool_embed_reference.py) applied to ONE uncached model.forward of the whole prompt — alone,
chunked, in steps shared with generation requests, after a prefix-cache hit, after a recompute preemption — the
refusals, the idle cost, and /v1/embeddings through worker, coordinator and gateway."""

import asyncio
import base64
import random
import struct

import aiohttp
import numpy as np
import pytest
import torch
from aiohttp import web

from src.client import InferenceClient
from src.config import EngineConfig, ModelConfig
from src.coordinator import Coordinator
from src.engine.llm_engine import LLMEngine
from src.http_server import Gateway
from src.models.llama import AttnMetadata
from src.preproc import ByteTokenizer, SamplingParams, normalize_request, request_cost
from src.worker import Worker
from tests import pool_embed_reference as R


def make_engine(tokens=512, blocks=256, seqs=8, prefix=True, **kw):
    cfg = EngineConfig(max_num_seqs=seqs, max_num_batched_tokens=tokens, num_kv_blocks=blocks, max_latency_ms=0.0,
                       block_size=16, enable_prefix_caching=prefix, preemption_mode="recompute", **kw)
    eng = LLMEngine.from_preset("llama-tiny", device="cpu", cfg=cfg, max_model_len=256, capture=False)
    eng.eos_token_id = None
    return eng


@torch.inference_mode()
def uncached_hidden(model, prompt):
    """The final-norm hidden rows [L, H] of one prompt from a single forward over a pool of its own."""
    n = len(prompt)
    nb = -(-n // 16)
    pool = torch.zeros(model.arch.num_layers, 2, nb, model.hkv, 16, model.head_dim, dtype=model.dtype)
    bt = torch.arange(nb, dtype=torch.int32).view(1, nb)
    pos = torch.arange(n)
    meta = AttnMetadata(True, pos.clone(), bt, torch.tensor([n], dtype=torch.int32),
                        torch.tensor([0, n], dtype=torch.int32), n)
    return model.forward(torch.tensor(prompt), pos, meta, pool)


def prompts(n, lo=5, hi=120, seed=0):
    r = random.Random(seed)
    return [[r.randrange(3, 1000) for _ in range(r.randrange(lo, hi))] for _ in range(n)]


def assert_vector(eng, prompt, vec, mode, dims=0, normalize=True):
    rows = uncached_hidden(eng.model, prompt)
    want, tol = R.oracle(rows, mode, dims, normalize), R.tolerance(rows, mode, dims, normalize)
    assert isinstance(vec, np.ndarray) and vec.dtype == np.float32 and vec.shape == want.shape
    err = np.abs(vec.astype(np.float64) - want)
    assert (err <= tol).all(), (mode, len(prompt), float(err.max()), float(tol.max()))


def run(eng, reqs, hook=None):
    """reqs: (prompt, SamplingParams) -> the finished sequences in order."""
    done = {}
    for i, (p, sp) in enumerate(reqs):
        eng.add_request(f"e{i}-{random.random()}", p, sp, on_finish=lambda s, i=i: done.__setitem__(i, s))
    steps = 0
    while eng.has_work():
        eng.step()
        steps += 1
        if hook is not None:
            hook(steps)
    return [done[i] for i in range(len(reqs))]


@pytest.mark.parametrize("mode", ["last", "mean"])
def test_vectors_equal_the_oracle_whole_and_chunked(mode):
    ps = prompts(6, seed=1)
    for tokens in (512, 24):  # every prompt in one step | chunks of at most 24 tokens
        eng = make_engine(tokens=tokens)
        seqs = run(eng, [(p, SamplingParams(pooling=mode)) for p in ps])
        for p, s in zip(ps, seqs):
            assert s.finish_reason == "embed" and s.output_ids == [] and not s.block_table
            assert_vector(eng, p, s.embedding, mode)
            assert abs(float(np.linalg.norm(s.embedding)) - 1.0) < 1e-5
        st = eng.get_stats()
        assert st["pool_embed_launches"] >= 1 and st["generated_tokens"] == 0 and st["steps_decode"] == 0
        if tokens == 24:
            assert st["steps_prefill"] > len(ps)  # it was chunked
        assert not eng.runner._pool_slots and sorted(eng.runner._pool_free) == list(range(8))
    # unnormalised, truncated
    eng = make_engine()
    sp = SamplingParams(pooling=mode, embed_normalize=False, embed_dimensions=64)
    sp2 = SamplingParams(pooling=mode, embed_dimensions=8)
    seqs = run(eng, [(ps[0], sp), (ps[1], sp2), (ps[2], SamplingParams(pooling=mode))])
    assert_vector(eng, ps[0], seqs[0].embedding, mode, 64, False)
    assert_vector(eng, ps[1], seqs[1].embedding, mode, 8, True)
    assert_vector(eng, ps[2], seqs[2].embedding, mode)


def test_steps_shared_with_generation_leave_its_tokens_unchanged():
    ps = prompts(6, seed=2)
    gen = SamplingParams(max_tokens=6, ignore_eos=True)
    eng = make_engine(tokens=64)
    alone = [s.output_ids for s in run(eng, [(p, gen) for p in ps[:3]])]
    eng = make_engine(tokens=64)
    reqs = [(ps[0], gen), (ps[3], SamplingParams(pooling="last")), (ps[1], gen),
            (ps[4], SamplingParams(pooling="mean")), (ps[2], gen), (ps[5], SamplingParams(pooling="last"))]
    seqs = run(eng, reqs)
    assert [seqs[i].output_ids for i in (0, 2, 4)] == alone
    assert_vector(eng, ps[3], seqs[1].embedding, "last")
    assert_vector(eng, ps[4], seqs[3].embedding, "mean")
    assert_vector(eng, ps[5], seqs[5].embedding, "last")
    assert all(seqs[i].embedding is None for i in (0, 2, 4))
    # an embedding request that arrives while the others decode (a mixed step, or one between decode steps)
    eng = make_engine(tokens=64, mixed_batching=True)
    late = []

    def hook(step):
        if step == 3:
            eng.add_request("late", ps[4], SamplingParams(pooling="mean"), on_finish=late.append)
    seqs = run(eng, [(p, gen) for p in ps[:3]], hook)
    assert [s.output_ids for s in seqs] == alone
    assert_vector(eng, ps[4], late[0].embedding, "mean")


def test_last_after_a_prefix_hit_and_mean_without_one():
    r = random.Random(3)
    shared = [r.randrange(3, 1000) for _ in range(64)]
    a, b = shared + [7, 8, 9], shared + [11, 12, 13, 14, 15]
    eng = make_engine()
    run(eng, [(a, SamplingParams(max_tokens=2, ignore_eos=True))])   # publishes the shared blocks
    s_last, = run(eng, [(b, SamplingParams(pooling="last"))])
    assert s_last.num_prefix_hit == 64
    assert_vector(eng, b, s_last.embedding, "last")
    s_mean, = run(eng, [(b, SamplingParams(pooling="mean"))])
    assert s_mean.num_prefix_hit == 0
    assert_vector(eng, b, s_mean.embedding, "mean")
    # an embedding request publishes its prompt blocks like any other
    c = shared + [21, 22]
    s_gen, = run(eng, [(c, SamplingParams(max_tokens=1))])
    assert s_gen.num_prefix_hit == 64


@pytest.mark.parametrize("mode", ["last", "mean"])
def test_recompute_preemption_restarts_cleanly(mode):
    """A chunked embedding request that loses its blocks half way (recompute preemption) starts again at position
    0: mean pooling's partial sums are dropped with its slot and POOL_FIRST clears the new one."""
    p = prompts(1, lo=100, hi=101, seed=4)[0]
    eng = make_engine(tokens=24)
    hit = []

    def hook(step):
        if step == 2:
            seq = next(iter(eng.seqs.values()))
            assert 0 < seq.num_computed < len(p)
            if mode == "mean":
                assert seq.seq_id in eng.runner._pool_slots
            eng.scheduler._preempt(seq)
            eng._release_logit_state(seq, preempted=True)
            assert seq.num_computed == 0 and not eng.runner._pool_slots
            hit.append(seq.num_preemptions)
    s, = run(eng, [(p, SamplingParams(pooling=mode))], hook)
    assert hit == [1] and s.finish_reason == "embed"
    assert_vector(eng, p, s.embedding, mode)
    assert sorted(eng.runner._pool_free) == list(range(8))


def test_refusals():
    for kw in (dict(logprobs=1), dict(prompt_logprobs=0), dict(presence_penalty=0.5), dict(frequency_penalty=0.5),
               dict(repetition_penalty=1.2), dict(logit_bias={5: 1.0}), dict(allowed_token_ids=[5, 6]),
               dict(guided_choice=[[5, 6]]), dict(guided_regex="ab"), dict(pooling="max"), dict(pooling=""),
               dict(embed_dimensions=12), dict(embed_dimensions=0), dict(embed_dimensions=True),
               dict(embed_normalize=1)):
        with pytest.raises(ValueError):
            SamplingParams(**{"pooling": "last", **kw})
    with pytest.raises(ValueError):
        SamplingParams(embed_dimensions=8)  # without pooling
    with pytest.raises(ValueError):
        SamplingParams(max_tokens=0)  # unchanged for everyone else
    tok = ByteTokenizer(1024)
    with pytest.raises(ValueError):
        normalize_request({"prompt": "x", "pooling": "last", "stream": True}, tok)
    # max_tokens does not count against max_model_len
    gi = normalize_request({"prompt_token_ids": list(range(3, 253)), "pooling": "mean", "max_tokens": 100}, tok, 256)
    assert gi.sampling.pooling == "mean"
    with pytest.raises(ValueError):
        normalize_request({"prompt_token_ids": list(range(3, 253)), "max_tokens": 100}, tok, 256)
    assert request_cost({"prompt_token_ids": [1, 2, 3], "pooling": "last"}) == (3, 0)
    assert request_cost({"prompt_token_ids": [1, 2, 3]}) == (3, 16)

    eng = make_engine()
    sp = SamplingParams(pooling="last", max_tokens=200)
    eng.add_request("fits", list(range(3, 253)), sp)  # 250 + 200 > 256: only the prompt has to fit
    with pytest.raises(ValueError, match="max_model_len"):
        eng.add_request("long", list(range(3, 303)), sp)
    with pytest.raises(ValueError, match="pooling is not supported on the disaggregated prefill path"):
        eng.add_request("x", [5, 6, 7], sp, export_kv=True)
    with pytest.raises(ValueError, match="streaming"):
        eng.add_request("s", [5, 6, 7], sp, on_token=lambda s, t: None)
    with pytest.raises(ValueError, match="hidden size"):
        eng.add_request("d", [5, 6, 7], SamplingParams(pooling="last", embed_dimensions=512))

    class FakeTP:
        enabled = True
    real = eng.model.tp
    eng.model.tp = FakeTP()
    try:
        with pytest.raises(ValueError, match="pooling is not supported on a tensor-parallel engine"):
            eng.add_request("tp", [5, 6, 7], sp)
    finally:
        eng.model.tp = real
    assert set(eng.seqs) == {"fits"}


def test_nobody_asks_nothing_is_launched_or_allocated():
    eng = make_engine(tokens=64)
    ps = prompts(4, seed=5)
    run(eng, [(p, SamplingParams(max_tokens=5, ignore_eos=True)) for p in ps])
    assert eng.get_stats()["pool_embed_launches"] == 0
    assert eng.runner.d_pool is None and eng.runner.h_pool is None and not eng.runner._pool_free
    run(eng, [(ps[0], SamplingParams(pooling="last"))])
    assert eng.get_stats()["pool_embed_launches"] == 1 and eng.runner.d_pool is not None
    assert eng.runner.d_pool[0].shape == (8, eng.arch.hidden_size) and eng.runner.d_pool[0].dtype == torch.float32


def llm_cfg():
    return ModelConfig(model_name="tiny", model_path="", arch="llama", preset="llama-tiny", max_batch_size=4,
                       max_model_len=256, max_num_batched_tokens=128, num_kv_blocks=128, use_cuda_graph=False,
                       max_latency_ms=1.0, overrides={"device": "cpu"})


def test_v1_embeddings_through_worker_coordinator_gateway():
    async def main():
        w = Worker("h0", host="127.0.0.1", install_signal_handlers=False)
        assert w.load_model(llm_cfg())
        model = w.models["tiny"].engine.model
        tok = w.models["tiny"].tokenizer
        wport = await w.start()
        coord = Coordinator(port=0, max_batch_size=4, max_latency_ms=2)
        cport = await coord.start()
        await coord.add_static_worker(f"127.0.0.1:{wport}")
        gw = Gateway(f"127.0.0.1:{cport}")
        runner = web.AppRunner(gw.app())
        await runner.setup()
        site = web.TCPSite(runner, "127.0.0.1", 0)
        await site.start()
        base = f"http://127.0.0.1:{site._server.sockets[0].getsockname()[1]}"

        def check(vec, ids, mode="last", dims=0, normalize=True):
            rows = uncached_hidden(model, ids)
            want, tol = R.oracle(rows, mode, dims, normalize), R.tolerance(rows, mode, dims, normalize)
            got = np.asarray(vec, dtype=np.float32).astype(np.float64)
            assert got.shape == want.shape and (np.abs(got - want) <= tol).all()

        texts = ["hello world", "a second, rather longer sentence to embed", "x"]
        async with aiohttp.ClientSession() as s:
            async def post(body, status=200):
                async with s.post(base + "/v1/embeddings", json=body) as r:
                    assert r.status == status, (body, r.status, await r.text())
                    return await r.json()

            one = await post({"model": "tiny", "input": texts[0]})
            assert one["object"] == "list" and one["model"] == "tiny" and len(one["data"]) == 1
            d0 = one["data"][0]
            assert d0["object"] == "embedding" and d0["index"] == 0 and len(d0["embedding"]) == 256
            n0 = len(tok.encode(texts[0]))
            assert one["usage"] == {"prompt_tokens": n0, "total_tokens": n0}
            check(d0["embedding"], tok.encode(texts[0]))

            batch = await post({"model": "tiny", "input": texts, "pooling": "mean"})
            assert [d["index"] for d in batch["data"]] == [0, 1, 2]
            for t, d in zip(texts, batch["data"]):
                check(d["embedding"], tok.encode(t), "mean")
            total = sum(len(tok.encode(t)) for t in texts)
            assert batch["usage"] == {"prompt_tokens": total, "total_tokens": total}

            ids = [5, 77, 300, 12, 999, 4]
            flat = await post({"model": "tiny", "input": ids})
            assert len(flat["data"]) == 1 and flat["usage"]["prompt_tokens"] == 6
            check(flat["data"][0]["embedding"], ids)
            lists = await post({"model": "tiny", "input": [ids, ids[:3]], "dimensions": 64, "normalize": False})
            check(lists["data"][0]["embedding"], ids, dims=64, normalize=False)
            check(lists["data"][1]["embedding"], ids[:3], dims=64, normalize=False)
            assert lists["usage"] == {"prompt_tokens": 9, "total_tokens": 9}

            f = await post({"model": "tiny", "input": texts[:2], "dimensions": 32, "cache": False})
            b = await post({"model": "tiny", "input": texts[:2], "dimensions": 32, "encoding_format": "base64",
                            "cache": False})
            for df, db in zip(f["data"], b["data"]):
                raw = base64.b64decode(db["embedding"])
                assert len(raw) == 4 * 32
                assert list(struct.unpack("<32f", raw)) == [np.float32(v).item() for v in df["embedding"]]

            # the request rides the existing infer op
            rpc = await InferenceClient(f"127.0.0.1:{cport}").infer("tiny", {"prompt": texts[0], "pooling": "last"},
                                                                    cache=False)
            out = rpc["outputs"]
            assert out["finish_reason"] == "embed" and out["prompt_tokens"] == n0 and "text" not in out
            assert out["embedding"] == d0["embedding"]

            for bad in ({"model": "tiny", "input": []}, {"model": "tiny", "input": ""},
                        {"model": "tiny", "input": ["x"] * 2049}, {"model": "tiny", "input": "x", "pooling": "max"},
                        {"model": "tiny", "input": "x", "stream": True}, {"model": "tiny", "input": "x", "dimensions": 12},
                        {"model": "tiny", "input": "x", "encoding_format": "hex"}, {"model": "tiny", "input": [[1], "x", 3]},
                        {"model": "tiny", "input": "x", "dimensions": 512}, {"input": "x"}):
                await post(bad, 400)
            await post({"model": "nope", "input": "x"}, 404)
            # a streamed RPC with pooling is refused by the worker too
            frames = [fr async for fr in InferenceClient(f"127.0.0.1:{cport}").infer_stream(
                "tiny", {"prompt": "x", "pooling": "last"})]
            assert frames and not frames[-1].get("success")

            async with s.get(base + "/metrics") as r:
                m = await r.text()
            assert 'die_http_embedding_requests_total{model="tiny"}' in m
            assert "die_http_embedding_prompt_tokens_total" in m
            assert "die_http_requests_total{" not in m  # the completion families did not count these
        await runner.cleanup()
        await coord.stop()
        await w.shutdown()
    asyncio.run(main())
