"""
HTTP gateway: an OpenAI-style completions API (plus health and Prometheus metrics) in front of the
coordinator's framed-RPC API. It holds no model state — every request becomes one coordinator RPC
(or one streamed RPC), so any number of gateways can front one coordinator.

    python -m src.http_server --coordinator 127.0.0.1:9000 --port 8000

    POST /v1/completions   {"model", "prompt": str | [token ids], "max_tokens", "temperature",
                            "top_p", "top_k", "seed", "stop_token_ids", "ignore_eos", "stream",
                            "logprobs": 0..20, "echo", "presence_penalty", "frequency_penalty" (-2..2),
                            "repetition_penalty" (> 0), "logit_bias": {token id: -100..100}, <= 300 entries,
                            at most one of "allowed_token_ids": [ids], "guided_choice": [str | [ids]],
                            "guided_regex": str, "response_format": {"type": "json_object"} (or
                            "guided_json_object": true), "response_format": {"type": "json_schema",
                            "json_schema": {"name", "schema": {...}}} (or "guided_json": {...})}
                           stream=true answers with server-sent events ("data: {...}" chunks,
                           then "data: [DONE]"), text and token ids per chunk.
                           logprobs=N: choice.logprobs = {"tokens", "token_logprobs", "top_logprobs":
                           [{token: logprob}] (the N most likely), "text_offset", "top_token_ids"}, of the
                           model's raw distribution (before temperature / top-k / top-p); with echo=true the
                           prompt tokens are scored too (choice.prompt_logprobs, same layout, null first)
    POST /v1/chat/completions  {"model", "messages": [{"role", "content"}], same sampling keys}:
                           the messages rendered in the Llama-3 chat layout (header / end-of-turn
                           markers as text) plus an open assistant turn; answers "chat.completion"
                           objects, or "chat.completion.chunk" deltas when streaming.
                           logprobs=true (with top_logprobs 0..20): choice.logprobs = {"content": [{"token",
                           "logprob", "bytes", "top_logprobs": [{"token", "logprob", "bytes"}]}]}
    Stream chunks carry the same logprobs layouts for their delta; a request that does not ask gets
    "logprobs": null; an out-of-range value is a 400. Non-finite logprobs arrive as -9999.0.
    Penalties and logit_bias (both endpoints) rewrite the logits on the GPU before sampling; a bad value is a
    400, and so is a request that sets them on a model served tensor-parallel. With them, logprobs are those
    of the processed distribution (before temperature / top-k / top-p); without them nothing changes.
    Constrained decoding (both endpoints): allowed_token_ids bars every other token at every step, guided_choice
    yields exactly one of its choices and then EOS, guided_regex an output that fully matches the pattern (the
    byte-level subset of src/guided.py) and then EOS — on the byte-level tokenizer and on HuggingFace BPE
    vocabularies alike (ByteLevel BPE, or pieces with byte fallback: every token's bytes are walked through the
    pattern's automaton on the GPU). Barred tokens have logprob -inf (-9999.0 here). A malformed value, two of the
    three at once, unsupported regex syntax, ignore_eos with a choice or a pattern, or any of them on a model
    served tensor-parallel is a 400; so is guided_regex with a tokenizer whose layout is not recognised, or with a
    pattern that needs a byte no single-byte token of the vocabulary spells.
    JSON mode (both endpoints): response_format {"type": "json_object"}, or the plain field guided_json_object:
    true, constrains the output to one JSON object (compact, or with a single space after ',' and ':'; at most 32
    containers deep) followed by EOS: a byte pushdown automaton walked over every token's bytes on the GPU. A
    request cut off by max_tokens returns an incomplete document with finish_reason "length", as OpenAI documents.
    {"type": "text"} does nothing. Any other type is a 400 naming it; so are a malformed
    response_format, json_object next to allowed_token_ids / guided_choice / guided_regex or with ignore_eos, and
    JSON mode on a model served tensor-parallel or with a tokenizer that has no byte table.
    Structured outputs (both endpoints): response_format {"type": "json_schema", "json_schema": {"name": ...,
    "schema": {...}}} ("name" optional, "strict" and "description" accepted and ignored), or the plain field
    guided_json: {...} (or its JSON text), constrains the output to one document valid against the schema, in JSON
    mode's text conventions, followed by EOS: the schema is compiled to a byte pushdown automaton with a stack of
    return states (src/guided_schema.py lists the supported keywords) that the GPU walks over every token's bytes.
    A json_schema member that is missing, is not an object or lacks an object "schema", an unsupported keyword
    (named with its JSON pointer), a schema with a dead end or over the state cap, a second guided field,
    ignore_eos, a model served tensor-parallel or a tokenizer without a byte table is a 400.
    POST /v1/embeddings    {"model", "input": str | [str] | [token ids] | [[token ids]] (<= 2048 items),
                            "encoding_format": "float" | "base64", "dimensions": multiple of 8,
                            "pooling": "last" | "mean", "normalize": bool}
                           One embedding per input item: the pooled final-norm hidden state of the item's tokens
                           ("last", the default: the last token's; "mean": the mean over all tokens), cut to its
                           first "dimensions" components, L2-normalised unless normalize is false. Every item is
                           one infer RPC, all in flight at once, so the worker batches them into shared prefill
                           steps. Answers {"object": "list", "data": [{"object": "embedding", "index",
                           "embedding"}], "model", "usage": {"prompt_tokens", "total_tokens"}}; base64 is the
                           little-endian float32 bytes. A bad value, "stream", or a model served tensor-parallel
                           or with disaggregated prefill is a 400.
    GET  /v1/models        the coordinator's registered models
    GET  /health           200 when the coordinator answers its health RPC
    GET  /metrics          Prometheus text format (requests, errors, latency, tokens)
"""

from __future__ import annotations

import argparse
import asyncio
import base64
import json
import struct
import time
import uuid
from typing import Any, Dict, Optional

from aiohttp import web
from prometheus_client import CollectorRegistry, Counter, Histogram, generate_latest
from prometheus_client.exposition import CONTENT_TYPE_LATEST

from src.client import InferenceClient
from src.preproc import SamplingParams
from src.utils import setup_logging

_LOGIT_PROCESSING = ("presence_penalty", "frequency_penalty", "repetition_penalty", "logit_bias")
_GUIDED = ("allowed_token_ids", "guided_choice", "guided_regex", "guided_json_object", "guided_json")
_SAMPLING = ("max_tokens", "temperature", "top_p", "top_k", "seed", "stop_token_ids", "ignore_eos") + \
    _LOGIT_PROCESSING + _GUIDED
_ROLES = ("system", "user", "assistant", "tool")
MAX_LOGPROBS = 20
MAX_EMBED_INPUTS = 2048  # items of one /v1/embeddings request (the OpenAI API's cap)


def _logprob_count(v: Any, name: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= MAX_LOGPROBS:
        raise ValueError(f"{name} must be an integer in [0, {MAX_LOGPROBS}]")
    return v


def _token_strings(lp: Dict[str, Any]):
    """(tokens, top tokens) of a backend logprobs block: its per-token strings, or the ids as text without them."""
    n = len(lp.get("token_logprobs") or [])
    toks = lp.get("tokens") or [""] * n
    tops = lp.get("top_tokens") or [None if r is None else [str(t) for t in r] for r in lp.get("top_token_ids") or []]
    return toks, tops


def render_logprobs(lp: Optional[Dict[str, Any]], chat: bool, offset: int = 0) -> Optional[Dict[str, Any]]:
    """A backend logprobs block ({"token_logprobs", "ranks", "top_token_ids", "top_logprobs", "tokens",
    "top_tokens"}) in the OpenAI completions or chat layout; offset: the text position of its first token."""
    if not isinstance(lp, dict):
        return None
    toks, tops = _token_strings(lp)
    vals, top_vals = lp.get("token_logprobs") or [], lp.get("top_logprobs") or []
    if chat:
        def item(tok, v):
            return {"token": tok, "logprob": v, "bytes": list(tok.encode("utf-8"))}
        content = []
        for i, v in enumerate(vals):
            e = item(toks[i], v)
            row = tops[i] if i < len(tops) and tops[i] is not None else []
            e["top_logprobs"] = [item(t, top_vals[i][j]) for j, t in enumerate(row)]
            content.append(e)
        return {"content": content}
    offsets, top_dicts = [], []
    for i in range(len(vals)):
        offsets.append(offset)
        offset += len(toks[i])
        if i >= len(tops) or tops[i] is None:
            top_dicts.append(None)
            continue
        d: Dict[str, Any] = {}
        for j, t in enumerate(tops[i]):  # two ids may render alike: the more likely one keeps the key
            d.setdefault(t, top_vals[i][j])
        top_dicts.append(d)
    return {"tokens": list(toks), "token_logprobs": list(vals), "top_logprobs": top_dicts, "text_offset": offsets,
            "top_token_ids": lp.get("top_token_ids")}


def render_chat(messages: Any) -> str:
    """Llama-3 chat layout: one header + body + end-of-turn per message, then an open assistant
    header for the model to continue. (The tokenizer adds the beginning-of-text token.)"""
    if not isinstance(messages, list) or not messages:
        raise ValueError("messages must be a non-empty list")
    out = []
    for m in messages:
        if not isinstance(m, dict) or m.get("role") not in _ROLES or not isinstance(m.get("content"), str):
            raise ValueError("each message needs a role in %s and a string content" % (_ROLES,))
        out.append(f"<|start_header_id|>{m['role']}<|end_header_id|>\n\n{m['content']}<|eot_id|>")
    out.append("<|start_header_id|>assistant<|end_header_id|>\n\n")
    return "".join(out)


class Gateway:
    def __init__(self, coordinator: str, timeout: float = 600.0):
        self.client = InferenceClient(coordinator, timeout=timeout)
        self.reg = CollectorRegistry()
        self.m_req = Counter("die_http_requests", "completion requests", ["model", "stream"], registry=self.reg)
        self.m_err = Counter("die_http_errors", "failed completion requests", ["model"], registry=self.reg)
        self.m_tok = Counter("die_http_output_tokens", "generated tokens", ["model"], registry=self.reg)
        self.m_lat = Histogram("die_http_latency_seconds", "request latency", ["model"], registry=self.reg,
                               buckets=(0.01, 0.05, 0.1, 0.25, 0.5, 1, 2, 5, 10, 30, 60, 120))
        self.m_ttft = Histogram("die_http_ttft_seconds", "time to first token (engine)", ["model"],
                                registry=self.reg, buckets=(0.005, 0.01, 0.025, 0.05, 0.1, 0.25, 0.5, 1, 2, 5))

        # embeddings: families of their own (the completion families keep their label sets)
        self.m_emb_req = Counter("die_http_embedding_requests", "embedding requests", ["model"], registry=self.reg)
        self.m_emb_err = Counter("die_http_embedding_errors", "failed embedding requests", ["model"],
                                 registry=self.reg)
        self.m_emb_items = Counter("die_http_embedding_inputs", "embedded input items", ["model"], registry=self.reg)
        self.m_emb_tok = Counter("die_http_embedding_prompt_tokens", "embedded prompt tokens", ["model"],
                                 registry=self.reg)
        self.m_emb_lat = Histogram("die_http_embedding_latency_seconds", "embedding request latency", ["model"],
                                   registry=self.reg, buckets=(0.005, 0.01, 0.05, 0.1, 0.25, 0.5, 1, 2, 5, 10, 30))

    def app(self) -> web.Application:
        a = web.Application()
        a.router.add_post("/v1/completions", self.completions)
        a.router.add_post("/v1/chat/completions", self.chat_completions)
        a.router.add_post("/v1/embeddings", self.embeddings)
        a.router.add_get("/v1/models", self.models)
        a.router.add_get("/health", self.health)
        a.router.add_get("/metrics", self.metrics)
        a.on_cleanup.append(self._close)
        return a

    async def _close(self, _app) -> None:
        self.client.close()

    @staticmethod
    def _inputs(body: Dict[str, Any], chat: bool = False) -> Dict[str, Any]:
        prompt = body.get("prompt")
        if isinstance(prompt, list) and len(prompt) == 1 and isinstance(prompt[0], (str, list)):
            prompt = prompt[0]  # OpenAI allows a batch of one
        if isinstance(prompt, str):
            inp: Dict[str, Any] = {"prompt": prompt}
        elif isinstance(prompt, list) and all(isinstance(x, int) for x in prompt):
            inp = {"prompt_token_ids": prompt}
        else:
            raise ValueError("prompt must be a string or a list of token ids")
        inp.update({k: body[k] for k in _SAMPLING if k in body and body[k] is not None})
        inp.setdefault("max_tokens", 16)
        fmt = body.get("response_format")
        if fmt is not None:  # OpenAI's JSON mode; "text" is the default and does nothing
            if not isinstance(fmt, dict) or not isinstance(fmt.get("type"), str):
                raise ValueError('response_format must be an object {"type": "text" | "json_object" | "json_schema"}')
            if fmt["type"] == "json_object":
                inp["guided_json_object"] = True
            elif fmt["type"] == "json_schema":
                js = fmt.get("json_schema")
                if not isinstance(js, dict) or not isinstance(js.get("schema"), dict):
                    raise ValueError('response_format type json_schema needs "json_schema": {"schema": {...}} '
                                     '("name" optional; "strict" and "description" are accepted and ignored)')
                if js.get("name") is not None and not isinstance(js["name"], str):
                    raise ValueError("response_format json_schema: name must be a string")
                if "guided_json" in inp:
                    raise ValueError("response_format json_schema and guided_json name two schemas")
                inp["guided_json"] = js["schema"]
            elif fmt["type"] != "text":
                raise ValueError(f"response_format type {fmt['type']!r} is not supported (text, json_object, "
                                 "json_schema)")
        # ranges and types of the penalties / bias: refused here with a 400, not by a worker after routing
        SamplingParams(**{k: inp[k] for k in _LOGIT_PROCESSING if k in inp})
        # the same for constrained decoding (shapes, "at most one", the regex subset, ignore_eos); a text choice
        # is tokenised by the worker: here it only has to be a non-empty string
        chk = {k: inp[k] for k in _GUIDED + ("ignore_eos",) if k in inp}
        if isinstance(chk.get("guided_choice"), list):
            if any(isinstance(c, str) and not c for c in chk["guided_choice"]):
                raise ValueError("guided_choice holds an empty string")
            chk["guided_choice"] = [[0] if isinstance(c, str) else c for c in chk["guided_choice"]]
        SamplingParams(**chk)
        if chat:  # logprobs: bool, top_logprobs: int
            want = body.get("logprobs")
            if want is not None and not isinstance(want, bool):
                raise ValueError("logprobs must be a boolean")
            if body.get("top_logprobs") is not None:
                n = _logprob_count(body["top_logprobs"], "top_logprobs")
                if not want:
                    raise ValueError("top_logprobs needs logprobs: true")
                inp["logprobs"] = n
            elif want:
                inp["logprobs"] = 0
        elif body.get("logprobs") is not None:  # logprobs: int; with echo the prompt is scored too
            inp["logprobs"] = _logprob_count(body["logprobs"], "logprobs")
            if body.get("echo"):
                inp["prompt_logprobs"] = inp["logprobs"]
        return inp

    @staticmethod
    def _choice(out: Dict[str, Any], chat: bool = False) -> Dict[str, Any]:
        c = {"index": 0, "token_ids": out.get("token_ids", []), "finish_reason": out.get("finish_reason"),
             "logprobs": render_logprobs(out.get("logprobs"), chat)}
        if out.get("prompt_logprobs") is not None:
            c["prompt_logprobs"] = render_logprobs(out["prompt_logprobs"], chat)
        if chat:
            c["message"] = {"role": "assistant", "content": out.get("text", "")}
        else:
            c["text"] = out.get("text", "")
        return c

    async def completions(self, req: web.Request) -> web.StreamResponse:
        return await self._serve(req, chat=False)

    async def chat_completions(self, req: web.Request) -> web.StreamResponse:
        return await self._serve(req, chat=True)

    async def _serve(self, req: web.Request, chat: bool) -> web.StreamResponse:
        t0 = time.perf_counter()
        try:
            body = await req.json()
            model = body["model"]
            if chat:
                body = dict(body, prompt=render_chat(body.get("messages")))
            inputs = self._inputs(body, chat)
        except (ValueError, KeyError, json.JSONDecodeError) as e:
            return web.json_response({"error": {"message": f"bad request: {e}", "type": "invalid_request"}},
                                     status=400)
        stream = bool(body.get("stream"))
        self.m_req.labels(model, str(stream).lower()).inc()
        cid = ("chatcmpl-" if chat else "cmpl-") + uuid.uuid4().hex[:24]
        created = int(time.time())
        if not stream:
            rep = await self.client.infer(model, inputs, cache=body.get("cache", True))
            return self._finish(model, cid, created, rep, t0, chat)
        resp = web.StreamResponse(headers={"Content-Type": "text/event-stream", "Cache-Control": "no-cache"})
        await resp.prepare(req)
        final: Optional[Dict[str, Any]] = None
        first = True
        offset = 0  # text position of the next chunk (completions logprobs' text_offset)
        try:
            async for frame in self.client.infer_stream(model, inputs):
                if frame.get("done") is False:
                    lps = render_logprobs(frame.get("delta_logprobs"), chat, offset)
                    offset += len(frame.get("delta_text", ""))
                    if chat:
                        delta: Dict[str, Any] = {"content": frame.get("delta_text", "")}
                        if first:
                            delta["role"] = "assistant"
                        chunk = {"id": cid, "object": "chat.completion.chunk", "created": created, "model": model,
                                 "choices": [{"index": 0, "delta": delta,
                                              "token_ids": frame.get("delta_token_ids", []), "finish_reason": None,
                                              "logprobs": lps}]}
                    else:
                        chunk = {"id": cid, "object": "text_completion", "created": created, "model": model,
                                 "choices": [{"index": 0, "text": frame.get("delta_text", ""),
                                              "token_ids": frame.get("delta_token_ids", []),
                                              "finish_reason": None, "logprobs": lps}]}
                    first = False
                    await resp.write(b"data: " + json.dumps(chunk).encode() + b"\n\n")
                else:
                    final = frame
        except (ConnectionError, asyncio.CancelledError):
            raise  # the HTTP client went away: dropping the RPC stream aborts the request upstream
        if final is None or not final.get("success"):
            self.m_err.labels(model).inc()
            err = {"error": {"message": (final or {}).get("error", "stream ended"), "type": "server_error"}}
            await resp.write(b"data: " + json.dumps(err).encode() + b"\n\n")
        else:
            out = final["outputs"]
            self._observe(model, out, t0)
            end = {"index": 0, "token_ids": [], "finish_reason": out.get("finish_reason")}
            end.update({"delta": {}} if chat else {"text": ""})
            last = {"id": cid, "object": "chat.completion.chunk" if chat else "text_completion", "created": created,
                    "model": model, "choices": [end], "usage": self._usage(out)}
            await resp.write(b"data: " + json.dumps(last).encode() + b"\n\n")
        await resp.write(b"data: [DONE]\n\n")
        await resp.write_eof()
        return resp

    @staticmethod
    def _embedding_inputs(body: Dict[str, Any]) -> list:
        """One infer payload per item of "input"; a ValueError for anything malformed."""
        if body.get("stream"):
            raise ValueError("embeddings cannot be streamed")
        x = body.get("input")
        if isinstance(x, str):
            items = [x]
        elif isinstance(x, list) and x and all(isinstance(t, int) and not isinstance(t, bool) for t in x):
            items = [x]
        elif isinstance(x, list):
            items = x
        else:
            raise ValueError("input must be a string, a list of strings, a list of token ids or a list of those")
        if not items:
            raise ValueError("input is empty")
        if len(items) > MAX_EMBED_INPUTS:
            raise ValueError(f"input holds more than {MAX_EMBED_INPUTS} items")
        fmt = body.get("encoding_format", "float")
        if fmt not in ("float", "base64"):
            raise ValueError("encoding_format must be float or base64")
        pooling = body.get("pooling", "last")
        normalize = body.get("normalize", True)
        common: Dict[str, Any] = {"pooling": pooling, "embed_normalize": normalize, "return_text": False}
        if body.get("dimensions") is not None:
            common["embed_dimensions"] = body["dimensions"]
        # values and types: refused here with a 400, not by a worker after routing
        SamplingParams(**{k: v for k, v in common.items() if k != "return_text"})
        out = []
        for it in items:
            if isinstance(it, str) and it:
                out.append(dict(common, prompt=it))
            elif isinstance(it, list) and it and all(isinstance(t, int) and not isinstance(t, bool) and t >= 0
                                                     for t in it):
                out.append(dict(common, prompt_token_ids=it))
            else:
                raise ValueError("every input item must be a non-empty string or a non-empty list of token ids")
        return out

    async def embeddings(self, req: web.Request) -> web.Response:
        t0 = time.perf_counter()
        try:
            body = await req.json()
            model = body["model"]
            payloads = self._embedding_inputs(body)
        except (ValueError, KeyError, TypeError, json.JSONDecodeError) as e:
            return web.json_response({"error": {"message": f"bad request: {e}", "type": "invalid_request"}},
                                     status=400)
        self.m_emb_req.labels(model).inc()
        # one RPC per item, all in flight at once: the worker's engine batches them into shared prefill steps
        reps = await asyncio.gather(*(self.client.infer(model, p, cache=body.get("cache", True)) for p in payloads))
        b64 = body.get("encoding_format") == "base64"
        data, tokens = [], 0
        for i, rep in enumerate(reps):
            out = rep.get("outputs") if rep.get("success") else None
            if not isinstance(out, dict) or "embedding" not in out:
                self.m_emb_err.labels(model).inc()
                msg = str(rep.get("error", "the model returned no embedding"))
                # a request the engine refused (tensor parallelism, disaggregated prefill, a bad value) is the
                # client's error
                refused = any(w in msg for w in ("not supported on", "exceeds", "out of vocabulary"))
                status = 404 if "not registered" in msg else 400 if refused else 502
                return web.json_response({"error": {"message": msg, "type": "server_error", "index": i}},
                                         status=status)
            vec = out["embedding"]
            tokens += int(out.get("prompt_tokens", 0))
            emb = base64.b64encode(struct.pack(f"<{len(vec)}f", *vec)).decode() if b64 else vec
            data.append({"object": "embedding", "index": i, "embedding": emb})
        self.m_emb_items.labels(model).inc(len(data))
        self.m_emb_tok.labels(model).inc(tokens)
        self.m_emb_lat.labels(model).observe(time.perf_counter() - t0)
        return web.json_response({"object": "list", "data": data, "model": model,
                                  "usage": {"prompt_tokens": tokens, "total_tokens": tokens}})

    def _observe(self, model: str, out: Dict[str, Any], t0: float) -> None:
        self.m_lat.labels(model).observe(time.perf_counter() - t0)
        self.m_tok.labels(model).inc(out.get("num_output_tokens", 0))
        if out.get("ttft_ms") is not None:
            self.m_ttft.labels(model).observe(out["ttft_ms"] / 1e3)

    @staticmethod
    def _usage(out: Dict[str, Any]) -> Dict[str, int]:
        p, c = int(out.get("num_prompt_tokens", 0)), int(out.get("num_output_tokens", 0))
        return {"prompt_tokens": p, "completion_tokens": c, "total_tokens": p + c}

    def _finish(self, model: str, cid: str, created: int, rep: Dict[str, Any], t0: float,
                chat: bool = False) -> web.Response:
        if not rep.get("success"):
            self.m_err.labels(model).inc()
            msg = str(rep.get("error", ""))
            # a request the engine refused (e.g. penalties on a tensor-parallel engine) is the client's error
            status = 404 if "not registered" in msg else 400 if "not supported on a" in msg else 502
            return web.json_response({"error": {"message": rep.get("error"), "type": "server_error"}}, status=status)
        out = rep["outputs"]
        if not isinstance(out, dict) or "token_ids" not in out:  # a mock model: pass its outputs through
            return web.json_response({"id": cid, "object": "text_completion", "created": created, "model": model,
                                      "outputs": out})
        self._observe(model, out, t0)
        return web.json_response({"id": cid, "object": "chat.completion" if chat else "text_completion",
                                  "created": created, "model": model, "choices": [self._choice(out, chat)],
                                  "usage": self._usage(out), "cached": bool(rep.get("cached"))})

    async def models(self, _req: web.Request) -> web.Response:
        rep = await self.client.call({"op": "models"})
        data = [{"id": m, "object": "model", "versions": v} for m, v in rep.get("models", {}).items()]
        return web.json_response({"object": "list", "data": data})

    async def health(self, _req: web.Request) -> web.Response:
        try:
            rep = await asyncio.wait_for(self.client.call({"op": "health"}), 5.0)
            ok = bool(rep.get("success"))
        except Exception:  # noqa: BLE001 - any failure means unhealthy
            ok = False
        return web.json_response({"healthy": ok}, status=200 if ok else 503)

    async def metrics(self, _req: web.Request) -> web.Response:
        return web.Response(body=generate_latest(self.reg), headers={"Content-Type": CONTENT_TYPE_LATEST})


def main(argv=None) -> None:
    setup_logging()
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--coordinator", default="127.0.0.1:9000")
    p.add_argument("--host", default="0.0.0.0")
    p.add_argument("--port", type=int, default=8000)
    a = p.parse_args(argv)
    web.run_app(Gateway(a.coordinator).app(), host=a.host, port=a.port)


if __name__ == "__main__":
    main()
