#!/usr/bin/env python3
"""Send requests to a coordinator (or a worker) and print the replies.

    python examples/example_client.py --address 127.0.0.1:9000 --model echo --inputs '{"x": 1}'
    python examples/example_client.py --model llama --prompt "Hello" --max-tokens 32
    python examples/example_client.py --model llama --prompt "Hi" -n 64 --concurrency 32   # mini load test
    python examples/example_client.py --model llama --prompt "Hello" --max-tokens 64 --stream  # token stream
    python examples/example_client.py --model llama --prompt "Hello" --logprobs 5   # per-token logprobs + top 5
    python examples/example_client.py --model llama --prompt "Hello" --repetition-penalty 1.2 --logit-bias '{"50256": -100}'
    python examples/example_client.py --model llama --prompt "Is water wet? " --guided-choice yes no
    python examples/example_client.py --model llama --prompt "A date: " --guided-regex '\d{4}-\d{2}-\d{2}'
    python examples/example_client.py --model llama --prompt "A JSON record: " --max-tokens 64 --json   # JSON mode
    python examples/example_client.py --model llama --prompt "A point: " --max-tokens 64 \
        --guided-json '{"type": "object", "properties": {"x": {"type": "integer"}, "y": {"type": "integer"}}, "required": ["x", "y"]}'
    python examples/example_client.py --model llama --prompt "a sentence to embed" --embed mean   # the prompt's vector
"""

import argparse
import asyncio
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from src.client import InferenceClient  # noqa: E402
from src.utils import percentile  # noqa: E402


async def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--address", default="127.0.0.1:9000")
    ap.add_argument("--model", default="echo")
    ap.add_argument("--inputs", default=None, help="raw JSON inputs (mock models)")
    ap.add_argument("--prompt", default=None)
    ap.add_argument("--max-tokens", type=int, default=16)
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--logprobs", type=int, default=None, metavar="N",
                    help="per-token logprobs of the raw distribution: 0 = the chosen token's, 1..20 = also the top N")
    ap.add_argument("--repetition-penalty", type=float, default=None, help="> 0; 1.0 = off")
    ap.add_argument("--logit-bias", default=None, metavar="JSON", help='{"token id": bias in [-100, 100]}, <= 300 entries')
    ap.add_argument("--guided-choice", nargs="+", default=None, metavar="TEXT",
                    help="the output is exactly one of these strings, then EOS")
    ap.add_argument("--guided-regex", default=None, metavar="PATTERN",
                    help="the output fully matches this pattern (the byte-level subset of src/guided.py), then EOS")
    ap.add_argument("--json", action="store_true", dest="json_object",
                    help="JSON mode: the output is one JSON object, then EOS (a request cut off by --max-tokens "
                         "returns an incomplete document with finish_reason length)")
    ap.add_argument("--guided-json", default=None, metavar="FILE_OR_JSON",
                    help="structured output: a JSON Schema (a file name or the JSON text itself); the output is one "
                         "document valid against it, then EOS")
    ap.add_argument("--embed", nargs="?", const="last", default=None, choices=["last", "mean"], metavar="POOLING",
                    help="return the prompt's embedding (last-token or mean pooling, L2-normalised) instead of text")
    ap.add_argument("--request-key", default=None, help="session key for shard affinity")
    ap.add_argument("-n", type=int, default=1)
    ap.add_argument("--concurrency", type=int, default=1)
    ap.add_argument("--poll", action="store_true", help="submit + poll instead of waiting")
    ap.add_argument("--stream", action="store_true", help="print token deltas as they are generated")
    a = ap.parse_args()
    if a.prompt is not None:
        inputs = {"prompt": a.prompt, "max_tokens": a.max_tokens, "temperature": a.temperature}
        if a.logprobs is not None:
            inputs["logprobs"] = a.logprobs
        if a.repetition_penalty is not None:
            inputs["repetition_penalty"] = a.repetition_penalty
        if a.logit_bias is not None:
            inputs["logit_bias"] = json.loads(a.logit_bias)
        if a.guided_choice is not None:
            inputs["guided_choice"] = a.guided_choice
        if a.guided_regex is not None:
            inputs["guided_regex"] = a.guided_regex
        if a.json_object:
            inputs["guided_json_object"] = True
        if a.guided_json is not None:
            text = a.guided_json
            if not text.lstrip().startswith("{"):
                with open(text, "r", encoding="utf-8") as f:
                    text = f.read()
            inputs["guided_json"] = json.loads(text)
        if a.embed is not None:
            inputs = {"prompt": a.prompt, "pooling": a.embed}
    else:
        inputs = json.loads(a.inputs) if a.inputs else {"text": "hello"}
    c = InferenceClient(a.address)
    if a.stream:
        t0 = time.perf_counter()
        async for frame in c.infer_stream(a.model, inputs, request_key=a.request_key):
            if frame.get("done") is False:
                lps = (frame.get("delta_logprobs") or {}).get("token_logprobs")
                print(f"[{1e3 * (time.perf_counter() - t0):8.1f} ms] +{frame['delta_token_ids']}"
                      + (f" logprobs {[round(v, 3) for v in lps]}" if lps else ""), flush=True)
            else:
                print(json.dumps(frame, indent=2)[:4000])
        c.close()
        return
    sem = asyncio.Semaphore(a.concurrency)
    lat = []

    async def one(i):
        async with sem:
            t0 = time.perf_counter()
            if a.poll:
                rid = await c.submit(a.model, inputs)
                r = await c.result(rid)
            else:
                r = await c.infer(a.model, inputs, request_key=a.request_key, cache=a.n == 1)
            lat.append(time.perf_counter() - t0)
            return r

    t0 = time.perf_counter()
    rs = await asyncio.gather(*(one(i) for i in range(a.n)))
    el = time.perf_counter() - t0
    if a.n == 1 and a.embed is not None and rs[0].get("success"):
        out = rs[0]["outputs"]
        vec = out["embedding"]
        print(f"{len(vec)} dimensions, {out['prompt_tokens']} prompt tokens: "
              f"[{', '.join(f'{v:.4f}' for v in vec[:8])}, ...]")
    elif a.n == 1:
        print(json.dumps(rs[0], indent=2)[:4000])
    else:
        ok = sum(1 for r in rs if r.get("success"))
        print(f"{ok}/{a.n} ok, {a.n / el:.1f} req/s, p50 {1e3 * percentile(lat, 50):.1f} ms, "
              f"p99 {1e3 * percentile(lat, 99):.1f} ms")
    c.close()


if __name__ == "__main__":
    asyncio.run(main())
