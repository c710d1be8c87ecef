"""What weight_dtype="fp8_experts" costs and buys at the engine level on a MoE model: the same model (random weights),
the same memory fraction and the same requests (one wave of batch x (prompt -> gen), greedy) with bf16 experts and with
FP8 (e4m3) experts, alternating, `runs` engines each, both from this tree. The two engines differ in two launches per
layer of a decode step of <= 32 tokens: the grouped bf16 GEMMs, or the grouped W8A16 GEMMs on half the bytes. Per engine
one line: the planned block count, the FP8 copies' bytes, and per timed wave (after a warm-up wave) the wall time, the
requests per second and the time per decode step, taken as (wave - a wave of the same prompts with one generated token)
/ (gen - 1). No speed-up is promised: the line says what it is.
A sixth argument lists the weight dtypes to alternate, comma-separated (default auto,fp8_experts; mxfp4_experts: the
grouped W4A16 GEMMs on 17 / 64 of the bytes; "fp8_copies_GiB" counts whichever quantised copies the engine keeps).
python bench/w8_moe_engine_cost.py [preset] [batch] [prompt] [gen] [runs] [dtypes]"""
import gc
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402


def wave(eng, prompts, gen):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.generate(prompts, SamplingParams(max_tokens=gen))
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    preset = sys.argv[1] if len(sys.argv) > 1 else "mixtral-8x7b"
    b, p, g = (int(x) for x in sys.argv[2:5]) if len(sys.argv) > 4 else (32, 512, 128)
    runs = int(sys.argv[5]) if len(sys.argv) > 5 else 2
    dtypes = tuple(sys.argv[6].split(",")) if len(sys.argv) > 6 else ("auto", "fp8_experts")
    rng = random.Random(0)
    for run in range(runs):
        for dtype in dtypes:
            cfg = EngineConfig(max_num_seqs=b, max_num_batched_tokens=b * p, max_latency_ms=0.0, weight_dtype=dtype,
                               enable_prefix_caching=False)
            print(f"building {preset} weight_dtype={dtype} (run {run})", file=sys.stderr, flush=True)
            eng = LLMEngine.from_preset(preset, device="cuda:0", cfg=cfg, max_model_len=p + g + 16)
            eng.eos_token_id = None
            draw = lambda: [[rng.randrange(3, 1000) for _ in range(p)] for _ in range(b)]  # noqa: E731
            print("built; warm-up wave", file=sys.stderr, flush=True)
            wave(eng, draw(), g)  # warms up
            waves = []
            for _ in range(2):
                ps = draw()
                full, first = wave(eng, ps, g), wave(eng, ps, 1)
                waves.append({"wave_s": round(full, 4), "req_per_s": round(b / full, 2),
                              "prefill_wave_s": round(first, 4),
                              "ms_per_decode_step": round((full - first) / (g - 1) * 1e3, 3)})
            print(json.dumps({"bench": "w8_moe_engine_cost", "preset": preset, "weight_dtype": dtype, "run": run,
                              "batch": b, "prompt": p, "gen": g, "kv_blocks": eng.pool.num_blocks,
                              "fp8_copies_GiB": round(eng.model._w8_bytes() / 2**30, 2),
                              "w8_moe_tiles": eng.model.w8_moe_tiles, "w4_moe_tiles": eng.model.w4_moe_tiles,
                              "waves": waves}), flush=True)
            del eng
            gc.collect()  # a dead engine is a cycle: freed before the next one is built
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
