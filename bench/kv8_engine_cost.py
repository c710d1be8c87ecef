"""What kv_cache_dtype="fp8" costs and buys at the engine level: the same model (random weights), the same memory
fraction and the same requests (batch x (prompt -> gen), greedy) on a bf16 pool and on an e4m3 pool. Prints per
dtype the planned block count and the wall time of one wave after a warm-up wave. Both engines decode on the
five-launch fused layer (the FP8 one through attention_kv8.hip's fused prologue; before that kernel existed its
decode steps ran _forward_decode_slab, which is what profiles/kv8_fused_decode_engine.jsonl compares against).
python bench/kv8_engine_cost.py [preset] [batch] [prompt] [gen]"""
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


def main():
    preset = sys.argv[1] if len(sys.argv) > 1 else "llama3-8b"
    b, p, g = (int(x) for x in sys.argv[2:5]) if len(sys.argv) > 4 else (32, 512, 128)
    rng = random.Random(0)
    for dtype in ("auto", "fp8"):
        cfg = EngineConfig(max_num_seqs=b, max_num_batched_tokens=b * p, max_latency_ms=0.0, kv_cache_dtype=dtype,
                           gpu_memory_fraction=0.5, enable_prefix_caching=False)
        eng = LLMEngine.from_preset(preset, device="cuda:0", cfg=cfg, max_model_len=p + g + 16)
        eng.eos_token_id = None
        times = []
        for _ in range(3):  # the first wave warms up
            ps = [[rng.randrange(3, 1000) for _ in range(p)] for _ in range(b)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.generate(ps, SamplingParams(max_tokens=g))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        print(json.dumps({"bench": "kv8_engine_cost", "preset": preset, "kv_cache_dtype": dtype, "batch": b,
                          "prompt": p, "gen": g, "kv_blocks": eng.pool.num_blocks,
                          "kv_GiB": round(eng.pool.nbytes / 2**30, 2), "wave_s": [round(t, 4) for t in times[1:]]}),
              flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
