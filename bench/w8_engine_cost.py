"""What weight_dtype="fp8" costs and buys at the engine level: the same model (random weights), the same memory
fraction and the same requests (batch x (prompt -> gen), greedy) with bf16 weights and with FP8 (e4m3) weights,
alternating, `runs` engines each. Prints per engine the planned block count, the decode copies' bytes and the wall
time of two waves after a warm-up wave. The bf16 engine decodes on the five-launch fused layer, the FP8 engine on the
slab sequence with the W8A16 decode GEMM (half the weight stream, more launches): no speed-up is promised, the line
says what it is. Both engines run from this tree: a default engine takes none of the new code on its decode path.
`plan`: "table" (W8_TILE_CFG's measured tiles, the default) or "rule" (the table emptied: every projection gets the
closest-to-256-workgroups tile); each line names it.
python bench/w8_engine_cost.py [preset] [batch] [prompt] [gen] [runs] [plan]"""
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.ops.w8 import W8_TILE_CFG  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402


def main():
    preset = sys.argv[1] if len(sys.argv) > 1 else "llama3-8b"
    b, p, g = (int(x) for x in sys.argv[2:5]) if len(sys.argv) > 4 else (32, 512, 128)
    runs = int(sys.argv[5]) if len(sys.argv) > 5 else 3
    plan = sys.argv[6] if len(sys.argv) > 6 else "table"
    if plan == "rule":
        W8_TILE_CFG.clear()
    rng = random.Random(0)
    for run in range(runs):
        for dtype in ("auto", "fp8"):
            cfg = EngineConfig(max_num_seqs=b, max_num_batched_tokens=b * p, max_latency_ms=0.0, weight_dtype=dtype,
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
            print(json.dumps({"bench": "w8_engine_cost", "plan": "W8_TILE_CFG" if plan == "table" else "closest-to-256 rule",
                              "preset": preset, "weight_dtype": dtype, "run": run, "batch": b,
                              "prompt": p, "gen": g, "kv_blocks": eng.pool.num_blocks,
                              "decode_copies_GiB": round(eng.model.decode_copy_bytes(eng.model.decode_buckets(b)) / 2**30, 2),
                              "w8_plan": eng.model.w8_plan, "wave_s": [round(t, 4) for t in times[1:]]}), flush=True)
            del eng
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
