"""What the wide W8A16 decode GEMM (33 to 128 rows) costs and buys at the engine level: bench/w8_engine_cost.py's
protocol (the same random model, memory fraction and requests, batch x (prompt -> gen), greedy, two timed waves after a
warm-up wave) with three engines in turn, `runs` times: bf16 weights ("auto"), FP8 weights with the wide row buckets
switched off ("fp8_narrow": steps above 32 rows run the bf16 kernels on the dequantised weights, which is what every
FP8-weight engine did before the wide kernel existed) and FP8 weights as shipped in this tree ("fp8"). No speed-up is
promised, the lines say what it is.
python bench/w8_wide_engine_cost.py [preset] [batch] [prompt] [gen] [runs]"""
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from src import ops  # noqa: E402
from src.config import EngineConfig  # noqa: E402
from src.engine import LLMEngine  # noqa: E402
from src.preproc import SamplingParams  # noqa: E402


def main():
    preset = sys.argv[1] if len(sys.argv) > 1 else "llama3-8b"
    b, p, g = (int(x) for x in sys.argv[2:5]) if len(sys.argv) > 4 else (64, 512, 128)
    runs = int(sys.argv[5]) if len(sys.argv) > 5 else 3
    shipped, wide = ops.W8_WIDE_BUCKETS, os.environ.get("DIE_W8_WIDE_BUCKETS")
    if wide is not None:  # e.g. "64,128": what "fp8" runs, to measure a bucket that is not shipped
        shipped = tuple(int(v) for v in wide.split(",") if v)
    rng = random.Random(0)
    for run in range(runs):
        for kind in ("auto", "fp8_narrow", "fp8"):
            ops.W8_WIDE_BUCKETS = () if kind == "fp8_narrow" else shipped   # read per step by CausalLM._w8_path
            cfg = EngineConfig(max_num_seqs=b, max_num_batched_tokens=b * p, max_latency_ms=0.0,
                               weight_dtype=kind.split("_")[0], gpu_memory_fraction=0.5, enable_prefix_caching=False)
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
            print(json.dumps({"bench": "w8_wide_engine_cost", "preset": preset, "engine": kind, "run": run, "batch": b,
                              "prompt": p, "gen": g, "wide_buckets": list(ops.W8_WIDE_BUCKETS) if kind != "auto" else None,
                              "kv_blocks": eng.pool.num_blocks, "wave_s": [round(t, 4) for t in times[1:]]}), flush=True)
            del eng
            torch.cuda.empty_cache()
    ops.W8_WIDE_BUCKETS = shipped


if __name__ == "__main__":
    main()
