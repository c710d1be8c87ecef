"""What FP8 expert weights above 32 tokens cost and buy at the engine level on a MoE model: bench/w8_moe_engine_cost.py's
protocol (the same random model, memory fraction and requests, one wave of batch x (prompt -> gen), greedy, two timed
waves after a warm-up wave) with two fp8_experts engines in turn, `runs` times, both from this tree: "wide"
(ops.w8.W8_MOE_MAX_T = 128: decode steps of 33 to 128 tokens run the wide grouped W8 GEMM on the FP8 copies) and "narrow"
(W8_MOE_MAX_T = 32: those steps run the bf16 grouped GEMM on the dequantised experts, which is what every fp8_experts
engine did before the wide grouped kernel existed). ops.moe_apply reads the switch at every call and a decode hipGraph
keeps what it read at capture, so an engine is built, warmed up and timed under one value. Every engine holds
max(batches) sequences and runs each batch in turn (a wave of b prompts is a step of b tokens): one build serves all
batches. One line per engine and batch. No speed-up is promised: the lines say what it is.
With a sixth argument `mxfp4_experts` the same protocol asks the same question of the MXFP4 copies: an mxfp4_experts engine
with ops.w4.W4_MOE_MAX_T = 128 ("wide": those steps run the wide grouped W4 GEMM), one with 32 ("narrow": the bf16
grouped GEMM, what every mxfp4_experts engine did before that kernel existed) and an fp8_experts engine with
W8_MOE_MAX_T = 128 for scale ("fp8"), in turn, `runs` times.
python bench/w8_moe_wide_engine_cost.py [preset] [batches, e.g. 64,128] [prompt] [gen] [runs] [fp8_experts | mxfp4_experts]"""
import gc
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


def wave(eng, prompts, gen):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.generate(prompts, SamplingParams(max_tokens=gen))
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    preset = sys.argv[1] if len(sys.argv) > 1 else "mixtral-8x7b"
    batches = tuple(int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "64,128").split(","))
    p, g = (int(x) for x in sys.argv[3:5]) if len(sys.argv) > 4 else (512, 128)
    runs = int(sys.argv[5]) if len(sys.argv) > 5 else 2
    mode = sys.argv[6] if len(sys.argv) > 6 else "fp8_experts"
    shipped, shipped4, top = ops.w8.W8_MOE_MAX_T, ops.w4.W4_MOE_MAX_T, max(batches)
    if mode == "mxfp4_experts":   # (line's engine, weight_dtype, the limit its dtype's moe_apply branch reads)
        engines = (("wide", mode, ops.w4.W4_WIDE_MAX_M), ("narrow", mode, ops.W4_MAX_M),
                   ("fp8", "fp8_experts", ops.W8_WIDE_MAX_M))
    else:
        engines = (("wide", mode, ops.W8_WIDE_MAX_M), ("narrow", mode, ops.W8_MAX_M))
    rng = random.Random(0)
    for run in range(runs):
        for kind, dtype, max_t in engines:
            ops.w8.W8_MOE_MAX_T = ops.w4.W4_MOE_MAX_T = max_t
            cfg = EngineConfig(max_num_seqs=top, max_num_batched_tokens=top * p, max_latency_ms=0.0,
                               weight_dtype=dtype, enable_prefix_caching=False)
            print(f"building {preset} {dtype} MOE_MAX_T={max_t} (run {run})", file=sys.stderr, flush=True)
            eng = LLMEngine.from_preset(preset, device="cuda:0", cfg=cfg, max_model_len=p + g + 16)
            eng.eos_token_id = None
            for b in batches:
                draw = lambda: [[rng.randrange(3, 1000) for _ in range(p)] for _ in range(b)]  # noqa: E731
                print(f"built; batch {b}: warm-up wave", file=sys.stderr, flush=True)
                wave(eng, draw(), g)  # warms up
                waves = []
                for _ in range(2):
                    ps = draw()
                    full, first = wave(eng, ps, g), wave(eng, ps, 1)
                    waves.append({"wave_s": round(full, 4), "req_per_s": round(b / full, 2),
                                  "prefill_wave_s": round(first, 4),
                                  "ms_per_decode_step": round((full - first) / (g - 1) * 1e3, 3)})
                print(json.dumps({"bench": "w8_moe_wide_engine_cost", "preset": preset, "engine": kind,
                                  "weight_dtype": dtype,
                                  ("W4_MOE_MAX_T" if dtype == "mxfp4_experts" else "W8_MOE_MAX_T"): max_t,
                                  "run": run, "batch": b, "prompt": p, "gen": g,
                                  "kv_blocks": eng.pool.num_blocks, "w8_moe_tiles": eng.model.w8_moe_tiles,
                                  "w4_moe_tiles": eng.model.w4_moe_tiles,
                                  "waves": waves}), flush=True)
            del eng
            gc.collect()  # a dead engine is a cycle: freed before the next one is built
            torch.cuda.empty_cache()
    ops.w8.W8_MOE_MAX_T, ops.w4.W4_MOE_MAX_T = shipped, shipped4


if __name__ == "__main__":
    main()
