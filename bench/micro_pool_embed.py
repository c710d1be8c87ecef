"""ops.pool_embed (1024-thread workgroups, 16-byte row loads, no float atomics) at the served shapes: H = 4096 and
8192; 32 segments x 512 rows, and one segment of 8,192 rows; last and mean pooling, L2-normalised; mean with one
workgroup per segment and with the rows split over ops.pool_parts(rows) workgroups (the served form).
Each figure is the median over 20 timings of 10 back-to-back launches (device events around the 10). Per form one
JSON line with the kernel's time, the time the bytes it must read would take at 6.3 TB/s (mean: every row of the
segments; last: one row per segment), and the torch expression on the same rows
(F.normalize(hidden.view(S, L, H).float().mean(1)) / F.normalize(hidden[last].float())). The result is checked
against the torch expression first.

--engine PRESET [--layers N]: the prefill step of the same tokens as generation requests (max_tokens = 1: the path
every request took before there were embedding requests), and as last / mean embedding requests, median of three
alternated runs in one process; with the kernel's time from above that gives the kernel's share of the step. With
--layers the model is built with N layers and the line also carries the step's time scaled to the preset's depth
(an extrapolation: the per-layer work dominates a prefill step).

python bench/micro_pool_embed.py [--hidden 4096 8192] [--engine llama3-8b]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from src import ops  # noqa: E402

REPS, INNER = 20, 10
HBM_TB_S = 6.3
SHAPES = ((32, 512), (1, 8192))  # (segments, rows each)


def timed(fn) -> float:
    """Median microseconds per call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / INNER)
    ts.sort()
    return ts[len(ts) // 2]


def kernel_section(h: int, dev) -> dict:
    res = {}
    for segs_n, rows in SHAPES:
        t = segs_n * rows
        g = torch.Generator(device=dev).manual_seed(h + t)
        hidden = (torch.randn(t, h, device=dev, generator=g) + 0.25).to(torch.bfloat16)
        acc = torch.zeros(segs_n, h, device=dev)
        out = torch.zeros(segs_n, h, device=dev)
        last_rows = torch.arange(segs_n, device=dev) * rows + rows - 1
        for mode, split in (("last", False), ("mean", False), ("mean", True)):
            mean = mode == "mean"
            parts = ops.pool_parts(rows) if split else 1
            if split and parts == 1:
                continue
            segs = torch.tensor([ops.pool_segment(i * rows, rows, i, rows, mean=mean, part_base=i * parts, parts=parts)
                                 for i in range(segs_n)], dtype=torch.int32, device=dev)
            scratch = (torch.zeros(segs_n * parts, h, device=dev), torch.zeros(segs_n, dtype=torch.int32, device=dev))
            if mean:
                def expr():
                    return F.normalize(hidden.view(segs_n, rows, h).float().mean(1), dim=-1)
            else:
                def expr():
                    return F.normalize(hidden.index_select(0, last_rows).float(), dim=-1)

            def kern():
                return ops.pool_embed(hidden, segs, acc, out, scratch=scratch, max_parts=parts)
            kern()
            err = float((out - expr()).abs().max())
            assert err < 1e-5, (mode, err)
            us = timed(kern)
            us_torch = timed(expr)
            nbytes = (t if mean else segs_n) * h * 2
            floor_us = nbytes / (HBM_TB_S * 1e12) * 1e6
            res[(segs_n, rows, mode)] = us  # the split form runs last: the served one where ops.pool_parts splits
            print(json.dumps({"bench": "pool_embed", "hidden": h, "segments": segs_n, "rows": rows, "mode": mode,
                              "parts_per_segment": parts, "us": round(us, 2), "read_bytes": nbytes,
                              "floor_us_at_6.3_tb_s": round(floor_us, 2), "x_floor": round(us / floor_us, 2),
                              "read_tb_s": round(nbytes / us / 1e6, 3), "torch_us": round(us_torch, 2),
                              "max_abs_diff_vs_torch": err}), flush=True)
    return res


def engine_section(preset: str, layers: int, kern: dict, dev) -> None:
    from src.config import EngineConfig
    from src.engine import LLMEngine
    from src.models.presets import get_preset
    from src.preproc import SamplingParams

    full_layers = get_preset(preset).num_layers
    over = {"num_layers": layers} if layers else {}
    cfg = EngineConfig(max_num_seqs=32, max_num_batched_tokens=16384, max_latency_ms=0.0, num_kv_blocks=2304,
                       enable_prefix_caching=False, use_cuda_graph=False)
    eng = LLMEngine.from_preset(preset, device=str(dev), cfg=cfg, max_model_len=8448, capture=False, **over)
    eng.eos_token_id = None
    h = eng.arch.hidden_size
    g = torch.Generator().manual_seed(0)
    kinds = {"generate": SamplingParams(max_tokens=1), "embed_last": SamplingParams(pooling="last"),
             "embed_mean": SamplingParams(pooling="mean")}

    def run(prompts, kind, tag):
        s0 = eng.get_stats()
        for i, p in enumerate(prompts):
            eng.add_request(f"{tag}-{kind}-{i}-{s0['steps']}", p, kinds[kind])
        while eng.has_work():
            eng.step()
        s1 = eng.get_stats()
        return (s1["prefill_time"] - s0["prefill_time"]) * 1e3, s1["steps"] - s0["steps"]

    for segs_n, rows in SHAPES:
        prompts = [torch.randint(3, 30000, (rows,), generator=g).tolist() for _ in range(segs_n)]
        for kind in kinds:
            run(prompts, kind, "warm")
        res = {}
        for rep in range(3):
            for kind in kinds:
                res.setdefault(kind, []).append(run(prompts, kind, f"r{rep}"))
        line = {"bench": "pool_embed_prefill_share", "preset": preset, "hidden": h, "layers": layers or full_layers,
                "preset_layers": full_layers, "segments": segs_n, "rows": rows}
        scale = full_layers / (layers or full_layers)
        for kind in kinds:
            ms = sorted(r[0] for r in res[kind])
            line[f"{kind}_prefill_ms"] = round(ms[1], 3)
            line[f"{kind}_steps"] = res[kind][0][1]
        gen_ms = line["generate_prefill_ms"]
        line["generate_prefill_ms_at_preset_depth"] = round(gen_ms * scale, 3)
        for mode in ("last", "mean"):
            us = kern.get((segs_n, rows, mode))
            if us is not None:
                line[f"kernel_{mode}_us"] = round(us, 2)
                line[f"kernel_{mode}_share_of_generate_prefill"] = round(us / 1e3 / (gen_ms * scale), 6)
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--engine", default=None, help="preset for the prefill-step share (e.g. llama3-8b)")
    ap.add_argument("--layers", type=int, default=0, help="build the preset with this many layers (0: all)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_pool_embed needs a GPU")
    dev = torch.device("cuda:0")
    kern = {}
    for h in a.hidden:
        kern[h] = kernel_section(h, dev)
    if a.engine:
        from src.models.presets import get_preset

        engine_section(a.engine, a.layers, kern.get(get_preset(a.engine).hidden_size, {}), dev)


if __name__ == "__main__":
    main()
