"""ops.logit_process (one 1024-thread workgroup per row: logits load + state load + logits store, 750 KiB per
128,256-entry row) at a decode step's shape (32 x 128,256 bf16), with and without bias lists and candidates, next
to ops.sample's one-workgroup-per-row argmax on the same rows. Each figure is the median over 20 timings of 10
back-to-back launches (events around the 10); one JSON line per form. The rows are checked bit for bit against
ops.reference.logit_process first.

--engine PRESET: also the decode ms/step of a --engine-rows batch on the processed graphs (every request with
repetition_penalty / frequency_penalty) against the raw graphs (plain requests), alternated three times in one
process on the same box.

python bench/micro_logit_process.py [--rows 32] [--vocab 128256] [--engine llama3-8b]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from src import ops  # noqa: E402
from src.ops import reference as ref  # noqa: E402

REPS, INNER = 20, 10


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


def kernel_section(rows: int, vocab: int, dev) -> None:
    g = torch.Generator(device=dev).manual_seed(rows)
    base = (torch.randn(rows, vocab, device=dev, generator=g) * 4).to(torch.bfloat16)
    state = torch.zeros(rows, vocab, dtype=torch.int16, device=dev)
    state[torch.rand(rows, vocab, device=dev, generator=g) < 0.01] = -32768   # prompt bits
    state += (torch.rand(rows, vocab, device=dev, generator=g) < 0.005).to(torch.int16) * 3
    slot = torch.randperm(rows, device=dev, generator=g).int()
    rp = 1.3
    params = torch.tensor([rp, float(torch.tensor(1.0) / torch.tensor(rp)), 0.5, 0.25], device=dev).repeat(rows, 1)
    nb = ops.LOGIT_BIAS_MAX
    bias_ids = torch.stack([torch.randperm(vocab, device=dev, generator=g)[:nb] for _ in range(rows)]).int()
    bias_vals = torch.rand(rows, nb, device=dev, generator=g) * 10 - 5
    cnt0 = torch.zeros(rows, dtype=torch.int32, device=dev)
    cnt300 = torch.full((rows,), nb, dtype=torch.int32, device=dev)
    count_ids = torch.randint(0, vocab, (rows,), device=dev, generator=g)
    lm_part = torch.zeros(rows, 501, 2, dtype=torch.int32, device=dev)

    # bit equality with the reference op once (bias lists of 300, no count update)
    got = base.clone()
    ops.logit_process(got, slot, state, params, cnt300, bias_ids, bias_vals)
    for r in (0, rows - 1):
        s = int(slot[r])
        st = state[s].cpu().to(torch.int32) & 0xffff
        bias = torch.zeros(vocab)
        bias[bias_ids[s].cpu().long()] = bias_vals[s].cpu()
        want = ref.logit_process(base[r].cpu(), (st & 0x8000) != 0, st & 0x7fff, *params[s].tolist(), bias)
        assert torch.equal(got[r].cpu().view(torch.int16), want.view(torch.int16))

    work = base.clone()
    traffic = rows * vocab * 6  # logits read + state read + logits write
    for form, cnt, cid, lm in (("penalties", cnt0, None, None), ("penalties_bias300", cnt300, None, None),
                               ("decode_step_form", cnt300, count_ids, lm_part)):
        us = timed(lambda: ops.logit_process(work, slot, state, params, cnt, bias_ids, bias_vals, count_ids=cid,
                                             lm_part=lm))
        print(json.dumps({"bench": "logit_process", "form": form, "rows": rows, "vocab": vocab, "us": round(us, 2),
                          "traffic_tb_s": round(traffic / us / 1e6, 3)}), flush=True)
    tok = torch.empty(rows, dtype=torch.long, device=dev)
    us = timed(lambda: ops.sample(base, out=tok))
    print(json.dumps({"bench": "logit_process", "form": "sample_greedy_one_wg_per_row", "rows": rows, "vocab": vocab,
                      "us": round(us, 2)}), flush=True)


def engine_section(preset: str, rows: int, gen: int, dev) -> None:
    from src.config import EngineConfig
    from src.engine import LLMEngine
    from src.preproc import SamplingParams

    cfg = EngineConfig(max_num_seqs=rows, max_num_batched_tokens=4096, max_latency_ms=0.0, num_kv_blocks=4096)
    eng = LLMEngine.from_preset(preset, device=str(dev), cfg=cfg, max_model_len=1024)
    eng.eos_token_id = None
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(3, 30000, (64,), generator=g).tolist() for _ in range(rows)]
    kinds = {"raw": {}, "processed": {"repetition_penalty": 1.2, "frequency_penalty": 0.5}}

    def run(kind):
        s0 = eng.get_stats()
        for i, p in enumerate(prompts):
            eng.add_request(f"b{kind}-{i}-{s0['steps']}", p, SamplingParams(max_tokens=gen, **kinds[kind]))
        while eng.has_work():
            eng.step()
        s1 = eng.get_stats()
        steps = gen - 1  # decode steps of the batch (the first token is the prefill's)
        return {"ms_per_step": round((s1["decode_time"] - s0["decode_time"]) * 1e3 / steps, 4),
                "logit_process_launches": s1["logit_process_launches"] - s0["logit_process_launches"],
                "decode_windows": s1.get("decode_windows", 0) - s0.get("decode_windows", 0)}

    run("raw"), run("processed")  # warm both paths
    res = {}
    for _ in range(3):  # alternate the two forms
        for kind in kinds:
            res.setdefault(kind, []).append(run(kind))
    for kind in kinds:
        ms = sorted(r["ms_per_step"] for r in res[kind])
        print(json.dumps({"bench": "decode_step_logit_process", "preset": preset, "rows": rows, "gen": gen,
                          "graphs": kind, "ms_per_step_median": ms[1], "ms_per_step_all": ms,
                          "logit_process_launches": res[kind][0]["logit_process_launches"],
                          "decode_windows": res[kind][0]["decode_windows"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[32])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--engine", default=None, help="preset for the decode ms/step A/B (e.g. llama3-8b)")
    ap.add_argument("--engine-rows", type=int, default=32)
    ap.add_argument("--gen", type=int, default=65)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_logit_process needs a GPU")
    dev = torch.device("cuda:0")
    for rows in a.rows:
        kernel_section(rows, a.vocab, dev)
    if a.engine:
        engine_section(a.engine, a.engine_rows, a.gen, dev)


if __name__ == "__main__":
    main()
