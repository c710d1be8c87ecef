"""ops.token_logprobs (one 1024-thread workgroup per row) at a decode step's shape (32 x 128,256 bf16, the rows in
L2) and at a prompt-scoring slab (1,024 x 128,256, 250 MiB: from HBM), N = 0 / 5 / 20, next to — on the same
logits — ops.sample greedy without lm_part (the row's argmax only) and torch's log_softmax + topk. Each figure is
the median over 20 timings of 10 back-to-back launches (events around the 10); one JSON line per form. The result
is checked against the torch pair first (ids where the torch top-k is tie-free, logprobs within 1e-4).

--engine PRESET: also the decode ms/step of a --rows batch with logprobs=5 against the plain step, through the
engine (windows of hipGraph replays, one token_logprobs launch behind each replay).

python bench/micro_token_logprobs.py [--rows 32 1024] [--vocab 128256] [--engine llama3-8b]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from src import ops  # noqa: E402

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
    logits = (torch.randn(rows, vocab, device=dev, generator=g) * 4).to(torch.bfloat16)
    targets = torch.randint(0, vocab, (rows,), device=dev, generator=g)
    row_bytes = rows * vocab * 2

    def emit(form, us, passes=None, **kw):
        rec = {"bench": "token_logprobs", "form": form, "rows": rows, "vocab": vocab, "us": round(us, 2)}
        if passes:  # bytes the kernel reads: `passes` walks over every row (random rows: the top-N threshold comes
            # from the key window of the second pass, not from the four-pass radix select)
            rec["passes"] = passes
            rec["read_tb_s"] = round(passes * row_bytes / us / 1e6, 3)
        rec.update(kw)
        print(json.dumps(rec), flush=True)

    # check against the torch pair once (fp32 log_softmax; top-k ids compared where the boundary is tie-free)
    lsm = torch.log_softmax(logits.float(), -1)
    lp, rank, top_lp, top_id = ops.token_logprobs(logits, targets, 20)
    assert (lp - lsm.gather(1, targets[:, None])[:, 0]).abs().max().item() < 1e-4
    tv, ti = torch.topk(lsm, 21, dim=-1)
    assert (top_lp - tv[:, :20]).abs().max().item() < 1e-4
    free = tv[:, 19] != tv[:, 20]
    assert torch.equal(top_id[free].long().sort(-1).values, ti[free][:, :20].sort(-1).values)
    del lsm, tv, ti

    for n in (0, 5, 20):
        out = (torch.empty(rows, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
               torch.empty(rows, 20, device=dev), torch.empty(rows, 20, dtype=torch.int32, device=dev))
        emit(f"token_logprobs_n{n}", timed(lambda: ops.token_logprobs(logits, targets, n, out=out)),
             passes=2 if n == 0 else 3)
    tok = torch.empty(rows, dtype=torch.long, device=dev)
    emit("sample_greedy_one_wg_per_row", timed(lambda: ops.sample(logits, out=tok)), passes=1)
    scratch = (torch.zeros(rows * 32, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev))
    emit("sample_greedy_split", timed(lambda: ops.sample(logits, out=tok, scratch=scratch)), passes=1)
    for n in (5, 20):
        emit(f"torch_log_softmax_topk_n{n}",
             timed(lambda: torch.topk(torch.log_softmax(logits.float(), -1), n, dim=-1)))
    emit("torch_log_softmax_only", timed(lambda: torch.log_softmax(logits.float(), -1)))


def engine_section(preset: str, rows: int, gen: int, dev) -> None:
    from src.config import EngineConfig
    from src.engine import LLMEngine
    from src.preproc import SamplingParams

    cfg = EngineConfig(max_num_seqs=rows, max_num_batched_tokens=4096, max_latency_ms=0.0, num_kv_blocks=4096)
    eng = LLMEngine.from_preset(preset, device=str(dev), cfg=cfg, max_model_len=1024)
    eng.eos_token_id = None
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(3, 30000, (64,), generator=g).tolist() for _ in range(rows)]

    def run(lp):
        s0 = eng.get_stats()
        done = []
        for i, p in enumerate(prompts):
            eng.add_request(f"b{lp}-{i}-{s0['steps']}", p, SamplingParams(max_tokens=gen, logprobs=lp),
                            on_finish=done.append)
        while eng.has_work():
            eng.step()
        s1 = eng.get_stats()
        steps = gen - 1  # decode steps of the batch (the first token is the prefill's)
        return {"ms_per_step": round((s1["decode_time"] - s0["decode_time"]) * 1e3 / steps, 4),
                "logprob_launches": s1["logprob_launches"] - s0["logprob_launches"],
                "decode_windows": s1.get("decode_windows", 0) - s0.get("decode_windows", 0),
                "tokens": [list(s.output_ids) for s in sorted(done, key=lambda s: s.request_id)]}

    run(None), run(5)  # warm both paths
    res = {}
    for rep in range(3):  # alternate the two forms
        for lp in (None, 5):
            r = run(lp)
            res.setdefault(lp, []).append(r)
    same = all(a["tokens"] == b["tokens"] for a, b in zip(res[None], res[5]))
    for lp in (None, 5):
        ms = sorted(r["ms_per_step"] for r in res[lp])
        print(json.dumps({"bench": "decode_step_logprobs", "preset": preset, "rows": rows, "gen": gen,
                          "logprobs": lp, "ms_per_step_median": ms[1], "ms_per_step_all": ms,
                          "logprob_launches": res[lp][0]["logprob_launches"],
                          "decode_windows": res[lp][0]["decode_windows"], "tokens_equal": same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[32, 1024])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--engine", default=None, help="preset for the decode ms/step A/B (e.g. llama3-8b)")
    ap.add_argument("--engine-rows", type=int, default=32)
    ap.add_argument("--gen", type=int, default=65)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_token_logprobs needs a GPU")
    dev = torch.device("cuda:0")
    for rows in a.rows:
        kernel_section(rows, a.vocab, dev)
    if a.engine:
        engine_section(a.engine, a.engine_rows, a.gen, dev)


if __name__ == "__main__":
    main()
