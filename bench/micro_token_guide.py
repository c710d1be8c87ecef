"""ops.token_guide (one 1024-thread workgroup per row: at most one 16-B load and one 16-B store per group of 8
logits, 500 KiB per 128,256-entry row) at a decode step's shape (32 x 128,256 bf16), with 2-edge states (nearly
everything barred: groups without an allowed entry are stored without being loaded) and with a full-vocabulary
allowed list (nothing barred: groups are loaded for the candidates and not stored), next to ops.logit_process
with empty bias lists on the same rows in the same run. Each figure is the median over 20 timings of 10
back-to-back launches (events around the 10); one JSON line per form. The rows are checked bit for bit against
ops.reference.token_guide_rows first.

--engine PRESET: also the decode ms/step of a --engine-rows batch on the guided graphs (every request with an
allowed_token_ids list) against the raw graphs (plain requests), alternated three times in one process on the same
box.

python bench/micro_token_guide.py [--rows 32] [--vocab 128256] [--engine llama3-8b]
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
    slot = torch.randperm(rows, device=dev, generator=g).int()
    # one region: state 0 = the whole vocabulary (self-loops), states 1.. = two edges each, back to themselves
    i32 = torch.int32
    pairs = torch.stack([torch.randperm(vocab, device=dev, generator=g)[:2].sort().values for _ in range(rows)]).to(i32)
    edges = torch.zeros(vocab + 2 * rows, 2, dtype=i32, device=dev)
    edges[:vocab, 0] = torch.arange(vocab, dtype=i32, device=dev)
    edges[vocab:, 0] = pairs.reshape(-1)
    edges[vocab:, 1] = torch.arange(1, rows + 1, dtype=i32, device=dev).repeat_interleave(2)
    rowptr = torch.cat([torch.tensor([0], dtype=i32, device=dev),
                        vocab + 2 * torch.arange(rows + 1, dtype=i32, device=dev)])
    desc = torch.tensor([0, rows + 1, 0, vocab + 2 * rows], dtype=i32, device=dev).repeat(rows, 1)
    cur_full = torch.zeros(rows, dtype=i32, device=dev)
    cur_two = torch.arange(1, rows + 1, dtype=i32, device=dev)
    err = torch.zeros(rows, dtype=i32, device=dev)
    lm_part = torch.zeros(rows, 501, 2, dtype=torch.int32, device=dev)
    # every advance id has an edge in its row's state (row r reads slot[r]: state slot[r] + 1, a self-loop)
    adv_two = pairs[slot.long(), 0].long().contiguous()
    adv_full = torch.randint(0, vocab, (rows,), device=dev, generator=g)

    # bit equality with the reference op once (2-edge states, advance and candidates)
    got, lm_got, cur_got = base.clone(), lm_part.clone(), cur_two.clone()
    ops.token_guide(got, slot, desc, rowptr, edges, cur_got, err, advance_ids=adv_two, lm_part=lm_got)
    want, lm_want, cur_want, err_want = base.cpu(), lm_part.cpu(), cur_two.cpu(), torch.zeros(rows, dtype=i32)
    ref.token_guide_rows(want, slot.cpu(), desc.cpu(), rowptr.cpu(), edges.cpu(), cur_want, err_want,
                         adv_two.cpu(), lm_want)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)) and torch.equal(lm_got.cpu(), lm_want)
    assert torch.equal(cur_got.cpu(), cur_want) and int(err.sum()) == 0 and int(err_want.sum()) == 0

    work = base.clone()
    forms = (("two_edge_states", cur_two, None, None, rows * vocab * 2),
             ("two_edge_states_decode_step_form", cur_two, adv_two, lm_part, rows * vocab * 2),
             ("full_vocabulary", cur_full, None, None, 0),
             ("full_vocabulary_decode_step_form", cur_full, adv_full, lm_part, rows * vocab * 2))
    for form, cur, adv, lm, traffic in forms:
        us = timed(lambda: ops.token_guide(work, slot, desc, rowptr, edges, cur, err, advance_ids=adv, lm_part=lm))
        print(json.dumps({"bench": "token_guide", "form": form, "rows": rows, "vocab": vocab, "us": round(us, 2),
                          "row_traffic_tb_s": round(traffic / us / 1e6, 3)}), flush=True)
    assert int(err.sum()) == 0
    # ops.logit_process with empty bias lists on the same rows, same run (750 KiB per row)
    state = torch.zeros(rows, vocab, dtype=torch.int16, device=dev)
    params = torch.tensor([1.3, float(torch.tensor(1.0) / torch.tensor(1.3)), 0.5, 0.25], device=dev).repeat(rows, 1)
    cnt0 = torch.zeros(rows, dtype=i32, device=dev)
    bias_ids = torch.zeros(rows, ops.LOGIT_BIAS_MAX, dtype=i32, device=dev)
    bias_vals = torch.zeros(rows, ops.LOGIT_BIAS_MAX, device=dev)
    work = base.clone()
    us = timed(lambda: ops.logit_process(work, slot, state, params, cnt0, bias_ids, bias_vals))
    print(json.dumps({"bench": "token_guide", "form": "logit_process_empty_bias", "rows": rows, "vocab": vocab,
                      "us": round(us, 2), "row_traffic_tb_s": round(rows * vocab * 6 / us / 1e6, 3)}), flush=True)


def engine_section(preset: str, rows: int, gen: int, dev) -> None:
    from src.config import EngineConfig
    from src.engine import LLMEngine
    from src.preproc import SamplingParams

    cfg = EngineConfig(max_num_seqs=rows, max_num_batched_tokens=4096, max_latency_ms=0.0, num_kv_blocks=4096)
    eng = LLMEngine.from_preset(preset, device=str(dev), cfg=cfg, max_model_len=1024)
    eng.eos_token_id = None
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(3, 30000, (64,), generator=g).tolist() for _ in range(rows)]
    kinds = {"raw": {}, "guided": {"allowed_token_ids": list(range(1000, 1512))}}

    def run(kind):
        s0 = eng.get_stats()
        for i, p in enumerate(prompts):
            eng.add_request(f"b{kind}-{i}-{s0['steps']}", p, SamplingParams(max_tokens=gen, **kinds[kind]))
        while eng.has_work():
            eng.step()
        s1 = eng.get_stats()
        steps = gen - 1  # decode steps of the batch (the first token is the prefill's)
        return {"ms_per_step": round((s1["decode_time"] - s0["decode_time"]) * 1e3 / steps, 4),
                "token_guide_launches": s1["token_guide_launches"] - s0["token_guide_launches"],
                "decode_windows": s1.get("decode_windows", 0) - s0.get("decode_windows", 0)}

    run("raw"), run("guided")  # warm both paths
    res = {}
    for _ in range(3):  # alternate the two forms
        for kind in kinds:
            res.setdefault(kind, []).append(run(kind))
    for kind in kinds:
        ms = sorted(r["ms_per_step"] for r in res[kind])
        print(json.dumps({"bench": "decode_step_token_guide", "preset": preset, "rows": rows, "gen": gen,
                          "graphs": kind, "ms_per_step_median": ms[1], "ms_per_step_all": ms,
                          "token_guide_launches": res[kind][0]["token_guide_launches"],
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
        raise SystemExit("micro_token_guide needs a GPU")
    dev = torch.device("cuda:0")
    for rows in a.rows:
        kernel_section(rows, a.vocab, dev)
    if a.engine:
        engine_section(a.engine, a.engine_rows, a.gen, dev)


if __name__ == "__main__":
    main()
