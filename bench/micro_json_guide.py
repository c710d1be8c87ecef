"""ops.json_guide (one 1024-thread workgroup per row walks every token's bytes through the JSON pushdown table, then
masks the row as ops.byte_guide does) at a decode step's shape (32 x 128,256 bf16) over the seeded byte table of
tests/json_guide_reference.py (tokens of 0..40 bytes, rich in JSON punctuation). The rows stand in a mix of
configurations (inside a string, before a value, after a value, in a number; depths 1..32). In the same run, and
ALTERNATED with it: ops.byte_guide over the same table with a regex DFA of the nearest state count ([a-z ]{0,N}, walked
from LDS; most tokens of this table die at its first byte), the like-for-like pair (every JSON row inside a string
against a DFA in which every byte has a transition: both walk every token to its end), a json_guide launch whose workgroups all exit at once (every slot -1: what a guided batch without a JSON
row pays) and the same for byte_guide. Each figure is the median over --rounds of a median over 20 timings of 10
back-to-back launches; "cold" is the first launch of the process (its LDS-size request and table misses included),
timed alone. Two rows are checked bit for bit against ops.reference.json_guide_rows first. One JSON line per form.

--engine PRESET: decode ms/step of a plain batch, a byte-guided batch and a JSON batch, alternated --engine-runs times in one
process.

python bench/micro_json_guide.py [--rows 32] [--vocab 128256] [--engine llama-mini]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from src import guided, ops  # noqa: E402
from src.ops import reference as ref  # noqa: E402
from tests import json_guide_reference as oracle  # noqa: E402

REPS, INNER = 20, 10
EOS = oracle.EOS
PREFIXES = (b'{"ke', b'{"k":', b'{"k":"v"', b'{"k":[1.5', b'{"k":[{"a":"x', oracle.KEY * 31, oracle.KEY * 32,
            b'{"k":[{"a":"x"}')


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


def once(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def kernel_section(rows: int, vocab: int, rounds: int, dev) -> None:
    i32 = torch.int32
    table, off, data = oracle.build_vocab(vocab, np.random.default_rng(vocab))
    trans, done = guided.build_json_table()
    n = trans.shape[0]
    d_off, d_by = torch.from_numpy(off).to(dev), torch.from_numpy(data).to(dev)
    d_jtr = torch.from_numpy(trans).to(dev)
    desc = torch.tensor([n, done, EOS, 0], dtype=i32, device=dev).repeat(rows, 1)
    cfgs = [oracle.device_config(trans, n, PREFIXES[r % len(PREFIXES)], False) for r in range(rows)]
    cur = torch.tensor([c[0] for c in cfgs], dtype=i32, device=dev)
    jstk = torch.from_numpy(np.array([[c[1], c[2]] for c in cfgs], dtype=np.uint32).view(np.int32)).to(dev)
    # the regex DFA of the nearest state count, on the same byte table (every byte has a single-byte token)
    pattern = "[a-z ]{0,%d}" % (n - 1)
    bg = guided.compile_byte_guide(pattern, table, EOS, len(table))
    d_btr = torch.from_numpy(bg.trans).to(dev)
    d_bac = torch.from_numpy(bg.accept).to(dev)
    bdesc = torch.tensor([0, bg.n_states, EOS, 0], dtype=i32, device=dev).repeat(rows, 1)
    bcur = torch.from_numpy(np.random.default_rng(rows).integers(0, bg.n_states, size=rows).astype(np.int32)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(rows)
    base = (torch.randn(rows, vocab, device=dev, generator=gen) * 4).to(torch.bfloat16)
    slot = torch.randperm(rows, device=dev, generator=gen).int()
    idle = torch.full((rows,), -1, dtype=i32, device=dev)
    err = torch.zeros(rows, dtype=i32, device=dev)
    lm_part = torch.zeros(rows, 501, 2, dtype=i32, device=dev)
    adv = torch.randint(0, vocab, (rows,), device=dev, generator=gen)

    work = base.clone()
    cold = once(lambda: ops.json_guide(work, slot, desc, d_jtr, d_off, d_by, cur, jstk, err, lm_part=lm_part))
    print(json.dumps({"bench": "json_guide", "form": "json_guide_cold_first_launch", "rows": rows, "vocab": vocab,
                      "us": round(cold, 1)}), flush=True)

    # bit equality with the reference op on two rows (no advance: every configuration is a legal start)
    got, lm_got, c_got, j_got = base[:2].clone(), lm_part[:2].clone(), cur.clone(), jstk.clone()
    ops.json_guide(got, slot[:2], desc, d_jtr, d_off, d_by, c_got, j_got, err, lm_part=lm_got)
    want, lm_want, c_want, j_want = base[:2].cpu(), lm_part[:2].cpu(), cur.cpu(), jstk.cpu()
    e_want = torch.zeros(rows, dtype=i32)
    ref.json_guide_rows(want, slot[:2].cpu(), desc.cpu(), d_jtr.cpu(), d_off.cpu(), d_by.cpu(), c_want, j_want, e_want,
                        None, lm_want)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)) and torch.equal(lm_got.cpu(), lm_want)
    assert int(err.sum()) == 0 and int(e_want.sum()) == 0
    print(json.dumps({"bench": "json_guide", "check": "bit-equal", "states": n, "regex_states": bg.n_states,
                      "allowed_in_two_rows": int((got.float() > float("-inf")).sum())}), flush=True)

    # the like-for-like pair: every JSON row inside a key string (nearly every byte is read, nothing pushes or pops)
    # against a DFA of as many states in which every byte has a transition; both walk every token to its end
    in_str = oracle.device_config(trans, n, b'{"ke', False)
    scur = torch.full((rows,), in_str[0], dtype=i32, device=dev)
    sjstk = torch.tensor([in_str[1], in_str[2]], dtype=i32, device=dev).repeat(rows, 1)
    alive = ((np.arange(n)[:, None] + 1 + np.arange(256)[None, :]) % n).astype(np.int16)
    d_atr = torch.from_numpy(alive).to(dev)
    d_aac = torch.zeros(n, dtype=torch.uint8, device=dev)
    adesc = torch.tensor([0, n, EOS, 0], dtype=i32, device=dev).repeat(rows, 1)
    runs = {
        "json_guide_all_rows_in_a_string": lambda: ops.json_guide(work, slot, desc, d_jtr, d_off, d_by, scur, sjstk,
                                                                  err, lm_part=lm_part),
        "byte_guide_%d_states_every_byte_alive" % n: lambda: ops.byte_guide(work, slot, adesc, d_atr, d_aac, d_off,
                                                                            d_by, bcur, err, lm_part=lm_part),
        "json_guide_%d_states" % n: lambda: ops.json_guide(work, slot, desc, d_jtr, d_off, d_by, cur, jstk, err,
                                                           lm_part=lm_part),
        "byte_guide_%d_states_lds" % bg.n_states: lambda: ops.byte_guide(work, slot, bdesc, d_btr, d_bac, d_off, d_by,
                                                                         bcur, err, lm_part=lm_part),
        "json_guide_all_slots_idle": lambda: ops.json_guide(work, idle, desc, d_jtr, d_off, d_by, cur, jstk, err,
                                                            advance_ids=adv, lm_part=lm_part),
        "byte_guide_all_slots_idle": lambda: ops.byte_guide(work, idle, bdesc, d_btr, d_bac, d_off, d_by, bcur, err,
                                                            advance_ids=adv, lm_part=lm_part),
    }
    # the like-for-like pair once more on bench/micro_byte_guide.py's vocabulary (1..8-byte tokens, mostly lowercase):
    # the table behind the 217 us in byte_guide.hip's header
    from micro_byte_guide import synthetic_vocab

    short = [b or b"" for b in synthetic_vocab(vocab)]
    soff = np.zeros(vocab + 1, dtype=np.int32)
    soff[1:] = np.cumsum([len(b) for b in short])
    d_soff = torch.from_numpy(soff).to(dev)
    d_sby = torch.from_numpy(np.frombuffer(b"".join(short), dtype=np.uint8).copy()).to(dev)
    runs["json_guide_all_rows_in_a_string_1_to_8_byte_tokens"] = lambda: ops.json_guide(
        work, slot, desc, d_jtr, d_soff, d_sby, scur, sjstk, err, lm_part=lm_part)
    runs["byte_guide_%d_states_every_byte_alive_1_to_8_byte_tokens" % n] = lambda: ops.byte_guide(
        work, slot, adesc, d_atr, d_aac, d_soff, d_sby, bcur, err, lm_part=lm_part)
    res = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            work.copy_(base)
            res[name].append(round(timed(fn), 2))
    assert int(err.sum()) == 0
    for name, us in res.items():
        print(json.dumps({"bench": "json_guide", "form": name, "rows": rows, "vocab": vocab,
                          "us_median": sorted(us)[len(us) // 2], "us_rounds": us}), flush=True)


def engine_section(preset: str, rows: int, gen: int, runs: int, dev) -> None:
    from src.config import EngineConfig
    from src.engine import LLMEngine
    from src.preproc import SamplingParams

    cfg = EngineConfig(max_num_seqs=rows, max_num_batched_tokens=4096, max_latency_ms=0.0, num_kv_blocks=4096)
    eng = LLMEngine.from_preset(preset, device=str(dev), cfg=cfg, max_model_len=1024)
    eng.eos_token_id = 2
    eng.token_bytes = oracle.engine_table(eng.arch.vocab_size)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(3, 30000, (64,), generator=g).tolist() for _ in range(rows)]
    # neither guided batch can end within gen tokens: the pattern never accepts, and the JSON rows open a key and
    # stay inside it ('{' is legal in a string and outranks the closing quote)
    kinds = {"raw": {"ignore_eos": True},
             "byte_guided": {"guided_regex": "[a-z ]{%d}" % (8 * gen)},
             "json_guided": {"guided_json_object": True, "logit_bias": {3 + ord("{"): 100, 3 + ord('"'): 90}}}

    def run(kind):
        s0 = eng.get_stats()
        for i, p in enumerate(prompts):
            eng.add_request(f"b{kind}-{i}-{s0['steps']}", p, SamplingParams(max_tokens=gen, **kinds[kind]))
        while eng.has_work():
            eng.step()
        s1 = eng.get_stats()
        steps = gen - 1  # decode steps of the batch (the first token is the prefill's)
        return round((s1["decode_time"] - s0["decode_time"]) * 1e3 / steps, 4)

    for kind in kinds:
        run(kind)  # warm every path
    res = {}
    for _ in range(runs):  # alternate the forms
        for kind in kinds:
            res.setdefault(kind, []).append(run(kind))
    for kind in kinds:
        ms = sorted(res[kind])
        print(json.dumps({"bench": "decode_step_json_guide", "preset": preset, "rows": rows, "gen": gen, "batch": kind,
                          "ms_per_step_median": ms[len(ms) // 2], "ms_per_step_all": ms}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[32])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--engine", default=None, help="preset for the decode ms/step comparison (e.g. llama-mini)")
    ap.add_argument("--engine-rows", type=int, default=32)
    ap.add_argument("--engine-runs", type=int, default=5)
    ap.add_argument("--gen", type=int, default=65)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_json_guide needs a GPU")
    dev = torch.device("cuda:0")
    for rows in a.rows:
        kernel_section(rows, a.vocab, a.rounds, dev)
    if a.engine:
        engine_section(a.engine, a.engine_rows, a.gen, a.engine_runs, dev)


if __name__ == "__main__":
    main()
