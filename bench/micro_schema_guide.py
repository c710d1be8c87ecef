"""ops.schema_guide (one 1024-thread workgroup per row walks every token's bytes through a schema's byte pushdown
table, int32 entries read from the arena through L2, return states on a stack) at a decode step's shape (32 x 128,256
bf16) over the seeded byte table of tests/json_guide_reference.py, by bench/micro_json_guide.py's protocol: each figure
is the median over --rounds of a median over 20 timings of 10 back-to-back launches, the forms ALTERNATED in one
process.

  * {"type": "object"} from micro_json_guide.py's prefixes against ops.json_guide on the same byte table and the same
    configurations: the language is identical, so the difference is the cost of int32 entries read through L2 (the
    JSON table is walked from LDS) and of the return-state stack;
  * a flat object schema of eight members, rows spread over its positions;
  * the launch whose workgroups all exit at once (every slot -1: what the schema graph set pays for rows that are not
    schema rows).
Two rows are checked bit for bit against ops.reference.schema_guide_rows first. One JSON line per form.

--engine PRESET: decode ms/step of a raw, a JSON and a schema batch, alternated --engine-runs times in one process.

python bench/micro_schema_guide.py [--rows 32] [--vocab 128256] [--engine llama-mini]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bench"))

from micro_json_guide import PREFIXES, once, timed  # noqa: E402
from src import guided, ops  # noqa: E402
from src.ops import reference as ref  # noqa: E402
from tests import json_guide_reference as oracle  # noqa: E402

EOS = oracle.EOS
FLAT = {"type": "object",
        "properties": {"id": {"type": "integer"}, "name": {"type": "string"}, "score": {"type": "number"},
                       "active": {"type": "boolean"}, "kind": {"enum": ["alpha", "beta", "gamma"]},
                       "tags": {"type": "array", "items": {"type": "string"}, "maxItems": 4},
                       "note": {"type": ["string", "null"]}, "code": {"type": "string", "pattern": "^[A-Z]{3}-[0-9]{4}$"}},
        "required": ["id", "name", "score", "active", "kind", "tags", "note", "code"]}
FLAT_DOC = b'{"id":17,"name":"ab cd","score":-1.5e3,"active":true,"kind":"beta","tags":["x","yz"],"note":null,"code":"ABC-1234"}'


def config_after(trans, prefix):
    c = (0, 0, ())
    for x in prefix:
        c = guided.schema_step(trans, c, x)[0]
    return c


def slot_tables(cfgs, base, n, rows, dev):
    i32 = torch.int32
    desc = torch.tensor([base, n, EOS, 0], dtype=i32, device=dev).repeat(rows, 1)
    cur = torch.tensor([c[0] for c in cfgs], dtype=i32, device=dev)
    sdep = torch.tensor([c[1] for c in cfgs], dtype=i32, device=dev)
    stk = np.zeros((rows, ops.GUIDE_SCHEMA_MAX_DEPTH), dtype=np.int16)
    for r, c in enumerate(cfgs):
        stk[r, :c[1]] = c[2]
    return desc, cur, sdep, torch.from_numpy(stk).to(dev)


def kernel_section(rows: int, vocab: int, rounds: int, dev) -> None:
    i32 = torch.int32
    table, off, data = oracle.build_vocab(vocab, np.random.default_rng(vocab))
    d_off, d_by = torch.from_numpy(off).to(dev), torch.from_numpy(data).to(dev)
    jtrans, done = guided.build_json_table()
    nj = jtrans.shape[0]
    d_jtr = torch.from_numpy(jtrans).to(dev)
    jdesc = torch.tensor([nj, done, EOS, 0], dtype=i32, device=dev).repeat(rows, 1)
    jcfgs = [oracle.device_config(jtrans, nj, PREFIXES[r % len(PREFIXES)], False) for r in range(rows)]
    jcur = torch.tensor([c[0] for c in jcfgs], dtype=i32, device=dev)
    jstk = torch.from_numpy(np.array([[c[1], c[2]] for c in jcfgs], dtype=np.uint32).view(np.int32)).to(dev)
    # both schema guides in one arena, as the runner holds them
    t_obj, a_obj = guided.schema_to_pda({"type": "object"})
    t_flat, a_flat = guided.schema_to_pda(FLAT)
    arena = torch.full((ops.GUIDE_SCHEMA_STATE_ARENA, 256), -1, dtype=i32, device=dev)
    acc = torch.zeros(ops.GUIDE_SCHEMA_STATE_ARENA, dtype=torch.uint8, device=dev)
    b_obj, b_flat = 0, len(t_obj)
    arena[b_obj:b_obj + len(t_obj)].copy_(torch.from_numpy(t_obj))
    acc[b_obj:b_obj + len(t_obj)].copy_(torch.from_numpy(a_obj))
    arena[b_flat:b_flat + len(t_flat)].copy_(torch.from_numpy(t_flat))
    acc[b_flat:b_flat + len(t_flat)].copy_(torch.from_numpy(a_flat))
    ocfgs = [config_after(t_obj, PREFIXES[r % len(PREFIXES)]) for r in range(rows)]
    assert [c[1] for c in ocfgs] == [c[1] for c in jcfgs]                  # the same depths as the JSON rows
    odesc, ocur, osdep, osstk = slot_tables(ocfgs, b_obj, len(t_obj), rows, dev)
    cuts = np.linspace(1, len(FLAT_DOC) - 1, rows).astype(int)
    fcfgs = [config_after(t_flat, FLAT_DOC[:k]) for k in cuts]
    fdesc, fcur, fsdep, fsstk = slot_tables(fcfgs, b_flat, len(t_flat), rows, dev)
    gen = torch.Generator(device=dev).manual_seed(rows)
    base = (torch.randn(rows, vocab, device=dev, generator=gen) * 4).to(torch.bfloat16)
    slot = torch.randperm(rows, device=dev, generator=gen).int()
    idle = torch.full((rows,), -1, dtype=i32, device=dev)
    err = torch.zeros(rows, dtype=i32, device=dev)
    lm_part = torch.zeros(rows, 501, 2, dtype=i32, device=dev)
    adv = torch.randint(0, vocab, (rows,), device=dev, generator=gen)

    work = base.clone()
    cold = once(lambda: ops.schema_guide(work, slot, odesc, arena, acc, d_off, d_by, ocur, osdep, osstk, err,
                                         lm_part=lm_part))
    print(json.dumps({"bench": "schema_guide", "form": "schema_guide_cold_first_launch", "rows": rows, "vocab": vocab,
                      "us": round(cold, 1)}), flush=True)

    # bit equality with the reference op on two rows of each guide, and with ops.json_guide on the identical language
    for name, (desc, cur, sdep, sstk) in (("object", (odesc, ocur, osdep, osstk)),
                                          ("flat", (fdesc, fcur, fsdep, fsstk))):
        got, lm_got = base[:2].clone(), lm_part[:2].clone()
        ops.schema_guide(got, slot[:2], desc, arena, acc, d_off, d_by, cur.clone(), sdep.clone(), sstk.clone(), err,
                         lm_part=lm_got)
        want, lm_want, e_want = base[:2].cpu(), lm_part[:2].cpu(), torch.zeros(rows, dtype=i32)
        ref.schema_guide_rows(want, slot[:2].cpu(), desc.cpu(), arena.cpu(), acc.cpu(), d_off.cpu(), d_by.cpu(),
                              cur.cpu(), sdep.cpu(), sstk.cpu(), e_want, None, lm_want)
        assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)) and torch.equal(lm_got.cpu(), lm_want)
        assert int(err.sum()) == 0 and int(e_want.sum()) == 0
        allowed = int((got.float() > float("-inf")).sum())
        if name.startswith("object"):
            jgot = base[:2].clone()
            ops.json_guide(jgot, slot[:2], jdesc, d_jtr, d_off, d_by, jcur.clone(), jstk.clone(), err)
            # json_guide has no per-token push cap: a token of this table that holds more than four pushes is the
            # only difference the two masks may show
            diff = int((jgot.view(torch.int16) != got.view(torch.int16)).sum())
            print(json.dumps({"bench": "schema_guide", "check": "against json_guide", "guide": name,
                              "entries_that_differ": diff}),
                  flush=True)
        print(json.dumps({"bench": "schema_guide", "check": "bit-equal", "guide": name,
                          "states": int(desc[0, 1]), "allowed_in_two_rows": allowed}), flush=True)

    runs = {
        "schema_guide_type_object_%d_states" % len(t_obj): lambda: ops.schema_guide(
            work, slot, odesc, arena, acc, d_off, d_by, ocur, osdep, osstk, err, lm_part=lm_part),
        "json_guide_%d_states_same_configurations" % nj: lambda: ops.json_guide(
            work, slot, jdesc, d_jtr, d_off, d_by, jcur, jstk, err, lm_part=lm_part),
        "schema_guide_flat_8_members_%d_states" % len(t_flat): lambda: ops.schema_guide(
            work, slot, fdesc, arena, acc, d_off, d_by, fcur, fsdep, fsstk, err, lm_part=lm_part),
        "schema_guide_all_slots_idle": lambda: ops.schema_guide(
            work, idle, odesc, arena, acc, d_off, d_by, ocur, osdep, osstk, err, advance_ids=adv, lm_part=lm_part),
        "json_guide_all_slots_idle": lambda: ops.json_guide(
            work, idle, jdesc, d_jtr, d_off, d_by, jcur, jstk, err, advance_ids=adv, lm_part=lm_part),
    }
    res = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            work.copy_(base)
            res[name].append(round(timed(fn), 2))
    assert int(err.sum()) == 0
    for name, us in res.items():
        print(json.dumps({"bench": "schema_guide", "form": name, "rows": rows, "vocab": vocab,
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
    # neither guided batch can end within gen tokens: the rows open a key (or the "name" string) and stay inside it
    # ('{' is legal in a string and outranks the closing quote)
    bias = {3 + ord("{"): 100, 3 + ord('"'): 90}
    kinds = {"raw": {"ignore_eos": True},
             "json_guided": {"guided_json_object": True, "logit_bias": bias},
             "schema_guided": {"guided_json": {"type": "object", "properties": {"name": {"type": "string"}},
                                               "required": ["name"]},
                               "logit_bias": {**bias, **{3 + ord(c): 80 for c in "name:"}}}}

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
        print(json.dumps({"bench": "decode_step_schema_guide", "preset": preset, "rows": rows, "gen": gen,
                          "batch": kind, "ms_per_step_median": ms[len(ms) // 2], "ms_per_step_all": ms}), flush=True)


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
        raise SystemExit("micro_schema_guide needs a GPU")
    dev = torch.device("cuda:0")
    for rows in a.rows:
        kernel_section(rows, a.vocab, a.rounds, dev)
    if a.engine:
        engine_section(a.engine, a.engine_rows, a.gen, a.engine_runs, dev)


if __name__ == "__main__":
    main()
