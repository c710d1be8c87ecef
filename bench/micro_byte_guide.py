"""ops.byte_guide (one 1024-thread workgroup per row walks every token's bytes through the row's byte DFA, then
masks the row as ops.token_guide does) at a decode step's shape (32 x 128,256 bf16) over a synthetic vocabulary of
1..8-byte tokens: a 27-state guide ([a-z]+( [a-z]+){0,8}) and a 201-state guide ([a-z ]{0,200}), both walked from
LDS, the 201-state guide once more behind junk states so that it is read through L2 instead, next to ops.token_guide on a
full-vocabulary CSR state and to a byte_guide launch whose workgroups all exit at once (every slot -1: what a batch
without a byte-guided row pays). The forms are ALTERNATED: --rounds passes over all of them, each figure the median
over the rounds of a median over 20 timings of 10 back-to-back launches; one JSON line per form. Two rows are
checked bit for bit against ops.reference.byte_guide_rows first.

--compile: host compile time of three patterns on the same vocabulary, the CSR lift (compile_regex) against the
byte form (compile_byte_guide); runs without a GPU.
--engine PRESET: decode ms/step of a plain batch, a CSR-guided batch (allowed_token_ids) and a byte-guided batch,
alternated three times in one process.

python bench/micro_byte_guide.py [--rows 32] [--vocab 128256] [--compile] [--engine llama-mini]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from src import guided, ops  # noqa: E402
from src.ops import reference as ref  # noqa: E402

REPS, INNER = 20, 10
EOS = 1
PATTERNS = (r"[a-z]+( [a-z]+){0,8}", r'\{"name": "[a-zA-Z ]{1,20}", "age": \d{1,3}\}', r"[a-z ]{0,200}")


def synthetic_vocab(vocab: int, seed: int = 0):
    """id -> bytes: 0 pad and 1 EOS without bytes, the 256 single bytes, then 2..8 bytes, mostly lowercase."""
    rng = np.random.default_rng(seed)
    alphabet = b"abcdefghijklmnopqrstuvwxyz" * 3 + b'    ABCDEFGHIJ0123456789{}":,.-'
    table = [None, None] + [bytes([b]) for b in range(256)]
    lens = rng.integers(2, 9, size=vocab - len(table))
    picks = rng.integers(0, len(alphabet), size=int(lens.sum()))
    at = 0
    for n in lens:
        table.append(bytes(alphabet[i] for i in picks[at:at + n]))
        at += n
    return table


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


def kernel_section(rows: int, vocab: int, rounds: int, dev) -> None:
    table = synthetic_vocab(vocab)
    off = np.zeros(vocab + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(b or b"") for b in table])
    data = np.frombuffer(b"".join(b or b"" for b in table), dtype=np.uint8).copy()
    g28 = guided.compile_byte_guide(PATTERNS[0], table, EOS, vocab)
    g201 = guided.compile_byte_guide(PATTERNS[2], table, EOS, vocab)
    pad = ops.GUIDE_BYTE_LDS_STATES + 1 - g201.n_states      # junk states in front: the region no longer fits LDS
    i32 = torch.int32
    n_arena = g28.n_states + g201.n_states + pad + g201.n_states
    trans = np.full((n_arena, 256), -1, dtype=np.int16)
    accept = np.zeros(n_arena, dtype=np.uint8)
    b28, b201, bl2 = 0, g28.n_states, g28.n_states + g201.n_states
    trans[b28:b201], accept[b28:b201] = g28.trans, g28.accept
    trans[b201:bl2], accept[b201:bl2] = g201.trans, g201.accept
    trans[bl2 + pad:], accept[bl2 + pad:] = np.where(g201.trans >= 0, g201.trans + pad, -1), g201.accept
    d_tr, d_ac = torch.from_numpy(trans).to(dev), torch.from_numpy(accept).to(dev)
    d_off, d_by = torch.from_numpy(off).to(dev), torch.from_numpy(data).to(dev)
    gen = torch.Generator(device=dev).manual_seed(rows)
    base = (torch.randn(rows, vocab, device=dev, generator=gen) * 4).to(torch.bfloat16)
    slot = torch.randperm(rows, device=dev, generator=gen).int()
    idle = torch.full((rows,), -1, dtype=i32, device=dev)
    err = torch.zeros(rows, dtype=i32, device=dev)
    lm_part = torch.zeros(rows, 501, 2, dtype=i32, device=dev)
    rng = np.random.default_rng(rows)

    def guide(base_state, n, shift=0):
        desc = torch.tensor([base_state, n, EOS, 0], dtype=i32, device=dev).repeat(rows, 1)
        cur = torch.from_numpy(rng.integers(0, n - shift, size=rows).astype(np.int32) + shift).to(dev)
        return desc, cur

    small = "byte_guide_%d_states_lds" % g28.n_states
    forms = {small: guide(b28, g28.n_states),
             "byte_guide_201_states_lds": guide(b201, g201.n_states),
             "byte_guide_201_states_l2": guide(bl2, g201.n_states + pad, shift=pad)}

    # bit equality with the reference op on two rows of each form (no advance: every state is a legal start)
    for name, (desc, cur) in forms.items():
        got, lm_got, cur_got = base[:2].clone(), lm_part[:2].clone(), cur.clone()
        ops.byte_guide(got, slot[:2], desc, d_tr, d_ac, d_off, d_by, cur_got, err, lm_part=lm_got)
        want, lm_want, cur_want, err_want = base[:2].cpu(), lm_part[:2].cpu(), cur.cpu(), torch.zeros(rows, dtype=i32)
        ref.byte_guide_rows(want, slot[:2].cpu(), desc.cpu(), d_tr.cpu(), d_ac.cpu(), d_off.cpu(), d_by.cpu(),
                            cur_want, err_want, None, lm_want)
        assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)) and torch.equal(lm_got.cpu(), lm_want)
        assert int(err.sum()) == 0 and int(err_want.sum()) == 0, name
        allowed = int((got.float() > float("-inf")).sum())
        print(json.dumps({"bench": "byte_guide", "form": name, "check": "bit-equal", "allowed_in_two_rows": allowed}),
              flush=True)

    # ops.token_guide on a full-vocabulary CSR state, as bench/micro_token_guide.py builds it
    edges = torch.zeros(vocab, 2, dtype=i32, device=dev)
    edges[:, 0] = torch.arange(vocab, dtype=i32, device=dev)
    rowptr = torch.tensor([0, vocab], dtype=i32, device=dev)
    tdesc = torch.tensor([0, 1, 0, vocab], dtype=i32, device=dev).repeat(rows, 1)
    tcur = torch.zeros(rows, dtype=i32, device=dev)
    adv_full = torch.randint(0, vocab, (rows,), device=dev, generator=gen)

    work = base.clone()
    runs = {}
    for name, (desc, cur) in forms.items():
        c = cur.clone()
        runs[name] = lambda desc=desc, c=c: ops.byte_guide(work, slot, desc, d_tr, d_ac, d_off, d_by, c, err,
                                                           lm_part=lm_part)
    d0, c0 = forms[small]
    runs["byte_guide_all_slots_idle"] = lambda: ops.byte_guide(work, idle, d0, d_tr, d_ac, d_off, d_by, c0, err,
                                                               advance_ids=adv_full, lm_part=lm_part)
    runs["token_guide_full_vocabulary"] = lambda: ops.token_guide(work, slot, tdesc, rowptr, edges, tcur, err,
                                                                  lm_part=lm_part)
    runs["token_guide_full_vocabulary_decode_step_form"] = lambda: ops.token_guide(
        work, slot, tdesc, rowptr, edges, tcur, err, advance_ids=adv_full, lm_part=lm_part)
    res = {k: [] for k in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            work.copy_(base)
            res[name].append(round(timed(fn), 2))
    assert int(err.sum()) == 0
    for name, us in res.items():
        print(json.dumps({"bench": "byte_guide", "form": name, "rows": rows, "vocab": vocab,
                          "us_median": sorted(us)[len(us) // 2], "us_rounds": us}), flush=True)


def compile_section(vocab: int) -> None:
    table = synthetic_vocab(vocab)
    for pattern in PATTERNS:
        t0 = time.perf_counter()
        g = guided.compile_byte_guide(pattern, table, EOS, vocab)
        t_byte = time.perf_counter() - t0
        t0 = time.perf_counter()
        try:
            a = guided.compile_regex(pattern, table, EOS, vocab)
            csr = {"csr_states": a.n_states, "csr_edges": a.n_edges}
        except ValueError as e:
            csr = {"csr_refused": str(e)}
        t_csr = time.perf_counter() - t0
        print(json.dumps({"bench": "guide_compile", "pattern": pattern, "vocab": vocab, "byte_states": g.n_states,
                          "byte_guide_ms": round(t_byte * 1e3, 2), "csr_lift_ms": round(t_csr * 1e3, 1), **csr}),
              flush=True)


def engine_section(preset: str, rows: int, gen: int, dev) -> None:
    from src.config import EngineConfig
    from src.engine import LLMEngine
    from src.preproc import SamplingParams

    cfg = EngineConfig(max_num_seqs=rows, max_num_batched_tokens=4096, max_latency_ms=0.0, num_kv_blocks=4096)
    eng = LLMEngine.from_preset(preset, device=str(dev), cfg=cfg, max_model_len=1024)
    eng.eos_token_id = EOS
    eng.token_bytes = synthetic_vocab(eng.arch.vocab_size)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(3, 30000, (64,), generator=g).tolist() for _ in range(rows)]
    kinds = {"raw": {"ignore_eos": True}, "csr_guided": {"allowed_token_ids": list(range(1000, 1512)), "ignore_eos": True},
             "byte_guided": {"guided_regex": "[a-z ]{%d}" % (8 * gen)}}     # never accepts within gen tokens: no EOS

    def run(kind):
        s0 = eng.get_stats()
        for i, p in enumerate(prompts):
            eng.add_request(f"b{kind}-{i}-{s0['steps']}", p, SamplingParams(max_tokens=gen, **kinds[kind]))
        while eng.has_work():
            eng.step()
        s1 = eng.get_stats()
        steps = gen - 1  # decode steps of the batch (the first token is the prefill's)
        return {"ms_per_step": round((s1["decode_time"] - s0["decode_time"]) * 1e3 / steps, 4),
                "byte_guide_launches": s1["byte_guide_launches"] - s0["byte_guide_launches"]}

    for kind in kinds:
        run(kind)  # warm every path
    res = {}
    for _ in range(3):  # alternate the forms
        for kind in kinds:
            res.setdefault(kind, []).append(run(kind))
    for kind in kinds:
        ms = sorted(r["ms_per_step"] for r in res[kind])
        print(json.dumps({"bench": "decode_step_byte_guide", "preset": preset, "rows": rows, "gen": gen, "batch": kind,
                          "ms_per_step_median": ms[1], "ms_per_step_all": ms,
                          "byte_guide_launches": res[kind][0]["byte_guide_launches"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[32])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--compile", action="store_true", help="host compile times only (no GPU needed)")
    ap.add_argument("--engine", default=None, help="preset for the decode ms/step comparison (e.g. llama-mini)")
    ap.add_argument("--engine-rows", type=int, default=32)
    ap.add_argument("--gen", type=int, default=65)
    a = ap.parse_args()
    if a.compile:
        compile_section(a.vocab)
        return
    if not torch.cuda.is_available():
        raise SystemExit("micro_byte_guide needs a GPU")
    dev = torch.device("cuda:0")
    for rows in a.rows:
        kernel_section(rows, a.vocab, a.rounds, dev)
    if a.engine:
        engine_section(a.engine, a.engine_rows, a.gen, dev)


if __name__ == "__main__":
    main()
