"""
The tests' own oracle of the logit-processing contract (csrc/kernels/logit_process.hip, ops.logit_process):
pure torch, fp32, every step ONE individually rounded operation in the kernel's order, so that torch on the CPU
reproduces the kernel bit for bit. Deliberately a copy of src/ops/reference.py's function, not an import.

For the bf16 logit z of token t, with c = how often t was generated so far (saturating at 32767):
    1. x = float(z) + bias[t]                      (0 where there is no bias)
    2. if t is in the prompt or c > 0:             x = x * inv_rp if x > 0 else x * rp
    3. x = x - freq * float(c)
    4. if c > 0:                                   x = x - pres
    5. one rounding to bf16
inv_rp is fp32(1 / rp), computed once on the host: nothing divides per element.
"""

from __future__ import annotations

import numpy as np
import torch

COUNT_MAX = 32767


def inv_f32(rp: float) -> float:
    """fp32(1 / fp32(rp)) as the host passes it to the kernel."""
    return float(np.float32(1.0) / np.float32(rp))


def logit_process(logits: torch.Tensor, in_prompt: torch.Tensor, counts: torch.Tensor, rp: float, inv_rp: float,
                  freq: float, pres: float, bias: torch.Tensor = None) -> torch.Tensor:
    """One row (or rows sharing the parameters): logits bf16 [..., V], in_prompt bool [..., V], counts integer
    [..., V] (already saturated), bias fp32 [..., V] or None -> the processed bf16 row(s)."""
    f32 = torch.float32
    x = logits.to(f32)
    b = torch.zeros_like(x) if bias is None else bias.to(f32)
    x = x + b
    c = counts.to(torch.int64).clamp(max=COUNT_MAX)
    seen = in_prompt.to(torch.bool) | (c > 0)
    t_rp, t_inv = torch.tensor(rp, dtype=f32), torch.tensor(inv_rp, dtype=f32)
    x = torch.where(seen, torch.where(x > 0, x * t_inv, x * t_rp), x)
    x = x - torch.tensor(freq, dtype=f32) * c.to(f32)
    x = torch.where(c > 0, x - torch.tensor(pres, dtype=f32), x)
    return x.to(torch.bfloat16)


@torch.inference_mode()
def greedy_reference_processed(model, prompt, n, rp=1.0, freq=0.0, pres=0.0, bias=None):
    """Greedy no-cache recompute with the oracle applied to every step's last row: (tokens, top1 - top2 margins of
    the PROCESSED row). The state is rebuilt from the token lists at every step: the prompt's tokens are "in the
    prompt", every token generated so far is counted."""
    from tests.logprobs_reference import all_rows_logits

    ids, toks, margins = list(prompt), [], []
    vocab = model.arch.vocab_size
    in_prompt = torch.zeros(vocab, dtype=torch.bool)
    in_prompt[torch.tensor(sorted(set(prompt)))] = True
    b = None
    if bias:
        b = torch.zeros(vocab, dtype=torch.float32)
        for t, v in bias.items():
            b[int(t)] = v
    for _ in range(n):
        lg = all_rows_logits(model, ids)[-1].to(torch.bfloat16).cpu()
        counts = torch.zeros(vocab, dtype=torch.int64)
        if toks:
            counts.index_add_(0, torch.tensor(toks), torch.ones(len(toks), dtype=torch.int64))
        out = logit_process(lg, in_prompt, counts, rp, inv_f32(rp), freq, pres, b).float()
        top = torch.topk(out, 2)
        best = float(top.values[0])
        toks.append(int((out == best).nonzero()[0, 0]))  # the lowest index holding the maximum
        margins.append(best - float(top.values[1]))
        ids.append(toks[-1])
    return toks, margins


def agree_until_near_tie(got, want, margins, threshold=0.25):
    """The number of leading steps compared: `got` must equal `want` up to the reference's first near-tie
    (a processed margin below `threshold`), where rounding may legitimately pick the other token."""
    first = next((i for i, m in enumerate(margins) if m < threshold), len(want))
    assert got[:first] == want[:first], (got, want, margins)
    return first
