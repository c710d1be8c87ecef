"""No-cache recomputes for the logprob tests: every row's logits of one eager prefill, and the greedy recompute
of tests/test_engine_gpu.py::reference_with_margins extended to return each step's float64 log_softmax."""

import torch

from src.models.llama import AttnMetadata


@torch.inference_mode()
def all_rows_logits(model, ids, block_size=16):
    """Logits [len(ids), vocab] of one eager all-rows prefill with a fresh KV pool."""
    dev = model.device
    t = len(ids)
    nb = (t + block_size - 1) // block_size
    pool = torch.zeros(model.arch.num_layers, 2, nb, model.hkv, block_size, model.head_dim, dtype=model.dtype,
                       device=dev)
    pos = torch.arange(t, dtype=torch.long, device=dev)
    meta = AttnMetadata(is_prefill=True, slot_mapping=pos.clone(),
                        block_tables=torch.arange(nb, dtype=torch.int32, device=dev)[None],
                        ctx_lens=torch.tensor([t], dtype=torch.int32, device=dev),
                        cu_q=torch.tensor([0, t], dtype=torch.int32, device=dev), max_q_len=t)
    h = model.forward(torch.tensor(ids, dtype=torch.long, device=dev), pos, meta, pool)
    return model.compute_logits(h)


@torch.inference_mode()
def reference_with_logprobs(model, prompt, n):
    """Greedy no-cache recompute: (tokens, top1-top2 logit margins, float64 log_softmax [n, vocab] on the CPU)."""
    ids, toks, margins, lsm = list(prompt), [], [], []
    for _ in range(n):
        lg = all_rows_logits(model, ids)[-1].float()
        top = torch.topk(lg, 2)
        toks.append(int(top.indices[0]))
        margins.append(float(top.values[0] - top.values[1]))
        lsm.append(torch.log_softmax(lg.double(), -1).cpu())
        ids.append(toks[-1])
    return toks, margins, torch.stack(lsm)
