"""
Post-processing: detokenisation and response shaping
(promised at `/root/reference/README.md:35,96-98`, absent from the reference).
"""

from __future__ import annotations

import math
from typing import Any, Dict, List, Optional


def build_llm_output(token_ids: List[int], tokenizer=None, *, prompt_len: int, finish_reason: str,
                     ttft_ms: Optional[float] = None, latency_ms: Optional[float] = None,
                     return_text: bool = True) -> Dict[str, Any]:
    out: Dict[str, Any] = {
        "token_ids": list(token_ids),
        "num_prompt_tokens": prompt_len,
        "num_output_tokens": len(token_ids),
        "finish_reason": finish_reason,
    }
    if return_text and tokenizer is not None:
        out["text"] = tokenizer.decode(token_ids)
    if ttft_ms is not None:
        out["ttft_ms"] = ttft_ms
    if latency_ms is not None:
        out["latency_ms"] = latency_ms
        n = len(token_ids)
        if ttft_ms is not None and n > 1:
            out["tpot_ms"] = (latency_ms - ttft_ms) / (n - 1)
    return out


LOGPROB_FLOOR = -9999.0  # what a non-finite log-probability is written as, so every transport stays valid JSON


def _lp(x: Optional[float]) -> Optional[float]:
    if x is None:
        return None
    return float(x) if math.isfinite(x) else LOGPROB_FLOOR


def logprobs_block(entries: List[Optional[dict]]) -> Dict[str, Any]:
    """The id-based logprob layout of an LLM output, one item per token: entries are the engine's
    ``{"logprob", "rank", "top_ids", "top_logprobs"}`` (None — a prompt's position 0, or an entry the producer
    could not report — stays None in every list)."""
    return {
        "token_logprobs": [None if e is None else _lp(e["logprob"]) for e in entries],
        "ranks": [None if e is None else int(e["rank"]) for e in entries],
        "top_token_ids": [None if e is None else [int(t) for t in e["top_ids"]] for e in entries],
        "top_logprobs": [None if e is None else [_lp(v) for v in e["top_logprobs"]] for e in entries],
    }


def postprocess(outputs: Any) -> Any:
    """Generic hook for non-LLM outputs (identity unless a dict of floats,
    which are rounded for transport)."""
    if isinstance(outputs, dict):
        return {k: (round(v, 6) if isinstance(v, float) else v) for k, v in outputs.items()}
    return outputs
