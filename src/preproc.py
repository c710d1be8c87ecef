"""
Pre-processing: request normalisation and tokenisation
(promised at `/root/reference/README.md:34,96-98`, absent from the reference).

* :class:`ByteTokenizer` — a deterministic byte-level tokenizer that needs no
  files (no network for HF downloads): ids 0/1/2 are pad/bos/eos, byte ``b``
  is id ``b + 3``. A local HF tokenizer directory can be used instead through
  :func:`load_tokenizer`.
* :func:`normalize_request` — validates an LLM request's ``inputs`` and turns
  it into :class:`GenerationInputs`.
* :class:`PreprocPool` — pushes CPU-bound tokenisation to a separate process
  pool ("disaggregated inference": pre/post-processing out of the worker's
  event loop, `README.md:15,96-98`).
"""

from __future__ import annotations

import asyncio
import concurrent.futures as cf
import json
import math
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

PAD_ID, BOS_ID, EOS_ID = 0, 1, 2
_BYTE_OFFSET = 3


class ByteTokenizer:
    """Byte-level tokenizer. Any id ≥ 259 (a random-init model emits them)
    decodes to a byte by folding it into range, so detokenisation is total."""

    def __init__(self, vocab_size: int = 128256):
        self.vocab_size = vocab_size
        self.pad_token_id, self.bos_token_id, self.eos_token_id = PAD_ID, BOS_ID, EOS_ID

    def encode(self, text: str, add_bos: bool = True) -> List[int]:
        ids = [b + _BYTE_OFFSET for b in text.encode("utf-8")]
        return ([BOS_ID] + ids) if add_bos else ids

    def decode(self, ids: Sequence[int], skip_special: bool = True) -> str:
        out = bytearray()
        for i in ids:
            if i < _BYTE_OFFSET:
                if not skip_special:
                    out += b"<" + str(i).encode() + b">"
                continue
            out.append((i - _BYTE_OFFSET) % 256)
        return out.decode("utf-8", errors="replace")


def load_tokenizer(path: Optional[str] = None, vocab_size: int = 128256):
    """A local HuggingFace tokenizer when ``path`` holds one, else ByteTokenizer."""
    if path:
        try:
            from transformers import AutoTokenizer  # type: ignore

            return AutoTokenizer.from_pretrained(path, local_files_only=True)
        except Exception:
            pass
    return ByteTokenizer(vocab_size)


MAX_LOGPROBS = 20  # the OpenAI chat API's cap on top_logprobs
POOLING_MODES = ("last", "mean")  # SamplingParams.pooling
MAX_LOGIT_BIAS = 300  # the OpenAI API's cap on logit_bias entries (launchers.h LOGIT_BIAS_MAX)


def _finite_number(v: Any, name: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{name} must be a finite number")
    return float(v)


@dataclass
class SamplingParams:
    max_tokens: int = 16
    temperature: float = 0.0          # 0 → greedy
    top_k: int = 0                    # 0 → disabled
    top_p: float = 1.0
    seed: Optional[int] = None
    ignore_eos: bool = False
    stop_token_ids: List[int] = field(default_factory=list)
    # log-probabilities of the model's raw distribution (before temperature / top-k / top-p): None = off,
    # 0 = the chosen token's logprob and rank only, 1..20 = also that many most likely tokens
    logprobs: Optional[int] = None
    prompt_logprobs: Optional[int] = None  # the same, for the prompt tokens
    # logit processing (ops.logit_process, applied to the bf16 logits row before anything else reads it):
    # OpenAI's presence / frequency penalties over the generated tokens, the multiplicative repetition penalty
    # over prompt and generated tokens (1.0 = off) and logit_bias {token id: value added to its logit}.
    # For a request that sets any of them, logprobs are computed from the PROCESSED row (still before
    # temperature / top-k / top-p); a request that sets none keeps exactly the raw-distribution meaning above.
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    repetition_penalty: float = 1.0
    logit_bias: Optional[Dict[int, float]] = None
    # constrained decoding (src/guided.py compiles each to a token automaton that ops.token_guide walks on the
    # device; every token outside the automaton's current edge set is barred, its logit -inf). At most one:
    # allowed_token_ids: every step samples only from these ids (no end-of-sequence logic: EOS only if listed);
    # guided_choice: token-id lists, the output is exactly one of them followed by EOS;
    # guided_regex: the decoded output fully matches the pattern (src/guided.py: the byte-level subset), then EOS.
    allowed_token_ids: Optional[List[int]] = None
    guided_choice: Optional[List[List[int]]] = None
    guided_regex: Optional[str] = None
    # JSON mode (the gateway's response_format {"type": "json_object"}): the output is one JSON object, compact or
    # with a single space after ',' and ':', then EOS (src/guided.py: a byte pushdown automaton that ops.json_guide
    # walks on the device). One of the "at most one" fields above.
    guided_json_object: bool = False
    # structured outputs (the gateway's response_format {"type": "json_schema"}): a JSON Schema, a dict or its JSON
    # text; the output is one document valid against it, in JSON mode's text conventions, then EOS
    # (src/guided_schema.py: the supported keywords, everything else is refused by name; ops.schema_guide walks the
    # compiled byte pushdown automaton on the device). One of the "at most one" fields above.
    guided_json: Optional[Any] = None
    # embeddings: with pooling set the request generates nothing. It ends when its prompt does, and its result is
    # the pooled final-norm hidden state of the prompt (ops.pool_embed): "last" = the last prompt token's row,
    # "mean" = the mean over all prompt rows; cut to its first embed_dimensions components (None: all; a multiple
    # of 8), then L2-normalised unless embed_normalize is off. max_tokens is ignored.
    pooling: Optional[str] = None
    embed_normalize: bool = True
    embed_dimensions: Optional[int] = None

    def __post_init__(self):
        if self.max_tokens < 1:
            raise ValueError("max_tokens must be >= 1")
        if self.temperature < 0:
            raise ValueError("temperature must be >= 0")
        if not (0.0 < self.top_p <= 1.0):
            raise ValueError("top_p must be in (0, 1]")
        if self.top_k < 0:
            raise ValueError("top_k must be >= 0")
        for name in ("logprobs", "prompt_logprobs"):
            v = getattr(self, name)
            if v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, int) or not (0 <= v <= MAX_LOGPROBS):
                raise ValueError(f"{name} must be None or an integer in [0, {MAX_LOGPROBS}]")
        for name in ("presence_penalty", "frequency_penalty"):
            v = _finite_number(getattr(self, name), name)
            if not (-2.0 <= v <= 2.0):
                raise ValueError(f"{name} must be in [-2, 2]")
            setattr(self, name, v)
        self.repetition_penalty = _finite_number(self.repetition_penalty, "repetition_penalty")
        if not self.repetition_penalty > 0.0:
            raise ValueError("repetition_penalty must be > 0")
        if self.logit_bias is not None:
            if not isinstance(self.logit_bias, dict):
                raise ValueError("logit_bias must be an object {token id: bias}")
            if len(self.logit_bias) > MAX_LOGIT_BIAS:
                raise ValueError(f"logit_bias holds at most {MAX_LOGIT_BIAS} entries")
            bias: Dict[int, float] = {}
            for k, v in self.logit_bias.items():
                if isinstance(k, str):  # JSON object keys are strings
                    try:
                        k = int(k.strip())
                    except ValueError:
                        raise ValueError(f"logit_bias key {k!r} is not a token id") from None
                if isinstance(k, bool) or not isinstance(k, int) or k < 0:
                    raise ValueError(f"logit_bias key {k!r} is not a token id")
                v = _finite_number(v, "logit_bias value")
                if not (-100.0 <= v <= 100.0):
                    raise ValueError("logit_bias values must be in [-100, 100]")
                if k in bias:
                    raise ValueError(f"logit_bias names token {k} twice")
                bias[k] = v
            self.logit_bias = bias or None
        self._check_guided()
        self._check_pooling()

    def _check_pooling(self) -> None:
        if self.pooling is None:
            if self.embed_dimensions is not None:
                raise ValueError("embed_dimensions needs pooling")
            return
        if self.pooling not in POOLING_MODES:
            raise ValueError(f"pooling must be one of {', '.join(POOLING_MODES)}")
        if not isinstance(self.embed_normalize, bool):
            raise ValueError("embed_normalize must be a boolean")
        d = self.embed_dimensions
        if d is not None and (isinstance(d, bool) or not isinstance(d, int) or d < 8 or d % 8):
            raise ValueError("embed_dimensions must be a positive multiple of 8")
        if self.logprobs is not None or self.prompt_logprobs is not None:
            raise ValueError("pooling cannot be combined with logprobs / prompt_logprobs")
        if self.processes_logits:
            raise ValueError("pooling cannot be combined with penalties or logit_bias")
        if self.guided:
            raise ValueError("pooling cannot be combined with allowed_token_ids / guided_choice / guided_regex / "
                             "guided_json_object / guided_json")

    def _check_guided(self) -> None:
        if not isinstance(self.guided_json_object, bool):
            raise ValueError("guided_json_object must be a boolean")
        if sum(v is not None for v in (self.allowed_token_ids, self.guided_choice, self.guided_regex,
                                       self.guided_json)) + self.guided_json_object > 1:
            raise ValueError("at most one of allowed_token_ids, guided_choice, guided_regex, guided_json_object and "
                             "guided_json may be set")

        def ids_of(v, name):
            if not isinstance(v, (list, tuple)) or not v:
                raise ValueError(f"{name} must be a non-empty list of token ids")
            for t in v:
                if isinstance(t, bool) or not isinstance(t, int) or t < 0:
                    raise ValueError(f"{name}: {t!r} is not a token id")
            return list(v)

        if self.allowed_token_ids is not None:
            ids = ids_of(self.allowed_token_ids, "allowed_token_ids")
            if len(set(ids)) != len(ids):
                raise ValueError("allowed_token_ids names a token twice")
            self.allowed_token_ids = ids
        if self.guided_choice is not None:
            from src.guided import GUIDE_MAX_CHOICE_TOKENS, GUIDE_MAX_CHOICES

            if not isinstance(self.guided_choice, (list, tuple)) or not (1 <= len(self.guided_choice) <= GUIDE_MAX_CHOICES):
                raise ValueError(f"guided_choice must be a list of 1..{GUIDE_MAX_CHOICES} token-id lists")
            seen, out = set(), []
            for c in self.guided_choice:
                c = tuple(ids_of(c, "guided_choice"))
                if c not in seen:  # duplicates removed, the first occurrence's place kept
                    seen.add(c)
                    out.append(list(c))
            if sum(len(c) for c in out) > GUIDE_MAX_CHOICE_TOKENS:
                raise ValueError(f"guided_choice holds more than {GUIDE_MAX_CHOICE_TOKENS} tokens")
            self.guided_choice = out
        if self.guided_regex is not None:
            from src.guided import parse_regex

            parse_regex(self.guided_regex)  # ValueError naming the position for anything outside the subset
        if self.ignore_eos and (self.guided_choice is not None or self.guided_regex is not None):
            raise ValueError("guided_choice / guided_regex cannot be combined with ignore_eos")
        if self.ignore_eos and self.guided_json_object:
            raise ValueError("guided_json_object cannot be combined with ignore_eos")
        if self.guided_json is not None:
            from src.guided import schema_to_pda

            if isinstance(self.guided_json, str):
                try:
                    self.guided_json = json.loads(self.guided_json)
                except ValueError:
                    raise ValueError("guided_json must be a JSON Schema: an object, or its JSON text") from None
            if self.ignore_eos:
                raise ValueError("guided_json cannot be combined with ignore_eos")
            schema_to_pda(self.guided_json)  # table-free compile: a ValueError names the keyword and its pointer

    @property
    def greedy(self) -> bool:
        return self.temperature == 0.0 or self.top_k == 1

    @property
    def processes_logits(self) -> bool:
        """Any penalty or bias set: the request's rows go through ops.logit_process before sampling."""
        return bool(self.presence_penalty != 0.0 or self.frequency_penalty != 0.0 or self.repetition_penalty != 1.0
                    or self.logit_bias)

    @property
    def guided(self) -> bool:
        """Constrained decoding asked for: the request's rows go through ops.token_guide before sampling."""
        return (self.allowed_token_ids is not None or self.guided_choice is not None or self.guided_regex is not None
                or self.guided_json_object or self.guided_json is not None)


@dataclass
class GenerationInputs:
    prompt_token_ids: List[int]
    sampling: SamplingParams
    prompt: Optional[str] = None
    return_text: bool = True


_SAMPLING_KEYS = ("max_tokens", "temperature", "top_k", "top_p", "seed", "ignore_eos", "stop_token_ids",
                  "logprobs", "prompt_logprobs", "presence_penalty", "frequency_penalty", "repetition_penalty",
                  "logit_bias", "allowed_token_ids", "guided_choice", "guided_regex", "guided_json_object", "guided_json",
                  "pooling",
                  "embed_normalize", "embed_dimensions")


def normalize_request(inputs: Any, tokenizer=None, max_model_len: Optional[int] = None) -> GenerationInputs:
    """Accepts a prompt string, a token-id list, or a dict with ``prompt`` /
    ``prompt_token_ids`` plus sampling fields."""
    tok = tokenizer or ByteTokenizer()
    if isinstance(inputs, str):
        inputs = {"prompt": inputs}
    elif isinstance(inputs, (list, tuple)) and all(isinstance(x, int) for x in inputs):
        inputs = {"prompt_token_ids": list(inputs)}
    if not isinstance(inputs, dict):
        raise ValueError("LLM inputs must be a prompt string, a token id list, or an object")
    prompt = inputs.get("prompt")
    ids = inputs.get("prompt_token_ids")
    if ids is None:
        if not isinstance(prompt, str):
            raise ValueError("inputs need 'prompt' (str) or 'prompt_token_ids' (list[int])")
        ids = tok.encode(prompt)
    if not ids:
        raise ValueError("empty prompt")
    ids = list(map(int, ids))  # C-speed conversion + range check: ~0.1 us/token on the serving path
    vs = getattr(tok, "vocab_size", None)
    if vs and (min(ids) < 0 or max(ids) >= vs):
        raise ValueError("prompt token id out of vocabulary range")
    fields = {k: inputs[k] for k in _SAMPLING_KEYS if k in inputs}
    gc = fields.get("guided_choice")
    if isinstance(gc, (list, tuple)) and any(isinstance(c, str) for c in gc):
        # text choices: the canonical tokenisation without BOS; the engine API only ever sees ids
        fields["guided_choice"] = [_encode_plain(tok, c) if isinstance(c, str) else c for c in gc]
    sp = SamplingParams(**fields)
    if vs and sp.logit_bias and max(sp.logit_bias) >= vs:
        raise ValueError("logit_bias token id out of vocabulary range")
    if vs and sp.guided:
        named = sp.allowed_token_ids or [t for c in sp.guided_choice or () for t in c]
        if named and max(named) >= vs:
            raise ValueError("allowed_token_ids / guided_choice token id out of vocabulary range")
    if sp.pooling is not None:  # nothing is generated: only the prompt has to fit
        if inputs.get("stream"):
            raise ValueError("pooling cannot be combined with stream")
        if max_model_len is not None and len(ids) > max_model_len:
            raise ValueError(f"prompt ({len(ids)}) exceeds max_model_len {max_model_len}")
    elif max_model_len is not None and len(ids) + sp.max_tokens > max_model_len:
        raise ValueError(f"prompt ({len(ids)}) + max_tokens ({sp.max_tokens}) exceeds max_model_len {max_model_len}")
    return GenerationInputs(prompt_token_ids=ids, sampling=sp, prompt=prompt,
                            return_text=bool(inputs.get("return_text", True)))


def _encode_plain(tok, text: str) -> List[int]:
    """``text`` as token ids without BOS or any other special token."""
    if isinstance(tok, ByteTokenizer):
        return tok.encode(text, add_bos=False)
    return list(tok.encode(text, add_special_tokens=False))


_POOL_TOKENIZERS: Dict[Tuple[Optional[str], int], Any] = {}


def _pool_tokenizer(path: Optional[str], vocab_size: int):
    """The tokenizer of a pool process (loaded once per process and kept)."""
    key = (path, vocab_size)
    tok = _POOL_TOKENIZERS.get(key)
    if tok is None:
        tok = _POOL_TOKENIZERS[key] = load_tokenizer(path, vocab_size)
    return tok


def _encode_batch(texts: List[str], vocab_size: int, path: Optional[str] = None) -> Tuple[List[List[int]], int]:
    tok = _pool_tokenizer(path, vocab_size)
    return [list(tok.encode(t)) for t in texts], os.getpid()


def _decode_batch(seqs: List[List[int]], vocab_size: int, path: Optional[str] = None) -> Tuple[List[str], int]:
    tok = _pool_tokenizer(path, vocab_size)
    return [tok.decode(s) for s in seqs], os.getpid()


def _warm(path: Optional[str], vocab_size: int) -> int:
    _pool_tokenizer(path, vocab_size)
    return os.getpid()


class PreprocPool:
    """Tokenise / detokenise in separate processes so that the serving loop never spends its own time on it
    (the reference's "pre/post-processing in a separate process", `/root/reference/README.md:15,96-98`).

    Requests that arrive in the same event-loop turn are coalesced into ONE call to the pool (one pickle round
    trip for a burst of prompts), up to ``max_batch`` texts per call. The processes are started with ``spawn``
    (never ``fork``: the worker process holds a HIP context and an engine thread) and warmed at construction, so
    the first request does not pay the interpreter start-up. ``pids`` records which processes did the work."""

    def __init__(self, processes: int = 2, vocab_size: int = 128256, tokenizer_path: Optional[str] = None,
                 max_batch: int = 64):
        import multiprocessing as mp

        self.vocab_size = vocab_size
        self.path = tokenizer_path
        self.max_batch = max_batch
        self._pool = cf.ProcessPoolExecutor(max_workers=processes, mp_context=mp.get_context("spawn"))
        self.pids: set = set()
        self.calls = 0
        self.items = 0
        self._pending: Dict[str, List[Tuple[Any, asyncio.Future]]] = {"enc": [], "dec": []}
        self._tasks: set = set()  # in-flight pool calls (the loop keeps only weak references to tasks)
        self._scheduled: Dict[str, bool] = {"enc": False, "dec": False}
        # start every process now (and load its tokenizer): a cold spawn costs ~0.1-1 s
        warm = [self._pool.submit(_warm, self.path, vocab_size) for _ in range(processes)]
        for f in warm:
            self.pids.add(f.result(timeout=120))

    async def encode(self, texts: List[str]) -> List[List[int]]:
        loop = asyncio.get_running_loop()
        out, pid = await loop.run_in_executor(self._pool, _encode_batch, list(texts), self.vocab_size, self.path)
        self._account(pid, len(texts))
        return out

    async def decode(self, seqs: List[List[int]]) -> List[str]:
        loop = asyncio.get_running_loop()
        out, pid = await loop.run_in_executor(self._pool, _decode_batch, [list(s) for s in seqs], self.vocab_size,
                                              self.path)
        self._account(pid, len(seqs))
        return out

    def _account(self, pid: int, n: int) -> None:
        self.pids.add(pid)
        self.calls += 1
        self.items += n

    # --- coalesced single-item forms (the serving path)
    def encode_one(self, text: str) -> "asyncio.Future":
        return self._enqueue("enc", text)

    def decode_one(self, ids: List[int]) -> "asyncio.Future":
        return self._enqueue("dec", list(ids))

    def _enqueue(self, kind: str, item: Any) -> "asyncio.Future":
        loop = asyncio.get_running_loop()
        fut = loop.create_future()
        self._pending[kind].append((item, fut))
        if not self._scheduled[kind]:
            self._scheduled[kind] = True
            loop.call_soon(self._flush, kind)
        return fut

    def _flush(self, kind: str) -> None:
        self._scheduled[kind] = False
        batch, self._pending[kind] = self._pending[kind], []
        for i in range(0, len(batch), self.max_batch):
            t = asyncio.ensure_future(self._run(kind, batch[i:i + self.max_batch]))
            self._tasks.add(t)
            t.add_done_callback(self._tasks.discard)

    async def _run(self, kind: str, batch: List[Tuple[Any, asyncio.Future]]) -> None:
        items = [x for x, _ in batch]
        try:
            res = await (self.encode(items) if kind == "enc" else self.decode(items))
        except Exception as e:  # noqa: BLE001 — every waiter of the batch gets the failure
            for _, f in batch:
                if not f.done():
                    f.set_exception(e)
            return
        for (_, f), r in zip(batch, res):
            if not f.done():
                f.set_result(r)

    def stats(self) -> Dict[str, Any]:
        return {"processes": sorted(self.pids), "calls": self.calls, "items": self.items}

    def close(self) -> None:
        self._pool.shutdown(wait=False, cancel_futures=True)


def preprocess(inputs: Dict[str, Any]) -> Dict[str, Any]:
    """Generic (non-LLM) normalisation used by the mock path: strip strings,
    lower-case keys."""
    if isinstance(inputs, dict):
        return {str(k).lower(): (v.strip() if isinstance(v, str) else v) for k, v in inputs.items()}
    if isinstance(inputs, str):
        return inputs.strip()  # type: ignore[return-value]
    return inputs


def request_cost(inputs: Any) -> Optional[Tuple[int, int]]:
    """(prompt tokens, max output tokens) of an LLM request as a load balancer can estimate it without the
    worker's tokenizer (text prompts: ~4 bytes per token), or None for other payloads."""
    if not isinstance(inputs, dict):
        return None
    ids = inputs.get("prompt_token_ids")
    if isinstance(ids, list):
        p = len(ids)
    elif isinstance(inputs.get("prompt"), str):
        p = len(inputs["prompt"].encode()) // 4 + 1
    else:
        return None
    if inputs.get("pooling") is not None:  # an embedding request generates nothing
        return p, 0
    try:
        g = int(inputs.get("max_tokens", SamplingParams.max_tokens))
    except (TypeError, ValueError):
        g = SamplingParams.max_tokens
    return p, max(1, g)

