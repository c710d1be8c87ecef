"""
Constrained decoding on the host: three front ends (``allowed_token_ids``, ``guided_choice``, ``guided_regex``)
and ``guided_json_object`` (the third form below). The first three
compile to a token automaton in CSR, which ``ops.token_guide`` walks on the device; a ``guided_regex`` over a
multi-byte vocabulary compiles to the second form below instead.

    row_ptr[S + 1]   edges of state s: [row_ptr[s], row_ptr[s + 1])
    edge_tok[E]      ascending and unique within a state
    edge_next[E]
    start state 0

Invariant: every reachable state has at least one edge (no dead ends), so a step always has a token to draw.

* ``allowed_token_ids``: one state with self-loops.
* ``guided_choice``: a trie; a completed choice has an EOS edge to a sink whose only edge is EOS -> sink (windows
  run past a finished sequence: the sink keeps those steps legal).
* ``guided_regex``: a byte-level subset of regular expressions -> Thompson NFA -> subset construction -> byte DFA
  with unreachable and dead states pruned -> lifted to tokens through a byte table ``token_bytes: id -> bytes |
  None``; accepting states get the EOS edge. The subset: literals (non-ASCII as their UTF-8 bytes), the escapes
  ``\\d \\w \\s \\D \\W \\S \\n \\t \\r`` and ``\\`` + punctuation, ``.``, classes ``[...]`` / ``[^...]`` with
  ranges, groups ``(...)``, ``|`` and the quantifiers ``* + ? {m} {m,} {m,n}``. ``.``, negated classes and the
  upper-case escapes range over ASCII bytes only (``.`` excludes ``\\n``). Anything else is a ValueError naming
  the position.

The second form, ``ByteGuide``: the pruned byte DFA itself (``trans`` int16 [S, 256], ``accept`` uint8 [S]).
``ops.byte_guide`` walks every token's bytes through it inside the decode step, so nothing is lifted on the host:
compile time is ``regex_to_dfa`` alone, memory is S * 512 bytes and no edge cap applies. ``compile_guide`` picks it
for a ``guided_regex`` whose byte table holds an entry longer than one byte (a BPE vocabulary); the single-byte
table keeps the CSR form. State S is a virtual sink: entered by EOS from an accepting state, only EOS is legal in it
and keeps it. A token longer than GUIDE_MAX_TOKEN_BYTES bytes is never allowed — that only narrows the set, and
its bytes can still be spelled by shorter tokens. Every byte that labels a transition must have a single-byte token
other than EOS (checked at compile time): then "no dead ends" carries over from the byte DFA to tokens.
``hf_token_bytes`` derives the byte table of a HuggingFace tokenizer (ByteLevel BPE, or SentencePiece pieces with
byte fallback).

The third form, ``JsonGuide`` (``guided_json_object``, the gateway's ``response_format: {"type": "json_object"}``):
JSON nests, so a byte DFA cannot hold it; the guide is a byte PUSHDOWN automaton, ``trans`` int16 [S, 256] whose
entries carry the next state in bits 0..7 and an action in bits 8..9 (``JSON_ACT_*``: none, push-object, push-array,
pop), -1 for no transition. The configuration is (state, depth, stack bits): bit d - 1 of the stack word is the kind
(0 object, 1 array) of the container at depth d, at most GUIDE_JSON_MAX_DEPTH = 32 open at once. The control
automaton keeps one copy of its value / string / literal / number states per enclosing kind, so the stack is read
only on a pop: a pop entry's state field names the "after a value in an object" state, directly followed by "after a
value in an array" and DONE, and the pop lands on the one the new top (or depth 0) selects. ``ops.json_guide`` walks
every token's bytes through it inside the decode step. The language (``build_json_table``): one object, compact or
with a single space after ``,`` and ``:``, well-formed UTF-8 strings, then only EOS.

No dead ends, from bytes to tokens: (a) every state but DONE has a byte transition that is legal at every depth —
a ``{`` or ``[`` at the cap has no transition, but wherever a value may start, ``"``, a digit, ``t`` ... start one too,
and every other state's transitions do not push; a pop is only reachable with depth >= 1, since the only state at
depth 0 besides DONE is the start state, which pushes; (b) from every configuration DONE is reachable (close what is
open: a string by ``"``, a number by its terminator, a literal by its remaining letters, a container by ``}`` /
``]``, which the per-kind copies make legal exactly in the matching kind); (c) every byte that labels a transition
must have a single-byte token other than EOS (checked at compile time, the ValueError names the byte), so the byte
of (a) is a token the device allows; in DONE, EOS is allowed. Hence every configuration a sequence can reach allows
at least one token, and a finite continuation to DONE then EOS exists.

The fourth form, ``SchemaGuide`` (``guided_json``, the gateway's ``response_format: {"type": "json_schema"}``): a
general byte pushdown automaton whose stack holds RETURN STATES, compiled from a JSON Schema by
src/guided_schema.py (its docstring has the construction, the refusals and the no-dead-end proof). ``trans`` int32
[S, 256]: -1, or the next state in bits 0..13, the return state in bits 14..27 (push only) and the action in bits
28..29 (``SCHEMA_ACT_*``: none, push, pop); ``accept`` uint8 [S]. The configuration is (state, depth, stack): at
most GUIDE_SCHEMA_MAX_DEPTH entries, a push at the cap is no transition, a pop goes to the popped return state. EOS
is legal when the state accepts and the depth is 0. A token that would hold more than GUIDE_SCHEMA_TOKEN_PUSHES of
its own not-yet-popped pushes at once is never allowed: like the byte cap this only narrows the set (its bytes can
be spelled by shorter tokens, and a single-byte token pushes at most once), and it lets the device keep a chain's
pushes in one 64-bit register. ``ops.schema_guide`` walks every token's bytes through it inside the decode step.

Pure numpy / Python: imported by ``src.preproc`` for early validation, never touches torch.
"""

from __future__ import annotations

import collections
import threading
from dataclasses import dataclass
from typing import Dict, FrozenSet, Iterable, List, Optional, Sequence, Tuple

import numpy as np

# per-request caps (csrc/kernels/launchers.h GUIDE_MAX_STATES / GUIDE_MAX_EDGES)
GUIDE_MAX_STATES = 16384
GUIDE_MAX_EDGES = 262144           # twice the largest vocabulary
GUIDE_MAX_CHOICES = 1024
GUIDE_MAX_CHOICE_TOKENS = 65536
GUIDE_MAX_TOKEN_BYTES = 32         # ops.byte_guide never allows a longer token (launchers.h)
GUIDE_JSON_MAX_DEPTH = 32          # containers open at once, the top-level object included (launchers.h)
GUIDE_JSON_MAX_STATES = 92         # ops.json_guide keeps the whole table in LDS (launchers.h)
JSON_ACT_NONE, JSON_ACT_PUSH_OBJECT, JSON_ACT_PUSH_ARRAY, JSON_ACT_POP = 0, 1, 2, 3   # bits 8..9 of a trans entry
GUIDE_SCHEMA_MAX_DEPTH = 32        # return states live at once in a SchemaGuide's stack (launchers.h)
GUIDE_SCHEMA_TOKEN_PUSHES = 4      # a token never holds more of its own not-yet-popped pushes (launchers.h)
SCHEMA_ACT_NONE, SCHEMA_ACT_PUSH, SCHEMA_ACT_POP = 0, 1, 2   # bits 28..29 of a SchemaGuide's trans entry
_SCHEMA_STATE_BITS = 14            # next state in bits 0..13, return state in bits 14..27
_SCHEMA_STATE_MASK = (1 << _SCHEMA_STATE_BITS) - 1
_SCHEMA_BOUND_MAX = 256            # minItems / maxItems / minLength / maxLength
_QUANT_MAX = 1024                  # {m,n} bound: larger counts only ever end at the state cap


@dataclass(frozen=True, eq=False)
class Automaton:
    row_ptr: np.ndarray    # int32 [S + 1]
    edge_tok: np.ndarray   # int32 [E]
    edge_next: np.ndarray  # int32 [E]
    key: tuple             # the canonical spec it was compiled from (arena regions are shared by it)

    @property
    def n_states(self) -> int:
        return len(self.row_ptr) - 1

    @property
    def n_edges(self) -> int:
        return len(self.edge_tok)

    def edges(self, state: int) -> Tuple[np.ndarray, np.ndarray]:
        lo, hi = int(self.row_ptr[state]), int(self.row_ptr[state + 1])
        return self.edge_tok[lo:hi], self.edge_next[lo:hi]


@dataclass(frozen=True, eq=False)
class ByteGuide:
    trans: np.ndarray      # int16 [S, 256], -1: no transition; start state 0
    accept: np.ndarray     # uint8 [S]
    eos: int
    key: tuple             # the canonical spec; its last element names the byte table (id_of / table_of)

    @property
    def n_states(self) -> int:
        return self.trans.shape[0]

    @property
    def sink(self) -> int:
        return self.trans.shape[0]


def walk_bytes(guide: ByteGuide, state: int, tokens: Iterable[int],
               token_bytes: Optional[Sequence[Optional[bytes]]] = None) -> int:
    """``walk`` for a ByteGuide, by the device's rules (csrc/kernels/byte_guide.hip): EOS from an accepting state
    or in the sink gives the sink; any other token walks its bytes. A ValueError where the device would report
    GUIDE_ERR_NO_EDGE."""
    if token_bytes is None:
        token_bytes = table_of(guide.key[-1])
    n = guide.n_states
    for t in tokens:
        t = int(t)
        if t == guide.eos:
            if state != n and not guide.accept[state]:
                raise ValueError(f"end of sequence in guide state {state}, which does not accept")
            state = n
            continue
        bs = token_bytes[t] if 0 <= t < len(token_bytes) else None
        if state == n or not bs or len(bs) > GUIDE_MAX_TOKEN_BYTES:
            raise ValueError(f"token {t} has no edge in guide state {state}")
        s = state
        for b in bs:
            s = int(guide.trans[s, b])
            if s < 0:
                raise ValueError(f"token {t} has no edge in guide state {state}")
        state = s
    return state


@dataclass(frozen=True, eq=False)
class JsonGuide:
    trans: np.ndarray      # int16 [S, 256]: -1, or next state | action << 8 (module docstring); start state 0
    done: int              # the only accepting state
    eos: int
    key: tuple             # the canonical spec; its last element names the byte table (id_of / table_of)

    @property
    def n_states(self) -> int:
        return self.trans.shape[0]

    @property
    def sink(self) -> int:
        return self.trans.shape[0]


def json_step(trans: np.ndarray, config: Tuple[int, int, int], byte: int) -> Optional[Tuple[int, int, int]]:
    """One byte from (state, depth, stack bits) by the device's rules; None: no transition, or a push at the cap."""
    s, d, k = config
    v = int(trans[s, byte])
    if v < 0:
        return None
    nxt, act = v & 0xFF, v >> 8
    if act == JSON_ACT_PUSH_OBJECT or act == JSON_ACT_PUSH_ARRAY:
        if d >= GUIDE_JSON_MAX_DEPTH:
            return None
        if act == JSON_ACT_PUSH_ARRAY:
            k |= 1 << d
        d += 1
    elif act == JSON_ACT_POP:
        if d < 1:
            raise ValueError("the JSON guide pops an empty stack")
        d -= 1
        k &= ~(1 << d)
        nxt += 2 if d == 0 else (k >> (d - 1)) & 1
    return nxt, d, k


def walk_json(guide: JsonGuide, config: Tuple[int, int, int], tokens: Iterable[int],
              token_bytes: Optional[Sequence[Optional[bytes]]] = None) -> Tuple[int, int, int]:
    """``walk`` for a JsonGuide over (state, depth, stack bits), by the device's rules
    (csrc/kernels/json_guide.hip): EOS from DONE or in the sink gives the sink; any other token walks its bytes,
    pushes and pops applied. A ValueError where the device would report GUIDE_ERR_NO_EDGE."""
    if token_bytes is None:
        token_bytes = table_of(guide.key[-1])
    n = guide.n_states
    for t in tokens:
        t = int(t)
        if t == guide.eos:
            if config[0] != n and config[0] != guide.done:
                raise ValueError(f"end of sequence in guide state {config[0]}, which does not accept")
            config = (n, config[1], config[2])
            continue
        bs = token_bytes[t] if 0 <= t < len(token_bytes) else None
        if config[0] == n or not bs or len(bs) > GUIDE_MAX_TOKEN_BYTES:
            raise ValueError(f"token {t} has no edge in guide state {config[0]}")
        c = config
        for b in bs:
            c = json_step(guide.trans, c, b)
            if c is None:
                raise ValueError(f"token {t} has no edge in guide state {config[0]}")
        config = c
    return config


@dataclass(frozen=True, eq=False)
class SchemaGuide:
    trans: np.ndarray      # int32 [S, 256]: -1, or next | return state << 14 | action << 28; start state 0
    accept: np.ndarray     # uint8 [S]
    eos: int
    key: tuple             # the canonical spec; its last element names the byte table (id_of / table_of)

    @property
    def n_states(self) -> int:
        return self.trans.shape[0]

    @property
    def sink(self) -> int:
        return self.trans.shape[0]


def schema_step(trans: np.ndarray, config: Tuple[int, int, tuple], byte: int,
                held: int = 0) -> Optional[Tuple[Tuple[int, int, tuple], int]]:
    """One byte from (state, depth, stack of return states) by the device's rules; ``held``: the pushes of the
    running token that are still on the stack. ((state, depth, stack), held), or None: no transition, a push at the
    depth cap or beyond the token's push cap."""
    s, d, stk = config
    v = int(trans[s, byte])
    if v < 0:
        return None
    act = v >> 28
    if act == SCHEMA_ACT_PUSH:
        if d >= GUIDE_SCHEMA_MAX_DEPTH or held >= GUIDE_SCHEMA_TOKEN_PUSHES:
            return None
        return (v & _SCHEMA_STATE_MASK, d + 1, stk + ((v >> _SCHEMA_STATE_BITS) & _SCHEMA_STATE_MASK,)), held + 1
    if act == SCHEMA_ACT_POP:
        if d < 1:
            raise ValueError("the schema guide pops an empty stack")
        return (stk[-1], d - 1, stk[:-1]), max(held - 1, 0)
    return (v & _SCHEMA_STATE_MASK, d, stk), held


def walk_schema(guide: SchemaGuide, config: Tuple[int, int, tuple], tokens: Iterable[int],
                token_bytes: Optional[Sequence[Optional[bytes]]] = None) -> Tuple[int, int, tuple]:
    """``walk`` for a SchemaGuide over (state, depth, stack of return states), by the device's rules
    (csrc/kernels/schema_guide.hip): EOS from an accepting state at depth 0 or in the sink gives the sink; any other
    token walks its bytes, pushes and pops applied, never more than GUIDE_SCHEMA_TOKEN_PUSHES of its own pushes
    held. A ValueError where the device would report GUIDE_ERR_NO_EDGE."""
    if token_bytes is None:
        token_bytes = table_of(guide.key[-1])
    n = guide.n_states
    for t in tokens:
        t = int(t)
        if t == guide.eos:
            if config[0] != n and not (guide.accept[config[0]] and config[1] == 0):
                raise ValueError(f"end of sequence in guide state {config[0]}, which does not accept")
            config = (n, config[1], config[2])
            continue
        bs = token_bytes[t] if 0 <= t < len(token_bytes) else None
        if config[0] == n or not bs or len(bs) > GUIDE_MAX_TOKEN_BYTES:
            raise ValueError(f"token {t} has no edge in guide state {config[0]}")
        c, held = config, 0
        for b in bs:
            r = schema_step(guide.trans, c, b, held)
            if r is None:
                raise ValueError(f"token {t} has no edge in guide state {config[0]}")
            c, held = r
        config = c
    return config


def walk(automaton, state, tokens: Iterable[int]):
    """The state after ``tokens`` from ``state`` (a JsonGuide: the configuration (state, depth, stack bits); start
    state 0 stands for (0, 0, 0); a SchemaGuide: (state, depth, stack of return states), 0 for (0, 0, ())). A token
    without an edge is a ValueError: the runner rebuilds
    device state from tokens the automaton itself allowed, so this never happens to a healthy sequence."""
    if isinstance(automaton, SchemaGuide):
        return walk_schema(automaton, (0, 0, ()) if isinstance(state, int) and state == 0 else state, tokens)
    if isinstance(automaton, JsonGuide):
        return walk_json(automaton, (0, 0, 0) if isinstance(state, int) and state == 0 else state, tokens)
    if isinstance(automaton, ByteGuide):
        return walk_bytes(automaton, state, tokens)
    for t in tokens:
        toks, nxt = automaton.edges(state)
        i = int(np.searchsorted(toks, t))
        if i >= len(toks) or int(toks[i]) != int(t):
            raise ValueError(f"token {int(t)} has no edge in guide state {state}")
        state = int(nxt[i])
    return state


def _check_caps(n_states: int, n_edges: int) -> None:
    if n_states > GUIDE_MAX_STATES:
        raise ValueError(f"the guide's automaton has more than {GUIDE_MAX_STATES} states")
    if n_edges > GUIDE_MAX_EDGES:
        raise ValueError(f"the guide's automaton has more than {GUIDE_MAX_EDGES} edges")


def _from_state_edges(per_state: List[Dict[int, int]], key: tuple) -> Automaton:
    """CSR from {token: next} per state (start = 0)."""
    n_edges = sum(len(e) for e in per_state)
    _check_caps(len(per_state), n_edges)
    row_ptr = np.zeros(len(per_state) + 1, dtype=np.int32)
    tok = np.empty(n_edges, dtype=np.int32)
    nxt = np.empty(n_edges, dtype=np.int32)
    at = 0
    for s, e in enumerate(per_state):
        if not e:
            raise AssertionError("guide state without an edge")
        ks = sorted(e)
        tok[at:at + len(ks)] = ks
        nxt[at:at + len(ks)] = [e[k] for k in ks]
        at += len(ks)
        row_ptr[s + 1] = at
    return Automaton(row_ptr, tok, nxt, key)


# ------------------------------------------------------------------ allowed_token_ids / guided_choice
def _check_vocab(ids: Iterable[int], vocab: Optional[int], what: str) -> None:
    if vocab is not None:
        for t in ids:
            if not 0 <= t < vocab:
                raise ValueError(f"{what} token id {t} outside [0, {vocab})")


def compile_allowed(ids: Sequence[int], vocab: Optional[int] = None) -> Automaton:
    ids = sorted(set(int(t) for t in ids))
    if not ids:
        raise ValueError("allowed_token_ids must not be empty")
    _check_vocab(ids, vocab, "allowed_token_ids")
    return _from_state_edges([{t: 0 for t in ids}], ("allowed", tuple(ids)))


def compile_choice(choices: Sequence[Sequence[int]], eos: int, vocab: Optional[int] = None) -> Automaton:
    canon = sorted(set(tuple(int(t) for t in c) for c in choices))
    if not canon or any(not c for c in canon):
        raise ValueError("guided_choice needs at least one choice and no empty one")
    for c in canon:
        _check_vocab(c, vocab, "guided_choice")
        if eos in c:
            raise ValueError("a guided_choice must not contain the end-of-sequence token")
    states: List[Dict[int, int]] = [{}]
    ends = []
    for c in canon:
        s = 0
        for t in c:
            n = states[s].get(t)
            if n is None:
                n = len(states)
                states.append({})
                states[s][t] = n
                if n >= GUIDE_MAX_STATES:
                    _check_caps(n + 2, 0)
            s = n
        ends.append(s)
    sink = len(states)
    states.append({eos: sink})
    for s in ends:
        states[s][eos] = sink
    return _from_state_edges(states, ("choice", tuple(canon), int(eos)))


# ------------------------------------------------------------------ guided_regex: parser
_ASCII = frozenset(range(128))
_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset(list(range(0x30, 0x3A)) + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + [0x5F])
_SPACE = frozenset(b" \t\n\r\f\v")
_ESC_CLASS = {"d": _DIGIT, "w": _WORD, "s": _SPACE, "D": _ASCII - _DIGIT, "W": _ASCII - _WORD, "S": _ASCII - _SPACE}
_ESC_CHAR = {"n": 0x0A, "t": 0x09, "r": 0x0D}
_PUNCT = frozenset("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~")

# AST: ("set", frozenset of bytes) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)


class _Parser:
    def __init__(self, pattern: str):
        self.p = pattern
        self.i = 0

    def err(self, what: str, pos: Optional[int] = None):
        raise ValueError(f"guided_regex: {what} at position {self.i if pos is None else pos}")

    def peek(self) -> Optional[str]:
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.err("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        at = self.i
        node = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "?":
                m, n = 0, 1
            elif c == "{":
                m, n = self.braces()
            else:
                return node
            if c != "{":
                self.i += 1
            if self.peek() == "?":
                self.err("lazy quantifiers are not supported")
            if self.peek() == "+":
                self.err("possessive quantifiers are not supported")
            if self.peek() in ("*", "{"):
                self.err("a quantifier cannot follow a quantifier")
            node = ("rep", node, m, n)
        return node

    def braces(self) -> Tuple[int, Optional[int]]:
        start = self.i
        self.i += 1
        m = self.number()
        if m is None:
            self.err("'{' must open a quantifier {m}, {m,} or {m,n}", start)
        n: Optional[int] = m
        if self.peek() == ",":
            self.i += 1
            n = self.number()
        if self.peek() != "}":
            self.err("unterminated quantifier", start)
        self.i += 1
        if n is not None and n < m:
            self.err("quantifier {m,n} with n < m", start)
        if m > _QUANT_MAX or (n is not None and n > _QUANT_MAX):
            self.err(f"quantifier count above {_QUANT_MAX}", start)
        return m, n

    def number(self) -> Optional[int]:
        j = self.i
        while self.i < len(self.p) and self.p[self.i] in "0123456789":
            self.i += 1
        return int(self.p[j:self.i]) if self.i > j else None

    def escape(self, in_class: bool):
        """After the backslash: a byte set (class escape) or a single byte."""
        at = self.i - 1
        c = self.peek()
        if c is None:
            self.err("a pattern cannot end in '\\'", at)
        self.i += 1
        if c in _ESC_CLASS:
            return _ESC_CLASS[c]
        if c in _ESC_CHAR:
            return frozenset([_ESC_CHAR[c]])
        if c in _PUNCT:
            return frozenset([ord(c)])
        if c in "0123456789":
            self.err("backreferences are not supported", at)
        if c in "AbBZzG":
            self.err("anchors are not supported", at)
        self.err(f"unsupported escape '\\{c}'", at)

    def atom(self):
        c = self.peek()
        at = self.i
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                nxt = self.p[self.i + 1: self.i + 3]
                if nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                    self.err("lookaround is not supported", at)
                if nxt[:1] in ("P", "<") or nxt[:1] == ":":
                    self.err("only plain groups (...) are supported", at)
                self.err("flags are not supported", at)
            node = self.alt()
            if self.peek() != ")":
                self.err("unterminated group", at)
            self.i += 1
            return node
        if c == "[":
            return ("set", self.char_class())
        if c == ".":
            self.i += 1
            return ("set", _ASCII - {0x0A})
        if c in ("^", "$"):
            self.err("anchors are not supported (the whole output is matched)")
        if c in "*+?{":
            self.err("a quantifier with nothing to repeat")
        if c in "]}":
            self.err(f"unbalanced '{c}'")
        self.i += 1
        if c == "\\":
            return ("set", self.escape(False))
        b = c.encode("utf-8")
        if len(b) == 1:
            return ("set", frozenset(b))
        return ("cat", [("set", frozenset([x])) for x in b])

    def class_item(self):
        """One member of a class: (byte or None, set). A single byte can open a range."""
        c = self.peek()
        if c is None:
            return None
        if c == "\\":
            self.i += 1
            s = self.escape(True)
            return (next(iter(s)) if len(s) == 1 and self.p[self.i - 1] not in _ESC_CLASS else None), s
        if ord(c) > 127:
            self.err("non-ASCII characters are not supported inside a class")
        if c == "[" and self.p[self.i + 1: self.i + 2] == ":":
            self.err("POSIX classes are not supported")
        self.i += 1
        return ord(c), frozenset([ord(c)])

    def char_class(self) -> FrozenSet[int]:
        start = self.i
        self.i += 1
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        members: set = set()
        first = True
        while True:
            c = self.peek()
            if c is None:
                self.err("unterminated class", start)
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            at = self.i
            lo, s = self.class_item()
            if self.peek() == "-" and self.p[self.i + 1: self.i + 2] not in ("]", ""):
                if lo is None:
                    self.err("a class escape cannot open a range", at)
                self.i += 1
                hi, _ = self.class_item()
                if hi is None:
                    self.err("a class escape cannot close a range", at)
                if hi < lo:
                    self.err("reversed range in a class", at)
                members.update(range(lo, hi + 1))
            else:
                members.update(s)
        out = frozenset(members)
        if negate:
            out = _ASCII - out
        if not out:
            self.err("a class that matches nothing", start)
        return out


def parse_regex(pattern: str):
    """The pattern's AST; ValueError (naming the position) for anything outside the supported subset."""
    if not isinstance(pattern, str) or not pattern:
        raise ValueError("guided_regex must be a non-empty string")
    return _Parser(pattern).parse()


# ------------------------------------------------------------------ guided_regex: NFA -> DFA
class _NFA:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.trans: List[List[Tuple[FrozenSet[int], int]]] = []

    def state(self) -> int:
        if len(self.eps) > 64 * GUIDE_MAX_STATES:
            raise ValueError(f"the guide's automaton has more than {GUIDE_MAX_STATES} states")
        self.eps.append([])
        self.trans.append([])
        return len(self.eps) - 1

    def build(self, node) -> Tuple[int, int]:
        """Thompson fragment (entry, exit) of an AST node."""
        kind = node[0]
        if kind == "set":
            a, b = self.state(), self.state()
            self.trans[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.state()
            for item in node[1]:
                x, y = self.build(item)
                self.eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = self.state(), self.state()
            for br in node[1]:
                x, y = self.build(br)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, m, n = node
        a = b = self.state()
        for _ in range(m):
            x, y = self.build(sub)
            self.eps[b].append(x)
            b = y
        if n is None:  # sub*
            x, y = self.build(sub)
            hub = self.state()
            self.eps[b].append(hub)
            self.eps[hub].append(x)
            self.eps[y].append(hub)
            return a, hub
        end = self.state()
        for _ in range(n - m):  # (sub(sub(...)?)?)?
            x, y = self.build(sub)
            self.eps[b].append(end)
            self.eps[b].append(x)
            b = y
        self.eps[b].append(end)
        return a, end


def _reach(n: int, src: np.ndarray, dst: np.ndarray, seeds: np.ndarray) -> np.ndarray:
    """bool [n]: the nodes reachable from `seeds` over the edges src -> dst (breadth first, every edge once)."""
    order = np.argsort(src, kind="stable")
    d = np.asarray(dst)[order]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=ptr[1:])
    seen = np.zeros(n, dtype=bool)
    front = np.unique(np.asarray(seeds, dtype=np.int64))
    seen[front] = True
    while len(front):
        cnt = ptr[front + 1] - ptr[front]
        total = int(cnt.sum())
        if not total:
            break
        first = np.repeat(ptr[front] - (np.cumsum(cnt) - cnt), cnt)
        nb = np.unique(d[first + np.arange(total)])
        front = nb[~seen[nb]]
        seen[front] = True
    return seen


def regex_to_dfa(pattern: str) -> Tuple[np.ndarray, np.ndarray]:
    """(trans int32 [S, 256] with -1 = no transition, accepting bool [S]) of the pruned byte DFA, start state 0:
    every state is reachable and can reach an accepting one. ValueError: unsupported syntax, a pattern that
    matches nothing, more than GUIDE_MAX_STATES states."""
    nfa = _NFA()
    entry, exit_ = nfa.build(parse_regex(pattern))

    def closure(states) -> FrozenSet[int]:
        seen = set(states)
        stack = list(states)
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    start = closure([entry])
    index = {start: 0}
    order = [start]
    rows: List[List[int]] = []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        by_byte: Dict[int, set] = {}
        for s in cur:
            for bs, t in nfa.trans[s]:
                for b in bs:
                    by_byte.setdefault(b, set()).add(t)
        row = [-1] * 256
        memo: Dict[FrozenSet[int], int] = {}
        for b, targets in by_byte.items():
            tk = frozenset(targets)
            j = memo.get(tk)
            if j is None:
                cl = closure(tk)
                j = index.get(cl)
                if j is None:
                    j = index[cl] = len(order)
                    order.append(cl)
                    if len(order) > GUIDE_MAX_STATES:
                        raise ValueError(f"the guide's automaton has more than {GUIDE_MAX_STATES} states")
                memo[tk] = j
            row[b] = j
        rows.append(row)
    trans = np.asarray(rows, dtype=np.int32).reshape(len(order), 256)
    accept = np.fromiter((exit_ in s for s in order), dtype=bool, count=len(order))
    # dead states: those that reach no accepting state (reachability over the reversed transitions)
    frm, byte = np.nonzero(trans >= 0)
    live = _reach(len(order), trans[frm, byte], frm, np.nonzero(accept)[0])
    if not live[0]:
        raise ValueError("guided_regex matches nothing")
    renum = np.full(len(order), -1, dtype=np.int32)
    renum[live] = np.arange(int(live.sum()), dtype=np.int32)  # state 0 stays 0: it is live and first
    trans = np.where(trans >= 0, renum[np.maximum(trans, 0)], -1)[live].astype(np.int32)
    return trans, accept[live]


def dfa_accepts(trans: np.ndarray, accept: np.ndarray, data: bytes) -> bool:
    s = 0
    for b in data:
        s = int(trans[s, b])
        if s < 0:
            return False
    return bool(accept[s])


def byte_table(vocab: int) -> List[Optional[bytes]]:
    """ByteTokenizer's table: ids 3..258 are one byte each, everything else has no bytes."""
    return [bytes([i - 3]) if 3 <= i < 259 and i < vocab else None for i in range(min(vocab, 259))] + \
        [None] * max(0, vocab - 259)


def compile_regex(pattern: str, token_bytes: Sequence[Optional[bytes]], eos: int,
                  vocab: Optional[int] = None) -> Automaton:
    trans, accept = regex_to_dfa(pattern)
    n = trans.shape[0]
    vocab = len(token_bytes) if vocab is None else min(vocab, len(token_bytes))
    src_l, tok_l, nxt_l = [], [], []
    all_states = np.arange(n, dtype=np.int32)
    for t in range(vocab):
        bs = token_bytes[t]
        if not bs or t == eos:
            continue
        st = all_states
        for b in bs:
            st = np.where(st >= 0, trans[np.maximum(st, 0), b], -1)
        ok = np.nonzero(st >= 0)[0]
        if len(ok):
            src_l.append(ok.astype(np.int32))
            tok_l.append(np.full(len(ok), t, dtype=np.int32))
            nxt_l.append(st[ok].astype(np.int32))
    sink = n
    acc = np.nonzero(accept)[0].astype(np.int32)
    src_l += [acc, np.asarray([sink], dtype=np.int32)]
    tok_l += [np.full(len(acc), eos, dtype=np.int32), np.asarray([eos], dtype=np.int32)]
    nxt_l += [np.full(len(acc), sink, dtype=np.int32), np.asarray([sink], dtype=np.int32)]
    src, tok, nxt = np.concatenate(src_l), np.concatenate(tok_l), np.concatenate(nxt_l)
    # the byte DFA has no dead state, but a byte without a token can leave one in the token automaton: keep the
    # states that still reach the sink, then those reachable from the start
    good = _reach(n + 1, nxt, src, np.asarray([sink]))
    if not good[0]:
        raise ValueError("guided_regex matches nothing this tokenizer can produce")
    keep = good[src] & good[nxt]
    src, tok, nxt = src[keep], tok[keep], nxt[keep]
    reach = _reach(n + 1, src, nxt, np.asarray([0]))
    keep = reach[src]
    src, tok, nxt = src[keep], tok[keep], nxt[keep]
    renum = np.full(n + 1, -1, dtype=np.int32)
    renum[reach] = np.arange(int(reach.sum()), dtype=np.int32)
    src, nxt = renum[src], renum[nxt]
    n_states = int(reach.sum())
    _check_caps(n_states, len(src))
    order = np.lexsort((tok, src))
    src, tok, nxt = src[order], tok[order], nxt[order]
    row_ptr = np.zeros(n_states + 1, dtype=np.int32)
    np.cumsum(np.bincount(src, minlength=n_states), out=row_ptr[1:])
    return Automaton(row_ptr, tok.astype(np.int32), nxt.astype(np.int32), ("regex", pattern, int(eos), id_of(token_bytes)))


_TABLE_IDS: Dict[int, tuple] = {}
_TABLES: List[Sequence[Optional[bytes]]] = []   # by id_of
_TABLE_FACTS: Dict[tuple, tuple] = {}


def id_of(token_bytes) -> int:
    """A small stable number per byte-table object (a cache key must not hold, or hash, a 128K-entry table); the
    table is kept alive so that its identity cannot be reused."""
    ent = _TABLE_IDS.get(id(token_bytes))
    if ent is None:
        ent = _TABLE_IDS[id(token_bytes)] = (token_bytes, len(_TABLE_IDS))
        _TABLES.append(token_bytes)
    return ent[1]


def table_of(table_id: int) -> Sequence[Optional[bytes]]:
    """The byte table that id_of numbered ``table_id`` (a ByteGuide's key ends in it)."""
    return _TABLES[table_id]


def _table_facts(token_bytes, eos: int, vocab: int) -> tuple:
    """(an entry is longer than one byte, the bytes that have a single-byte token other than EOS) of the table's
    first ``vocab`` entries: one pass per table, kept."""
    k = (id_of(token_bytes), int(eos), int(vocab))
    f = _TABLE_FACTS.get(k)
    if f is None:
        multi, single = False, set()
        for t in range(min(vocab, len(token_bytes))):
            bs = token_bytes[t]
            if not bs:
                continue
            if len(bs) > 1:
                multi = True
            elif t != eos:
                single.add(bs[0])
        f = _TABLE_FACTS[k] = (multi, frozenset(single))
    return f


def compile_byte_guide(pattern: str, token_bytes: Sequence[Optional[bytes]], eos: int,
                       vocab: Optional[int] = None) -> ByteGuide:
    """The ByteGuide of a pattern: regex_to_dfa and the soundness check, nothing per token. ValueError: what
    regex_to_dfa refuses, and a byte on a transition that no single-byte token (other than EOS) spells — a state
    could then be left without any legal token."""
    trans, accept = regex_to_dfa(pattern)
    vocab = len(token_bytes) if vocab is None else min(vocab, len(token_bytes))
    _, single = _table_facts(token_bytes, eos, vocab)
    used = np.nonzero((trans >= 0).any(axis=0))[0]
    for b in used:
        if int(b) not in single:
            raise ValueError(f"guided_regex needs byte 0x{int(b):02X}, which is not supported on this tokenizer: no "
                             "single-byte token spells it")
    return ByteGuide(np.ascontiguousarray(trans, dtype=np.int16), np.ascontiguousarray(accept, dtype=np.uint8),
                     int(eos), ("regex", pattern, int(eos), id_of(token_bytes)))


# ------------------------------------------------------------------ guided_json_object: the pushdown table
def build_json_table() -> Tuple[np.ndarray, int]:
    """(trans int16 [S, 256], DONE) of the JSON-object pushdown automaton described in the module docstring; start
    state 0. Value, string, literal and number states exist once per enclosing kind ("o": in an object, "a": in an
    array); the key string is a third copy. States after_o, after_a and DONE are consecutive: a pop lands on
    after_o + (0: the new top is an object, 1: an array, 2: depth 0)."""
    names: List[str] = []
    rows: List[List[int]] = []

    def st(name: str) -> int:
        names.append(name)
        rows.append([-1] * 256)
        return len(rows) - 1

    def edge(a: int, bs, b: int, act: int = JSON_ACT_NONE) -> None:
        for x in (bs if not isinstance(bs, int) else [bs]):
            x = x if isinstance(x, int) else ord(x)
            assert rows[a][x] == -1, (names[a], x)
            rows[a][x] = b | (act << 8)

    start = st("start")
    after = {"o": st("after_o"), "a": st("after_a")}
    done = st("done")
    assert (after["o"], after["a"], done) == (1, 2, 3)
    obj_open, key_end, colon, colon_sp = st("obj_open"), st("key_end"), st("colon"), st("colon_sp")
    comma_o, comma_o_sp = st("comma_o"), st("comma_o_sp")
    arr_open, comma_a, comma_a_sp = st("arr_open"), st("comma_a"), st("comma_a_sp")
    hexd = "0123456789abcdefABCDEF"

    def string(tag: str, end: int) -> int:
        """The states of a string whose opening quote was read; `end` follows the closing one. Returns the body."""
        body, esc = st("str_" + tag), st("esc_" + tag)
        u = [st(f"u{i}_{tag}") for i in range(4)]
        c1, c2, c3 = st("c1_" + tag), st("c2_" + tag), st("c3_" + tag)   # 1, 2, 3 continuation bytes to go
        e0, ed, f0, f4 = st("e0_" + tag), st("ed_" + tag), st("f0_" + tag), st("f4_" + tag)
        edge(body, [b for b in range(0x20, 0x80) if b not in (0x22, 0x5C)], body)
        edge(body, '"', end)
        edge(body, "\\", esc)
        edge(esc, '"\\/bfnrt', body)
        edge(esc, "u", u[0])
        for i in range(4):
            edge(u[i], hexd, u[i + 1] if i < 3 else body)
        cont = range(0x80, 0xC0)
        edge(body, range(0xC2, 0xE0), c1)                       # C0, C1: overlong
        edge(body, 0xE0, e0)
        edge(body, [b for b in range(0xE1, 0xF0) if b != 0xED], c2)
        edge(body, 0xED, ed)
        edge(body, 0xF0, f0)
        edge(body, range(0xF1, 0xF4), c3)
        edge(body, 0xF4, f4)                                    # F5..: above U+10FFFF
        edge(c1, cont, body)
        edge(c2, cont, c1)
        edge(c3, cont, c2)
        edge(e0, range(0xA0, 0xC0), c1)                         # E0 80..9F: overlong
        edge(ed, range(0x80, 0xA0), c1)                         # ED A0..BF: surrogates
        edge(f0, range(0x90, 0xC0), c2)                         # F0 80..8F: overlong
        edge(f4, range(0x80, 0x90), c2)                         # F4 90..: above U+10FFFF
        return body

    key = string("k", key_end)
    edge(start, "{", obj_open, JSON_ACT_PUSH_OBJECT)
    edge(obj_open, '"', key)
    edge(obj_open, "}", after["o"], JSON_ACT_POP)
    edge(key_end, ":", colon)
    edge(colon, " ", colon_sp)
    edge(after["o"], ",", comma_o)
    edge(after["o"], "}", after["o"], JSON_ACT_POP)
    edge(comma_o, " ", comma_o_sp)
    edge(comma_o, '"', key)
    edge(comma_o_sp, '"', key)
    edge(arr_open, "]", after["o"], JSON_ACT_POP)
    edge(after["a"], ",", comma_a)
    edge(after["a"], "]", after["o"], JSON_ACT_POP)
    edge(comma_a, " ", comma_a_sp)
    digits = "0123456789"
    for kind, value_starts in (("o", (colon, colon_sp)), ("a", (arr_open, comma_a, comma_a_sp))):
        aft = after[kind]
        sbody = string(kind, aft)
        lits = {}
        for word in ("true", "false", "null"):
            prev = None
            for i in range(1, len(word)):
                cur_ = st(f"{word[:i]}_{kind}")
                if prev is None:
                    lits[word] = cur_
                else:
                    edge(prev, word[i - 1], cur_)
                prev = cur_
            edge(prev, word[-1], aft)
        minus, zero, int_, dot = st("minus_" + kind), st("zero_" + kind), st("int_" + kind), st("dot_" + kind)
        frac, e_, esign, exp = st("frac_" + kind), st("e_" + kind), st("esign_" + kind), st("exp_" + kind)
        edge(minus, "0", zero)
        edge(minus, "123456789", int_)
        edge(int_, digits, int_)
        for s_ in (zero, int_):
            edge(s_, ".", dot)
        edge(dot, digits, frac)
        edge(frac, digits, frac)
        for s_ in (zero, int_, frac):
            edge(s_, "eE", e_)
        edge(e_, "+-", esign)
        edge(e_, digits, exp)
        edge(esign, digits, exp)
        edge(exp, digits, exp)
        for s_ in (zero, int_, frac, exp):      # a number's terminators act as they do after a value
            for b in range(256):
                if rows[aft][b] != -1:
                    edge(s_, b, rows[aft][b] & 0xFF, rows[aft][b] >> 8)
        for v in value_starts:
            edge(v, "{", obj_open, JSON_ACT_PUSH_OBJECT)
            edge(v, "[", arr_open, JSON_ACT_PUSH_ARRAY)
            edge(v, '"', sbody)
            edge(v, "-", minus)
            edge(v, "0", zero)
            edge(v, "123456789", int_)
            for word in ("true", "false", "null"):
                edge(v, word[0], lits[word])
    assert len(rows) <= GUIDE_JSON_MAX_STATES
    return np.asarray(rows, dtype=np.int16), done


_JSON_TABLE: Optional[Tuple[np.ndarray, int]] = None


def compile_json_guide(token_bytes: Sequence[Optional[bytes]], eos: int, vocab: Optional[int] = None) -> JsonGuide:
    """The JsonGuide of ``guided_json_object`` on a byte table: the fixed table and compile_byte_guide's soundness
    check (ValueError naming a byte on a transition that no single-byte token other than EOS spells)."""
    global _JSON_TABLE
    if _JSON_TABLE is None:
        _JSON_TABLE = build_json_table()
    trans, done = _JSON_TABLE
    vocab = len(token_bytes) if vocab is None else min(vocab, len(token_bytes))
    _, single = _table_facts(token_bytes, eos, vocab)
    for b in np.nonzero((trans >= 0).any(axis=0))[0]:
        if int(b) not in single:
            raise ValueError(f"guided_json_object needs byte 0x{int(b):02X}, which is not supported on this tokenizer: "
                             "no single-byte token spells it")
    return JsonGuide(trans, done, int(eos), ("json_object", int(eos), id_of(token_bytes)))


# ------------------------------------------------------------------ byte tables of HuggingFace tokenizers
def _bytelevel_alphabet() -> Dict[str, int]:
    """The inverse of GPT-2's bytes-to-unicode map: printable Latin-1 stands for itself, the other 68 bytes for
    U+0100 onwards in ascending byte order."""
    keep = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    inv = {chr(b): b for b in keep}
    n = 0
    for b in range(256):
        if b not in keep:
            inv[chr(256 + n)] = b
            n += 1
    return inv


_HF_CHECK_TEXTS = ("Hello, world! 123", " two  spaces\nand a line", "café ☃ {\"k\": [1, 2]}")


def hf_token_bytes(tokenizer, vocab: int) -> Optional[List[Optional[bytes]]]:
    """id -> bytes | None for a HuggingFace tokenizer, ``vocab`` entries (the model's vocabulary; ids beyond the
    tokenizer's are None, and so are special and added tokens). Two layouts are recognised: ByteLevel BPE (every
    piece is spelled in the bytes-to-unicode alphabet) and SentencePiece-style pieces with byte fallback (``<0xXX>``
    is that byte, ``▁`` a space, anything else its UTF-8 bytes). None when neither fits or when a few strings do
    not round-trip (the bytes of ``encode(text)`` must spell ``text``): guided_regex is then refused."""
    try:
        pieces = dict(tokenizer.get_vocab())
        special = set(int(i) for i in getattr(tokenizer, "all_special_ids", ()) or ())
        added = getattr(tokenizer, "get_added_vocab", None)
        special |= set(int(i) for i in (added() if added is not None else {}).values())
    except Exception:
        return None
    if not pieces:
        return None
    plain = [(p, int(i)) for p, i in pieces.items() if int(i) not in special and 0 <= int(i) < vocab]
    alpha = _bytelevel_alphabet()
    table: List[Optional[bytes]] = [None] * vocab
    if all(all(ch in alpha for ch in p) for p, _ in plain):
        for p, i in plain:
            table[i] = bytes(alpha[ch] for ch in p)
    elif any(len(p) == 6 and p.startswith("<0x") and p.endswith(">") for p, _ in plain):
        for p, i in plain:
            if len(p) == 6 and p.startswith("<0x") and p.endswith(">"):
                try:
                    table[i] = bytes([int(p[3:5], 16)])
                    continue
                except ValueError:
                    pass
            table[i] = p.replace("▁", " ").encode("utf-8")
    else:
        return None
    try:
        for text in _HF_CHECK_TEXTS:
            ids = tokenizer.encode(text, add_special_tokens=False)
            got = b"".join(table[i] or b"" for i in ids if 0 <= i < vocab)
            if got != text.encode("utf-8") or any(not 0 <= i < vocab or table[i] is None for i in ids):
                return None
    except Exception:
        return None
    return table


# ------------------------------------------------------------------ the one entry point, cached
_CACHE: "collections.OrderedDict[tuple, Automaton]" = collections.OrderedDict()
_CACHE_MAX = 64
_LOCK = threading.Lock()


def compile_guide(sampling, vocab: int, eos: Optional[int], token_bytes: Optional[Sequence[Optional[bytes]]] = None):
    """The automaton of a request's guide (SamplingParams.guided is true), from a small LRU keyed by the
    canonical spec: an Automaton, a ByteGuide for a guided_regex over a multi-byte vocabulary, a JsonGuide for
    guided_json_object, or a SchemaGuide for guided_json (its key: the schema dumped with sorted keys). ValueError
    for everything the engine must refuse."""
    if sampling.allowed_token_ids is not None:
        spec = ("allowed", tuple(sorted(sampling.allowed_token_ids)), vocab)
    else:
        if eos is None:
            raise ValueError("guided_choice / guided_regex / guided_json_object / guided_json are not supported on "
                             "an engine without an end-of-sequence token")
        if sampling.ignore_eos:
            raise ValueError("guided_choice / guided_regex / guided_json_object / guided_json cannot be combined "
                             "with ignore_eos")
        if getattr(sampling, "guided_json", None) is not None:
            if token_bytes is None:
                raise ValueError("guided_json is not supported on an engine without a byte table of its "
                                 "tokenizer (the byte-level tokenizer, ByteLevel BPE and byte-fallback "
                                 "vocabularies provide one)")
            from src.guided_schema import canonical_schema

            spec = ("json_schema", canonical_schema(sampling.guided_json), vocab, eos, id_of(token_bytes))
        elif getattr(sampling, "guided_json_object", False):
            if token_bytes is None:
                raise ValueError("guided_json_object is not supported on an engine without a byte table of its "
                                 "tokenizer (the byte-level tokenizer, ByteLevel BPE and byte-fallback "
                                 "vocabularies provide one)")
            spec = ("json_object", vocab, eos, id_of(token_bytes))
        elif sampling.guided_choice is not None:
            spec = ("choice", tuple(sorted(set(tuple(c) for c in sampling.guided_choice))), vocab, eos)
        else:
            if token_bytes is None:
                raise ValueError("guided_regex is not supported on an engine without a byte table of its "
                                 "tokenizer (the byte-level tokenizer, ByteLevel BPE and byte-fallback "
                                 "vocabularies provide one)")
            spec = ("regex", sampling.guided_regex, vocab, eos, id_of(token_bytes))
    with _LOCK:
        a = _CACHE.get(spec)
        if a is not None:
            _CACHE.move_to_end(spec)
            return a
    if spec[0] == "allowed":
        a = compile_allowed(spec[1], vocab)
    elif spec[0] == "choice":
        a = compile_choice(spec[1], eos, vocab)
    elif spec[0] == "json_object":
        a = compile_json_guide(token_bytes, eos, vocab)
    elif spec[0] == "json_schema":
        from src.guided_schema import compile_schema_guide

        a = compile_schema_guide(sampling.guided_json, token_bytes, eos, vocab)
    elif _table_facts(token_bytes, eos, min(vocab, len(token_bytes)))[0]:
        # a multi-byte vocabulary: the byte DFA itself, walked per token on the device (ops.byte_guide)
        a = compile_byte_guide(spec[1], token_bytes, eos, vocab)
    else:
        a = compile_regex(spec[1], token_bytes, eos, vocab)
    if isinstance(a, SchemaGuide):
        a = SchemaGuide(a.trans, a.accept, a.eos, spec)
    elif isinstance(a, JsonGuide):
        a = JsonGuide(a.trans, a.done, a.eos, spec)
    elif isinstance(a, ByteGuide):
        a = ByteGuide(a.trans, a.accept, a.eos, spec)
    else:
        a = Automaton(a.row_ptr, a.edge_tok, a.edge_next, spec)
    with _LOCK:
        _CACHE[spec] = a
        while len(_CACHE) > _CACHE_MAX:
            _CACHE.popitem(last=False)
    return a


# ------------------------------------------------------------------ arena bookkeeping (host side)
class FirstFit:
    """A first-fit free list over [0, size): the runner's bookkeeping for the device arenas."""

    def __init__(self, size: int):
        self.size = size
        self.free: List[List[int]] = [[0, size]]  # [offset, length], ascending, coalesced

    def alloc(self, n: int) -> Optional[int]:
        for i, (off, ln) in enumerate(self.free):
            if ln >= n:
                if ln == n:
                    del self.free[i]
                else:
                    self.free[i] = [off + n, ln - n]
                return off
        return None

    def release(self, off: int, n: int) -> None:
        if n <= 0:
            return
        i = 0
        while i < len(self.free) and self.free[i][0] < off:
            i += 1
        self.free.insert(i, [off, n])
        if i + 1 < len(self.free) and off + n == self.free[i + 1][0]:
            self.free[i][1] += self.free[i + 1][1]
            del self.free[i + 1]
        if i > 0 and self.free[i - 1][0] + self.free[i - 1][1] == off:
            self.free[i - 1][1] += self.free[i][1]
            del self.free[i]

    @property
    def used(self) -> int:
        return self.size - sum(ln for _, ln in self.free)


# guided_json: the JSON Schema compiler of the fourth form lives in src/guided_schema.py, which imports this module's
# pieces. Its names are served from here on first use, so either module can be imported first.
_SCHEMA_EXPORTS = ("canonical_schema", "compile_schema_guide", "schema_check_closable", "schema_closable_sets",
                   "schema_depth_sets", "schema_to_pda")


def __getattr__(name: str):
    if name in _SCHEMA_EXPORTS:
        from src import guided_schema

        return getattr(guided_schema, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
