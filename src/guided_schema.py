"""
``guided_json``: a JSON Schema compiled to a ``SchemaGuide`` (src/guided.py), the byte pushdown automaton with a
stack of return states that ``ops.schema_guide`` walks on the device. The output language is a SUBSET of the
documents valid against the schema, in JSON mode's text conventions (compact, or one space after ``,`` and ``:``;
well-formed UTF-8 strings with JSON escapes; JSON numbers).

Construction: one global NFA whose edges are epsilon, byte sets, ``CALL(frame, return node)`` and ``POP(byte)``,
then one subset construction over it. Everything that is not recursive is inlined and costs states, not stack. A
frame is what needs the stack: the target of a ``$ref`` met again while it is being expanded, and the two built-in
frames any-object and any-array of free-form values. A frame is entered by a push on its opening ``{`` / ``[`` (the
return state is the closure of the callers' "after this value" nodes) and left by a pop on its closing ``}`` / ``]``,
so a call is always bracketed and a number that ends inside a frame needs no lookahead. A frame's subsets are shared
by all its callers.

No dead ends, proved per compiled table (``schema_check_closable``): with R[d] the states reachable at depth d
(a push at depth d also marks its return state reachable at depth d), every state of R[d], d >= 1, must reach a pop,
and every state of R[0] an accepting state, over transitions that do not push and over pushes (below the depth cap)
whose frame state itself reaches a pop one level up, the walk going on from the return state. At the cap this is
"a pop is reachable over non-push transitions only". By induction on the depth every reachable configuration then has
a legal byte and a finite way to the end; the single-byte-token check of ``compile_schema_guide`` carries that over
to tokens, and a single-byte token pushes at most once, within the per-token push cap.

Pure numpy / Python, as src/guided.py.
"""

from __future__ import annotations

import collections
import json
import threading
from typing import Any, Dict, FrozenSet, List, Optional, Sequence, Tuple

import numpy as np

from src.guided import (_SCHEMA_BOUND_MAX, _SCHEMA_STATE_BITS, GUIDE_MAX_STATES, GUIDE_SCHEMA_MAX_DEPTH,
                        SCHEMA_ACT_POP, SCHEMA_ACT_PUSH, SchemaGuide, _reach, _table_facts, id_of, regex_to_dfa)

_ANNOTATIONS = frozenset(["title", "description", "default", "examples", "$schema", "$id", "$comment", "format",
                          "deprecated", "readOnly", "writeOnly", "$defs", "definitions"])
_BY_TYPE = {"object": ("properties", "required", "additionalProperties"),
            "array": ("items", "minItems", "maxItems"),
            "string": ("minLength", "maxLength", "pattern")}
_TYPES = ("object", "array", "string", "number", "integer", "boolean", "null")
_KNOWN = frozenset(["type", "enum", "const", "anyOf", "allOf", "$ref"] + [k for ks in _BY_TYPE.values() for k in ks])

_DIGITS = frozenset(b"0123456789")
_DIGITS19 = frozenset(b"123456789")
_HEX = frozenset(b"0123456789abcdefABCDEF")
_STR_PLAIN = frozenset(b for b in range(0x20, 0x80) if b not in (0x22, 0x5C))   # build_json_table's string body
_ESC_SIMPLE = frozenset(b'"\\/bfnrt')
_CONT = frozenset(range(0x80, 0xC0))
_NODE_LIMIT = 4 * GUIDE_MAX_STATES


def _err(what: str, ptr: str):
    raise ValueError(f"guided_json: {what} at {ptr or '#'}")


class _Builder:
    """The global NFA. Node fields: eps targets, (byte set, target) edges, (frame, return node) calls, pop bytes."""

    def __init__(self, root: Any):
        self.root = root
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[FrozenSet[int], int]]] = []
        self.calls: List[List[Tuple[int, int]]] = []
        self.pops: List[set] = []
        self.frame_entry: List[int] = []          # frame id -> entry node (its opening bytes leave from here)
        self.frame_of: Dict[str, int] = {}        # "$any_object", "$any_array" or a recursive $ref's pointer
        self.recursive: set = set()
        self.pending: List[Tuple[int, str]] = []  # frames whose body is still to be built

    # ---- nodes and edges
    def node(self) -> int:
        # a cheap bound before the subset construction, which would need seconds to find the state cap itself: the
        # construction yields about two NFA nodes per state (1.4 for bounded strings, fewer for literals)
        if len(self.eps) >= _NODE_LIMIT:
            raise ValueError(f"guided_json: the guide's automaton has more than {GUIDE_MAX_STATES} states (its "
                             f"construction passed {_NODE_LIMIT} nodes)")
        self.eps.append([])
        self.edges.append([])
        self.calls.append([])
        self.pops.append(set())
        return len(self.eps) - 1

    def edge(self, a: int, bs, b: int) -> None:
        self.edges[a].append((bs if isinstance(bs, frozenset) else frozenset(bs), b))

    def lit(self, a: int, data: bytes, end: int) -> None:
        """a --data--> end"""
        for i, x in enumerate(data):
            b = end if i == len(data) - 1 else self.node()
            self.edge(a, [x], b)
            a = b
        if not data:
            self.eps[a].append(end)

    def sep(self, a: int, byte: int) -> int:
        """a --byte--> x, with one optional space behind it: JSON mode's ',' and ':'."""
        x, y = self.node(), self.node()
        self.edge(a, [byte], x)
        self.edge(x, [0x20], y)
        self.eps[x].append(y)
        return y

    def close(self, a: int, byte: int, closer) -> None:
        """The container's closing byte from a: an ordinary edge to closer (a node), or a pop (closer None)."""
        if closer is None:
            self.pops[a].add(byte)
        else:
            self.edge(a, [byte], closer)

    # ---- scalars
    def char(self, a: int, b: int, allow_u: bool) -> None:
        """One string character from a to b: build_json_table's classes (unescaped, escapes, well-formed UTF-8)."""
        esc = self.node()
        self.edge(a, _STR_PLAIN, b)
        self.edge(a, [0x5C], esc)
        self.edge(esc, _ESC_SIMPLE, b)
        if allow_u:
            u = [self.node() for _ in range(4)]
            self.edge(esc, [0x75], u[0])
            for i in range(4):
                self.edge(u[i], _HEX, u[i + 1] if i < 3 else b)
        c1, c2, c3 = self.node(), self.node(), self.node()
        e0, ed, f0, f4 = self.node(), self.node(), self.node(), self.node()
        self.edge(a, range(0xC2, 0xE0), c1)
        self.edge(a, [0xE0], e0)
        self.edge(a, [x for x in range(0xE1, 0xF0) if x != 0xED], c2)
        self.edge(a, [0xED], ed)
        self.edge(a, [0xF0], f0)
        self.edge(a, range(0xF1, 0xF4), c3)
        self.edge(a, [0xF4], f4)
        self.edge(c1, _CONT, b)
        self.edge(c2, _CONT, c1)
        self.edge(c3, _CONT, c2)
        self.edge(e0, range(0xA0, 0xC0), c1)
        self.edge(ed, range(0x80, 0xA0), c1)
        self.edge(f0, range(0x90, 0xC0), c2)
        self.edge(f4, range(0x80, 0x90), c2)

    def string(self, end: int, lo: int = 0, hi: Optional[int] = None, bounded: bool = False) -> int:
        entry = self.node()
        n = [self.node() for _ in range((hi if hi is not None else lo) + 1)]
        self.edge(entry, [0x22], n[0])
        for k in range(len(n)):
            if k >= lo:
                self.edge(n[k], [0x22], end)
            if k + 1 < len(n):
                self.char(n[k], n[k + 1], not bounded)
            elif hi is None:
                self.char(n[k], n[k], not bounded)
        return entry

    def pattern(self, pat: str, end: int, ptr: str) -> int:
        if not isinstance(pat, str) or len(pat) < 2 or not pat.startswith("^") or not pat.endswith("$") or \
                pat.endswith("\\$"):
            _err("keyword 'pattern' is supported only in the form ^...$", ptr)
        try:
            trans, accept = regex_to_dfa(pat[1:-1])
        except ValueError as e:
            _err(f"keyword 'pattern': {e}", ptr)
        trans = trans.copy()
        trans[:, [b for b in range(256) if b < 0x20 or b in (0x22, 0x5C)]] = -1   # the string never needs an escape
        frm, byte = np.nonzero(trans >= 0)
        n = trans.shape[0]
        live = _reach(n, trans[frm, byte], frm, np.nonzero(accept)[0]) if len(frm) or accept.any() else \
            np.zeros(n, dtype=bool)
        if not live[0]:
            _err("keyword 'pattern' matches no string that needs no escape", ptr)
        trans = np.where((trans >= 0) & live[np.maximum(trans, 0)], trans, -1)
        frm, byte = np.nonzero(trans >= 0)
        reach = _reach(n, frm, trans[frm, byte], np.asarray([0])) & live
        entry = self.node()
        nodes = {int(s): self.node() for s in np.nonzero(reach)[0]}
        self.edge(entry, [0x22], nodes[0])
        for s, a in nodes.items():
            by_t: Dict[int, List[int]] = {}
            for b in np.nonzero(trans[s] >= 0)[0]:
                by_t.setdefault(int(trans[s, b]), []).append(int(b))
            for t, bs in by_t.items():
                self.edge(a, bs, nodes[t])
            if accept[s]:
                self.edge(a, [0x22], end)
        return entry

    def number(self, end: int, integer: bool) -> int:
        entry, minus, zero, int_ = self.node(), self.node(), self.node(), self.node()
        self.edge(entry, b"-", minus)
        for a in (entry, minus):
            self.edge(a, b"0", zero)
            self.edge(a, _DIGITS19, int_)
        self.edge(int_, _DIGITS, int_)
        ends = [zero, int_]
        if not integer:
            dot, frac, e_, esign, exp = (self.node() for _ in range(5))
            for a in (zero, int_):
                self.edge(a, b".", dot)
            self.edge(dot, _DIGITS, frac)
            self.edge(frac, _DIGITS, frac)
            for a in (zero, int_, frac):
                self.edge(a, b"eE", e_)
            self.edge(e_, b"+-", esign)
            for a in (e_, esign, exp):
                self.edge(a, _DIGITS, exp)
            ends += [frac, exp]
        for a in ends:
            self.eps[a].append(end)
        return entry

    def words(self, words: Sequence[bytes], end: int) -> int:
        entry = self.node()
        for w in words:
            self.lit(entry, w, end)
        return entry

    # ---- frames
    def frame(self, name: str) -> int:
        f = self.frame_of.get(name)
        if f is None:
            f = self.frame_of[name] = len(self.frame_entry)
            self.frame_entry.append(self.node())
            self.pending.append((f, name))
        return f

    def call(self, name: str, end: int) -> int:
        entry = self.node()
        self.calls[entry].append((self.frame(name), end))
        return entry

    def build_pending(self) -> None:
        while self.pending:
            f, name = self.pending.pop()
            entry = self.frame_entry[f]
            if name == "$any_object":
                self.eps[entry].append(self.any_object(None))
            elif name == "$any_array":
                self.eps[entry].append(self.array({}, "", None))
            else:
                for a in self.frame_alternatives(self.resolve(name, name), name, set()):
                    self.eps[entry].append(a)

    def frame_alternatives(self, s: Any, ptr: str, seen: set) -> List[int]:
        """The entry nodes of a recursive target's alternatives, each an object or an array closed by a pop."""
        refuse = "a recursive $ref's target must be an object or an array in every alternative, which the schema"
        if not isinstance(s, dict):
            _err(refuse, ptr)
        kw = self.keywords(s, ptr)
        if "$ref" in kw:
            p = self.pointer(kw, ptr)
            if p in seen:
                _err("a $ref that only refers to itself", ptr)
            return self.frame_alternatives(self.resolve(p, ptr), p, seen | {p})
        if "anyOf" in kw or "allOf" in kw:
            out: List[int] = []
            for i, sub in enumerate(self.combinator(kw, ptr)):
                out += self.frame_alternatives(sub, f"{ptr}/{'anyOf' if 'anyOf' in kw else 'allOf'}/{i}", seen)
            return out
        if "enum" in kw or "const" in kw:
            _err(refuse, ptr)
        types = self.types(kw, ptr)
        if not types or any(t not in ("object", "array") for t in types):
            _err(refuse, ptr)
        return [self.object(kw, ptr, None) if t == "object" else self.array(kw, ptr, None) for t in types]

    # ---- schema plumbing
    def resolve(self, p: str, ptr: str) -> Any:
        if p == "#":
            return self.root
        for pre in ("#/$defs/", "#/definitions/"):
            if p.startswith(pre):
                name = p[len(pre):].replace("~1", "/").replace("~0", "~")
                defs = self.root.get(pre[2:-1]) if isinstance(self.root, dict) else None
                if not isinstance(defs, dict) or name not in defs:
                    _err(f"$ref {p!r} names no definition", ptr)
                return defs[name]
        _err(f"$ref {p!r} is not supported (only '#', '#/$defs/NAME' and '#/definitions/NAME')", ptr)

    def pointer(self, kw: Dict[str, Any], ptr: str) -> str:
        p = kw["$ref"]
        if not isinstance(p, str):
            _err("$ref must be a string", ptr)
        if len(kw) > 1:
            other = sorted(k for k in kw if k != "$ref")[0]
            _err(f"keyword {other!r} next to $ref is not supported", ptr)
        return p

    def keywords(self, s: Dict[str, Any], ptr: str) -> Dict[str, Any]:
        """The schema's keywords without the annotations; anything unknown is refused by name."""
        for k in s:
            if k not in _KNOWN and k not in _ANNOTATIONS:
                _err(f"keyword {k!r} is not supported", f"{ptr}/{k}")
        return {k: v for k, v in s.items() if k in _KNOWN}

    def combinator(self, kw: Dict[str, Any], ptr: str) -> List[Any]:
        name = "anyOf" if "anyOf" in kw else "allOf"
        subs = kw[name]
        if len(kw) > 1:
            other = sorted(k for k in kw if k != name)[0]
            _err(f"keyword {other!r} next to {name} is not supported", ptr)
        if not isinstance(subs, list) or not subs:
            _err(f"{name} must be a non-empty list", f"{ptr}/{name}")
        if name == "allOf" and len(subs) != 1:
            _err("keyword 'allOf' is supported with exactly one element", f"{ptr}/allOf")
        return subs

    def types(self, kw: Dict[str, Any], ptr: str) -> List[str]:
        """The alternatives ``type`` names (without it: the types the other keywords imply; none: any value)."""
        t = kw.get("type")
        if t is None:
            types = [n for n, ks in _BY_TYPE.items() if any(k in kw for k in ks)]
        else:
            types = [t] if isinstance(t, str) else t
            if not isinstance(types, list) or not types or any(x not in _TYPES for x in types) or \
                    len(set(types)) != len(types):
                _err(f"type must be one of {', '.join(_TYPES)} or a list of them", f"{ptr}/type")
        for name, ks in _BY_TYPE.items():
            for k in ks:
                if k in kw and name not in types:
                    _err(f"keyword {k!r} applies to type {name!r} only, which the schema does not name", f"{ptr}/{k}")
        return list(types)

    def discover(self) -> None:
        """The pointers of recursive $refs: those met again while they are being expanded."""
        visited: set = set()

        def walk(s: Any, stack: Tuple[str, ...], ptr: str) -> None:
            if not isinstance(s, dict):
                return
            if isinstance(s.get("$ref"), str):
                p = s["$ref"]
                if p in stack:
                    self.recursive.add(p)
                elif p not in visited:
                    visited.add(p)
                    walk(self.resolve(p, ptr), stack + (p,), p)
                return
            props = s.get("properties")
            for k, v in (props.items() if isinstance(props, dict) else ()):
                walk(v, stack, f"{ptr}/properties/{k}")
            walk(s.get("items"), stack, f"{ptr}/items")
            walk(s.get("additionalProperties"), stack, f"{ptr}/additionalProperties")
            for name in ("anyOf", "allOf"):
                for i, v in enumerate(s[name] if isinstance(s.get(name), list) else ()):
                    walk(v, stack, f"{ptr}/{name}/{i}")

        walk(self.root, ("#",), "#")

    # ---- values
    def any_value(self, end: int) -> int:
        entry = self.node()
        self.eps[entry] += [self.string(end), self.number(end, False), self.words([b"true", b"false", b"null"], end),
                            self.call("$any_object", end), self.call("$any_array", end)]
        return entry

    def any_object(self, closer) -> int:
        """``{``, then members "key": value with any key and any value, then ``}`` by closer."""
        entry, opened, key, after = self.node(), self.node(), self.node(), self.node()
        self.edge(entry, b"{", opened)
        self.close(opened, 0x7D, closer)
        self.eps[opened].append(key)
        key_end = self.node()
        self.eps[key].append(self.string(key_end))
        self.eps[self.sep(key_end, 0x3A)].append(self.any_value(after))
        self.close(after, 0x7D, closer)
        self.eps[self.sep(after, 0x2C)].append(key)
        return entry

    def value(self, s: Any, ptr: str, end: int) -> int:
        """The entry node of the NFA of one value of schema s that ends in node ``end``."""
        if s is True:
            return self.any_value(end)
        if s is False:
            _err("the schema 'false' is not supported", ptr)
        if not isinstance(s, dict):
            _err("a schema must be an object or true", ptr)
        kw = self.keywords(s, ptr)
        if not kw:
            return self.any_value(end)
        if "$ref" in kw:
            p = self.pointer(kw, ptr)
            target = self.resolve(p, ptr)
            return self.call(p, end) if p in self.recursive else self.value(target, p, end)
        if "anyOf" in kw or "allOf" in kw:
            name = "anyOf" if "anyOf" in kw else "allOf"
            entry = self.node()
            for i, sub in enumerate(self.combinator(kw, ptr)):
                self.eps[entry].append(self.value(sub, f"{ptr}/{name}/{i}", end))
            return entry
        if "enum" in kw or "const" in kw:
            return self.enum(kw, ptr, end)
        entry = self.node()
        for t in self.types(kw, ptr):
            if t == "object":
                a = self.object(kw, ptr, end)
            elif t == "array":
                a = self.array(kw, ptr, end)
            elif t == "string":
                a = self.typed_string(kw, ptr, end)
            elif t in ("number", "integer"):
                a = self.number(end, t == "integer")
            else:
                a = self.words([b"true", b"false"] if t == "boolean" else [b"null"], end)
            self.eps[entry].append(a)
        return entry

    def enum(self, kw: Dict[str, Any], ptr: str, end: int) -> int:
        name = "enum" if "enum" in kw else "const"
        for k in kw:
            if k not in ("enum", "const", "type"):
                _err(f"keyword {k!r} next to {name} is not supported", ptr)
        if "enum" in kw and "const" in kw:
            _err("keyword 'const' next to enum is not supported", ptr)
        vals = kw["enum"] if name == "enum" else [kw["const"]]
        if not isinstance(vals, list) or not vals:
            _err("enum must be a non-empty list", f"{ptr}/enum")
        if "type" in kw:
            types = self.types({"type": kw["type"]}, ptr)

            def is_a(v, t):
                if t == "integer":
                    return isinstance(v, int) and not isinstance(v, bool) or isinstance(v, float) and v.is_integer()
                return {"object": isinstance(v, dict), "array": isinstance(v, list), "string": isinstance(v, str),
                        "number": isinstance(v, (int, float)) and not isinstance(v, bool),
                        "boolean": isinstance(v, bool), "null": v is None}[t]

            vals = [v for v in vals if any(is_a(v, t) for t in types)]
            if not vals:
                _err(f"no value of {name} has the schema's type", ptr)
        try:
            texts = [json.dumps(v, separators=(",", ":"), ensure_ascii=False, allow_nan=False).encode("utf-8")
                     for v in vals]
        except (TypeError, ValueError):
            _err(f"{name} holds a value that is not JSON", ptr)
        return self.words(sorted(set(texts)), end)

    def bound(self, kw: Dict[str, Any], name: str, ptr: str) -> Optional[int]:
        v = kw.get(name)
        if v is None:
            return None
        if isinstance(v, float) and v.is_integer():
            v = int(v)
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= _SCHEMA_BOUND_MAX:
            _err(f"{name} must be an integer in [0, {_SCHEMA_BOUND_MAX}]", f"{ptr}/{name}")
        return v

    def typed_string(self, kw: Dict[str, Any], ptr: str, end: int) -> int:
        lo, hi = self.bound(kw, "minLength", ptr), self.bound(kw, "maxLength", ptr)
        if "pattern" in kw:
            if lo is not None or hi is not None:
                _err("keyword 'pattern' together with minLength / maxLength is not supported", ptr)
            return self.pattern(kw["pattern"], end, f"{ptr}/pattern")
        if lo is not None and hi is not None and lo > hi:
            _err("minLength above maxLength", ptr)
        # under a length bound \u escapes are not offered: a surrogate pair can then never make the count wrong
        return self.string(end, lo or 0, hi, bounded=lo is not None or hi is not None)

    def object(self, kw: Dict[str, Any], ptr: str, closer) -> int:
        props, req, addl = kw.get("properties"), kw.get("required", []), kw.get("additionalProperties")
        if props is not None and not isinstance(props, dict):
            _err("properties must be an object", f"{ptr}/properties")
        if not isinstance(req, list) or any(not isinstance(r, str) for r in req):
            _err("required must be a list of names", f"{ptr}/required")
        if addl is not None and not isinstance(addl, (bool, dict)):
            _err("additionalProperties must be a schema", f"{ptr}/additionalProperties")
        for r in req:
            if r not in (props or {}):
                _err(f"required names {r!r}, which properties does not declare: the object is closed", f"{ptr}/required")
        if not props:
            if isinstance(addl, dict) and addl:
                _err("keyword 'additionalProperties' with a schema is not supported", f"{ptr}/additionalProperties")
            if addl is False:   # nothing may be in it
                entry, opened = self.node(), self.node()
                self.edge(entry, b"{", opened)
                self.close(opened, 0x7D, closer)
                return entry
            # any JSON object: the built-in frame (a frame's own alternative: its body, closed by the frame's pop)
            return self.any_object(None) if closer is None else self.call("$any_object", closer)
        if addl is not None and addl is not False:
            _err("keyword 'additionalProperties' other than false next to properties is not supported: the object "
                 "is closed", f"{ptr}/additionalProperties")
        # members in declaration order. first[i] / nxt[i]: about to decide member i with nothing / something emitted
        names = list(props)
        entry = self.node()
        first = [self.node() for _ in range(len(names) + 1)]
        nxt = [self.node() for _ in range(len(names) + 1)]
        self.edge(entry, b"{", first[0])
        for i, name in enumerate(names):
            member = self.node()   # the one copy of "name": value
            self.eps[first[i]].append(member)
            self.eps[self.sep(nxt[i], 0x2C)].append(member)
            key_end = self.node()
            self.lit(member, json.dumps(name, ensure_ascii=False).encode("utf-8"), key_end)
            self.eps[self.sep(key_end, 0x3A)].append(self.value(props[name], f"{ptr}/properties/{name}", nxt[i + 1]))
            if name not in req:
                self.eps[first[i]].append(first[i + 1])
                self.eps[nxt[i]].append(nxt[i + 1])
        self.close(first[-1], 0x7D, closer)
        self.close(nxt[-1], 0x7D, closer)
        return entry

    def array(self, kw: Dict[str, Any], ptr: str, closer) -> int:
        lo, hi = self.bound(kw, "minItems", ptr) or 0, self.bound(kw, "maxItems", ptr)
        if hi is not None and lo > hi:
            _err("minItems above maxItems", ptr)
        items = kw.get("items", True)
        top = hi if hi is not None else max(lo, 1)   # after[k]: k items read (k = top, unbounded: top or more)
        entry = self.node()
        after = [self.node() for _ in range(top + 1)]
        self.edge(entry, b"[", after[0])
        item_to: Dict[int, int] = {}                 # one copy of the item per count it leads to
        for k in range(top + 1):
            if k >= lo:
                self.close(after[k], 0x5D, closer)
            to = k + 1 if k < top else (top if hi is None else None)
            if to is None:
                continue
            if to not in item_to:
                item_to[to] = self.value(items, f"{ptr}/items", after[to])
            self.eps[after[k] if k == 0 else self.sep(after[k], 0x2C)].append(item_to[to])
        return entry


def _subsets(b: _Builder, start: int, final: int) -> Tuple[np.ndarray, np.ndarray]:
    def closure(nodes) -> FrozenSet[int]:
        seen = set(nodes)
        stack = list(nodes)
        while stack:
            for t in b.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)

    # a frame's opening bytes: byte -> the frame's subset after it
    opens: List[Dict[int, FrozenSet[int]]] = []
    for entry in b.frame_entry:
        by: Dict[int, set] = {}
        for n in closure([entry]):
            if b.calls[n] or b.pops[n]:
                raise ValueError("guided_json: a recursive $ref's target must open with '{' or '['")
            for bs, t in b.edges[n]:
                for x in bs:
                    by.setdefault(x, set()).add(t)
        if set(by) - {0x7B, 0x5B}:
            raise ValueError("guided_json: a recursive $ref's target must open with '{' or '['")
        opens.append({x: closure(ts) for x, ts in by.items()})

    index: Dict[FrozenSet[int], int] = {}
    order: List[FrozenSet[int]] = []

    def state_of(cl: FrozenSet[int]) -> int:
        j = index.get(cl)
        if j is None:
            j = index[cl] = len(order)
            order.append(cl)
            if len(order) > GUIDE_MAX_STATES:
                raise ValueError(f"guided_json: the guide's automaton has more than {GUIDE_MAX_STATES} states")
        return j

    state_of(closure([start]))
    rows: List[List[int]] = []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        by_byte: Dict[int, set] = {}
        pops: set = set()
        calls: Dict[int, set] = {}
        for n in cur:
            for bs, t in b.edges[n]:
                for x in bs:
                    by_byte.setdefault(x, set()).add(t)
            pops |= b.pops[n]
            for f, ret in b.calls[n]:
                calls.setdefault(f, set()).add(ret)
        row = [-1] * 256
        memo: Dict[FrozenSet[int], int] = {}
        for x, targets in by_byte.items():
            tk = frozenset(targets)
            j = memo.get(tk)
            if j is None:
                j = memo[tk] = state_of(closure(tk))
            row[x] = j
        for f, rets in calls.items():
            ret = None
            for x, inner in opens[f].items():
                if row[x] != -1:
                    raise ValueError(f"guided_json: byte {chr(x)!r} could open two different recursive or free-form "
                                     "values, or such a value and an inlined one, at the same place (alternatives "
                                     "that start alike are not supported)")
                if ret is None:
                    ret = state_of(closure(rets))
                row[x] = state_of(inner) | (ret << _SCHEMA_STATE_BITS) | (SCHEMA_ACT_PUSH << 28)
        for x in pops:
            if row[x] != -1:
                raise ValueError(f"guided_json: byte {chr(x)!r} could close a recursive or free-form value and also "
                                 "go on, at the same place")
            row[x] = SCHEMA_ACT_POP << 28
        rows.append(row)
    trans = np.asarray(rows, dtype=np.int32).reshape(len(order), 256)
    accept = np.fromiter((final in s for s in order), dtype=np.uint8, count=len(order))
    return trans, accept


def _pda_edges(trans: np.ndarray):
    """(plain src, plain dst, push src, push next, push return, states with a pop), each pair once."""
    n = trans.shape[0]
    mask = (1 << _SCHEMA_STATE_BITS) - 1
    act = np.where(trans >= 0, trans >> 28, -1)
    src = np.nonzero(act == 0)[0].astype(np.int64)
    pair = np.unique(src * n + (trans[act == 0] & mask))
    psrc = np.nonzero(act == SCHEMA_ACT_PUSH)[0].astype(np.int64)
    pv = trans[act == SCHEMA_ACT_PUSH].astype(np.int64)
    trip = np.unique((psrc << (2 * _SCHEMA_STATE_BITS)) | (pv & ((1 << (2 * _SCHEMA_STATE_BITS)) - 1)))
    return (pair // n, pair % n, trip >> (2 * _SCHEMA_STATE_BITS), trip & mask, (trip >> _SCHEMA_STATE_BITS) & mask,
            np.nonzero((act == SCHEMA_ACT_POP).any(axis=1))[0])


def schema_depth_sets(trans: np.ndarray) -> List[np.ndarray]:
    """R[d], d = 0..GUIDE_SCHEMA_MAX_DEPTH: bool [S], the states a walk can be in at depth d (a superset: a push
    at depth d marks its return state at depth d whether or not the frame can be left)."""
    n = trans.shape[0]
    plain_src, plain_dst, pfrm, push_nxt, push_ret, _ = _pda_edges(trans)
    src, dst = np.concatenate([plain_src, pfrm]), np.concatenate([plain_dst, push_ret])
    out: List[np.ndarray] = []
    seeds = np.asarray([0], dtype=np.int64)
    for d in range(GUIDE_SCHEMA_MAX_DEPTH + 1):
        if not len(seeds):
            r = np.zeros(n, dtype=bool)
        elif out and d < GUIDE_SCHEMA_MAX_DEPTH and np.array_equal(seeds, prev_seeds):
            r = out[-1]
        elif d < GUIDE_SCHEMA_MAX_DEPTH:
            r = _reach(n, src, dst, seeds)
        else:   # at the cap a push is no transition
            r = _reach(n, plain_src, plain_dst, seeds)
        out.append(r)
        prev_seeds = seeds
        seeds = np.unique(push_nxt[r[pfrm]])
    return out


def schema_closable_sets(trans: np.ndarray, accept: np.ndarray) -> List[np.ndarray]:
    """C[d]: bool [S]. d >= 1: the states that reach a pop at depth d; C[0]: those that reach an accepting state
    at depth 0 — over plain transitions, and over a push (below the cap) whose frame state is in C[d + 1], the
    walk going on from the return state."""
    n = trans.shape[0]
    plain_src, plain_dst, pfrm, push_nxt, push_ret, poppers = _pda_edges(trans)
    out: List[Optional[np.ndarray]] = [None] * (GUIDE_SCHEMA_MAX_DEPTH + 1)
    above = np.zeros(n, dtype=bool)   # C[d + 1]; nothing at the cap
    prev_ok = None
    for d in range(GUIDE_SCHEMA_MAX_DEPTH, -1, -1):
        ok = above[push_nxt] if d < GUIDE_SCHEMA_MAX_DEPTH else np.zeros(len(pfrm), dtype=bool)
        seeds = poppers if d >= 1 else np.nonzero(accept)[0]
        if d >= 1 and prev_ok is not None and np.array_equal(ok, prev_ok):
            out[d] = above   # the same edges and seeds as one level up
            continue
        prev_ok = ok
        src, dst = np.concatenate([plain_src, pfrm[ok]]), np.concatenate([plain_dst, push_ret[ok]])
        # backwards: the nodes from which a seed is reachable
        out[d] = _reach(n, dst, src, seeds) if len(seeds) else np.zeros(n, dtype=bool)
        above = out[d]
    return out


def schema_check_closable(trans: np.ndarray, accept: np.ndarray) -> None:
    """The module docstring's no-dead-end proof for one table; a ValueError names the first failing depth."""
    reach, can = schema_depth_sets(trans), schema_closable_sets(trans, accept)
    if (reach[0] & ((trans >= 0) & (trans >> 28 == SCHEMA_ACT_POP)).any(axis=1)).any():
        raise AssertionError("a schema guide that pops at depth 0")
    for d in range(GUIDE_SCHEMA_MAX_DEPTH + 1):
        stuck = reach[d] & ~can[d]
        if stuck.any():
            raise ValueError(f"guided_json: the schema has a dead end: at nesting depth {d} of its recursive or "
                             "free-form values a place is reached from which the document cannot be completed (a "
                             "required member that refers to its own object, or a required recursive or free-form "
                             f"value that the depth cap of {GUIDE_SCHEMA_MAX_DEPTH} bars)")


_PDA_CACHE: "collections.OrderedDict[str, Any]" = collections.OrderedDict()   # (trans, accept), or a refusal's text
_PDA_CACHE_MAX = 64
_PDA_LOCK = threading.Lock()


def canonical_schema(schema: Any) -> str:
    """The cache key of a schema: a dict or its JSON text, dumped with sorted keys. A ValueError for anything else."""
    if isinstance(schema, str):
        try:
            schema = json.loads(schema)
        except ValueError:
            raise ValueError("guided_json must be a JSON Schema: an object, or its JSON text") from None
    if not isinstance(schema, dict):
        raise ValueError("guided_json must be a JSON Schema: an object, or its JSON text")
    try:
        return json.dumps(schema, sort_keys=True, allow_nan=False)
    except (TypeError, ValueError):
        raise ValueError("guided_json must be a JSON Schema: an object, or its JSON text") from None


def schema_to_pda(schema: Any) -> Tuple[np.ndarray, np.ndarray]:
    """(trans int32 [S, 256], accept uint8 [S]) of a schema, table-free: everything ``compile_schema_guide``
    refuses except a byte without a single-byte token. Kept in a small LRU by the canonical text, so the same
    schema with its keys reordered is one entry: its members keep the order of whichever spelling came first, and a
    document in that order is valid against either."""
    key = canonical_schema(schema)
    root = json.loads(schema) if isinstance(schema, str) else schema
    with _PDA_LOCK:
        hit = _PDA_CACHE.get(key)
        if hit is not None:
            _PDA_CACHE.move_to_end(key)
    if isinstance(hit, str):   # a refusal is kept too: the state cap is only found after seconds of construction
        raise ValueError(hit)
    if hit is not None:
        return hit
    try:
        b = _Builder(root)
        b.discover()
        final = b.node()
        start = b.call("#", final) if "#" in b.recursive else b.value(root, "#", final)
        b.build_pending()
        trans, accept = _subsets(b, start, final)
        schema_check_closable(trans, accept)
        made: Any = (trans, accept)
    except ValueError as e:
        made = str(e)
    with _PDA_LOCK:
        _PDA_CACHE[key] = made
        while len(_PDA_CACHE) > _PDA_CACHE_MAX:
            _PDA_CACHE.popitem(last=False)
    if isinstance(made, str):
        raise ValueError(made)
    return made


def compile_schema_guide(schema: Any, token_bytes: Sequence[Optional[bytes]], eos: int,
                         vocab: Optional[int] = None) -> SchemaGuide:
    """The SchemaGuide of ``guided_json`` on a byte table: ``schema_to_pda`` and compile_byte_guide's soundness
    check (a ValueError names a byte on a transition that no single-byte token other than EOS spells)."""
    trans, accept = schema_to_pda(schema)
    vocab = len(token_bytes) if vocab is None else min(vocab, len(token_bytes))
    _, single = _table_facts(token_bytes, eos, vocab)
    for x in np.nonzero((trans >= 0).any(axis=0))[0]:
        if int(x) not in single:
            raise ValueError(f"guided_json needs byte 0x{int(x):02X}, which is not supported on this tokenizer: no "
                             "single-byte token spells it")
    return SchemaGuide(trans, accept, int(eos), ("json_schema", canonical_schema(schema), int(eos), id_of(token_bytes)))
