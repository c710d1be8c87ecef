"""An independent oracle for structured outputs (guided_json): a straightforward simulator of a SchemaGuide's
configuration rules, a small validator for the supported JSON Schema subset, and ``build_case``, the shared kernel
case. Not a test module.

The simulator shares no code with src/guided.py, src/ops/reference.py or the kernel: a configuration is (state,
list of return states); tokens are walked through a TRIE of the vocabulary's bytes depth first, so a dead prefix bars
every token below it (the reference walks level by level over arrays, the kernel one chain per lane).

Rules (csrc/kernels/schema_guide.hip is the written contract):
  * an entry is -1 or next | ret << 14 | act << 28, act 0 none, 1 push, 2 pop; anything else READ is a table error,
    and so are a next or return state at or above n_states and a pop with an empty stack;
  * a push at depth 32, or a token's fifth own push that is still on the stack, is no transition;
  * EOS is allowed iff the state accepts and the stack is empty; in the sink (state n_states) only EOS is.
"""

import functools
import json
import random

import numpy as np

DEPTH_CAP, PUSH_CAP, MAX_TOKEN_BYTES = 32, 4, 32
ERR_NO_EDGE, ERR_TABLE = 1, 2
DEAD, BAD = "dead", "bad"


# ------------------------------------------------------------------ the simulator
def byte_step(trans, ns, state, stack, held, byte):
    """One byte: DEAD, BAD or (state, stack, held). ``stack`` is not modified."""
    v = int(trans[state][byte])
    if v == -1:
        return DEAD
    if v < 0 or v >> 30:
        return BAD
    nxt, ret, act = v & 0x3FFF, (v >> 14) & 0x3FFF, v >> 28
    if act == 3 or nxt >= ns or ret >= ns:
        return BAD
    if act == 1:
        if len(stack) >= DEPTH_CAP or held >= PUSH_CAP:
            return DEAD
        return nxt, stack + [ret], held + 1
    if act == 2:
        if not stack:
            return BAD
        return stack[-1], stack[:-1], max(held - 1, 0)
    return nxt, stack, held


def feed(trans, ns, state, stack, data):
    """A token's bytes: DEAD, BAD or (state, stack)."""
    held = 0
    for b in data:
        r = byte_step(trans, ns, state, stack, held, b)
        if r in (DEAD, BAD):
            return r
        state, stack, held = r
    return state, stack


def text_config(trans, ns, text):
    """The configuration after ``text`` fed byte by byte (each byte a token of its own) from the start."""
    state, stack = 0, []
    for b in text.encode("utf-8") if isinstance(text, str) else text:
        r = feed(trans, ns, state, stack, bytes([b]))
        assert r not in (DEAD, BAD), (text, b)
        state, stack = r
    return state, stack


def accepts(trans, accept, text):
    state, stack = 0, []
    for b in text.encode("utf-8") if isinstance(text, str) else text:
        r = feed(trans, len(trans), state, stack, bytes([b]))
        if r in (DEAD, BAD):
            return False
        state, stack = r
    return bool(accept[state]) and not stack


def make_trie(tokens, lim):
    """{byte: node} with node[-1] = the ids ending there; only tokens of 1..32 bytes below lim are walked at all."""
    root = {}
    for t in range(min(lim, len(tokens))):
        bs = tokens[t]
        if not bs or len(bs) > MAX_TOKEN_BYTES:
            continue
        node = root
        for b in bs:
            node = node.setdefault(b, {})
        node.setdefault(-1, []).append(t)
    return root


def allowed_tokens(trans, ns, state, stack, trie):
    """(ids whose walk never dies, a table error was met)."""
    out, bad = [], False
    todo = [(trie, state, stack, 0)]
    while todo:
        node, s, stk, held = todo.pop()
        out += node.get(-1, ())
        for b, child in node.items():
            if b == -1:
                continue
            r = byte_step(trans, ns, s, stk, held, b)
            if r == BAD:
                bad = True
            elif r != DEAD:
                todo.append((child,) + r)
    return out, bad


def slot_step(c, slot, advance_tok, vocab):
    """One slot of one launch: None (a table error: nothing may be written) or (state, stack, flags, allowed ids).
    c: a case (build_case) or a corrupted copy of one."""
    sb, ns, eos = (int(v) for v in c["desc"][slot][:3])
    arena = min(len(c["trans"]), len(c["accept"]))
    state, depth = int(c["cur"][slot]), int(c["sdep"][slot])
    if sb < 0 or ns < 1 or ns > 16384 or sb + ns > arena or not 0 <= state <= ns or not 0 <= depth <= DEPTH_CAP or \
            not 0 <= eos < vocab:
        return None
    stack = [int(v) for v in c["sstk"][slot][:depth]]
    if any(not 0 <= v < ns for v in stack):
        return None
    trans, accept = c["trans"][sb:sb + ns], c["accept"][sb:sb + ns]
    off, data = c["tok_off"], c["tok_bytes"]
    n_tok = len(off) - 1
    lim = min(vocab, n_tok)
    flags = 0
    if advance_tok is not None:
        t = int(advance_tok)
        if t == eos:
            if state == ns or (accept[state] and not stack):
                state = ns
            else:
                flags = ERR_NO_EDGE
        elif state == ns or not 0 <= t < lim:
            flags = ERR_NO_EDGE
        else:
            lo, hi = int(off[t]), int(off[t + 1])
            if not 0 <= lo <= hi <= len(data):
                return None
            if hi == lo or hi - lo > MAX_TOKEN_BYTES:
                flags = ERR_NO_EDGE
            else:
                r = feed(trans, ns, state, stack, bytes(data[lo:hi]))
                if r == BAD:
                    return None
                if r == DEAD:
                    flags = ERR_NO_EDGE
                else:
                    state, stack = r
    if state == ns:
        return state, stack, flags, [eos]
    lo, hi = off[:lim].astype(np.int64), off[1:lim + 1].astype(np.int64)
    if ((lo < 0) | (hi < lo) | (hi > len(data))).any():
        return None
    key = (id(c["tok_off"]), id(c["tok_bytes"]), lim)
    trie = _TRIES.get(key)
    if trie is None:
        toks = [bytes(data[a:b]) for a, b in zip(lo, hi)]
        trie = _TRIES[key] = (make_trie(toks, lim), c["tok_off"], c["tok_bytes"])   # the arrays: ids stay unique
    ids, bad = allowed_tokens(trans, ns, state, stack, trie[0])
    if bad:
        return None
    ids = [t for t in ids if t != eos]
    if accept[state] and not stack:
        ids.append(eos)
    return state, stack, flags, ids


_TRIES = {}


def run_oracle(c, rows, stride, with_advance, with_lm, row_slot=None, advance=None, bits=None):
    """(row bits uint16 [rows, stride], cur, sdep, sstk, err, lm uint32 [rows, LM_PARTS, 2] | None) after one launch;
    sstk is compared in its live part only (entries at or above the depth are never read)."""
    vocab = c["vocab"]
    out = np.full((rows, stride), 0x447A, dtype=np.uint16)
    out[:, :vocab] = (c["bits"] if bits is None else bits)[:rows]
    cur, sdep, sstk = c["cur"].copy(), c["sdep"].copy(), c["sstk"].copy()
    err = np.zeros(SLOTS, dtype=np.int32)
    lm = start_lm(rows) if with_lm else None
    if row_slot is None:
        row_slot = (ROW_SLOT_ADV if with_advance else ROW_SLOT_PLAIN)[:rows]
    if with_advance and advance is None:
        advance = c["advance"][:rows]
    for r in range(rows):
        slot = int(row_slot[r])
        if slot < 0 or slot >= len(c["desc"]):
            continue
        res = slot_step(c, slot, advance[r] if with_advance else None, vocab)
        if res is None:
            err[slot] |= ERR_TABLE
            continue
        state, stack, flags, ids = res
        cur[slot], sdep[slot] = state, len(stack)
        sstk[slot, :len(stack)] = stack
        err[slot] |= flags
        keep = np.zeros(vocab, dtype=bool)
        keep[ids] = True
        out[r, :vocab] = np.where(keep, out[r, :vocab], 0xFF80)
        if with_lm:
            vals = (out[r, :vocab].astype(np.uint32) << 16).view(np.float32)
            best_v, best_i = np.float32(-np.inf), 0x7FFFFFFF
            idx = np.nonzero(keep)[0]
            if len(idx):
                v = vals[idx]
                ok = ~np.isnan(v)
                if ok.any():
                    m = v[ok].max()
                    first = idx[ok][v[ok] == m][0]
                    best_v, best_i = vals[first], int(first)
            lm[r, :, 0] = np.float32(-np.inf).view(np.uint32)
            lm[r, :, 1] = 0x7FFFFFFF
            lm[r, 0, 0] = np.float32(best_v).view(np.uint32)
            lm[r, 0, 1] = best_i
    return out, cur, sdep, sstk, err, lm


def live_equal(got_sdep, got_sstk, want_sdep, want_sstk):
    if not np.array_equal(got_sdep, want_sdep):
        return False
    return all(np.array_equal(got_sstk[s, :d], want_sstk[s, :d]) for s, d in enumerate(want_sdep) if 0 <= d <= DEPTH_CAP)


# ------------------------------------------------------------------ a validator for the supported schema subset
def _type_ok(v, t):
    if t == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    return {"object": isinstance(v, dict), "array": isinstance(v, list), "string": isinstance(v, str),
            "number": isinstance(v, (int, float)) and not isinstance(v, bool), "boolean": isinstance(v, bool),
            "null": v is None}[t]


def validate(v, s, root=None):
    """v is valid against schema s (the subset of src/guided_schema.py; objects with properties are closed)."""
    import re

    root = s if root is None else root
    if s is True or s == {}:
        return True
    if "$ref" in s:
        p = s["$ref"]
        target = root if p == "#" else root[p.split("/")[1]][p.split("/")[2]]
        return validate(v, target, root)
    if "anyOf" in s:
        return any(validate(v, x, root) for x in s["anyOf"])
    if "allOf" in s:
        return all(validate(v, x, root) for x in s["allOf"])
    if "enum" in s:
        return any(type(v) is type(x) and v == x for x in s["enum"])
    if "const" in s:
        return type(v) is type(s["const"]) and v == s["const"]
    t = s.get("type")
    if t is not None and not any(_type_ok(v, x) for x in ([t] if isinstance(t, str) else t)):
        return False
    if isinstance(v, dict) and s.get("properties"):
        props, req = s["properties"], s.get("required", [])
        if any(k not in props for k in v) or any(k not in v for k in req):
            return False
        return all(validate(x, props[k], root) for k, x in v.items())
    if isinstance(v, dict) and s.get("additionalProperties") is False and v:
        return False
    if isinstance(v, list):
        if not s.get("minItems", 0) <= len(v) <= s.get("maxItems", 1 << 30):
            return False
        return all(validate(x, s.get("items", True), root) for x in v)
    if isinstance(v, str):
        if not s.get("minLength", 0) <= len(v) <= s.get("maxLength", 1 << 30):
            return False
        if "pattern" in s and re.fullmatch(s["pattern"][1:-1], v) is None:
            return False
    return True


# ------------------------------------------------------------------ the shared kernel case
SLOTS = 16
LM_PARTS = 3
ARENA = 512            # states of the case's arenas: both guides' regions and room around them
BASES = (7, 140)       # where the two guides' regions start
SCHEMA_ANY = {"type": "object"}
SCHEMA_TREE = {"type": "object",
               "properties": {"pt": {"type": "object", "properties": {"x": {"type": "integer"}}, "required": ["x"]},
                              "kids": {"type": "array", "items": {"$ref": "#"}},
                              "name": {"type": "string", "maxLength": 12}},   # a guide larger than the first
               "required": ["pt"]}
DEEP31 = '{"k":' + "[" * 30
DEEP32 = '{"k":' + "[" * 31
# (guide, prefix text | None, fabricated (state of prefix, stack)) per slot; the last slots are fabricated
STARTS = (
    (0, ""),                         # 0: depth 0, the start state: only '{' (a push)
    (0, "{"),                        # 1: depth 1, inside the any-object frame
    (0, '{"k":[1,{"a":"x\\'),        # 2: inside an escape, depth 3
    (0, '{"k":-12'),                 # 3: inside a number in a frame: '}' pops, ',' goes on
    (0, DEEP31),                     # 4: depth 31: one more push is legal, two are not
    (0, DEEP32),                     # 5: depth 32: a push is no transition
    (0, DEEP32 + "1"),               # 6: depth 32 in a number: ']' pops, tokens pop several levels and push again
    (0, "{}"),                       # 7: accepting at depth 0
    (1, '{"pt":{"x":1'),             # 8: inside an inlined container, depth 1
    (1, '{"pt":{"x":1},"kids":[{"pt":{"x":0}}'),   # 9: after a frame returned into an array of frames
    (1, '{"pt":{"x":1},"kids":['),   # 10: depth 1, where '{' pushes and ']' closes an inlined array
    (0, b'{"k":"\xe2'),              # 11: inside a multi-byte character
)
SLOT_SINK, SLOT_ACCEPT_DEEP = 12, 13   # the sink; an accepting state at depth 1 (fabricated: EOS is barred)
ROW_SLOT_PLAIN = (1, -1, 4, 7, 9)
ROW_SLOT_ADV = (3, -1, 5, 7, 8)
ALL_SLOTS = tuple(range(14))

_FRAGMENTS = ['{', '}', '[', ']', '"', ':', ',', ', ', ': ', '{"', '"}', '":', '",', '"k"', '"pt"', '"x"', '"kids"',
              '{}', '[]', '[[', ']]', '}}', '1', '0', '-', '12', '.5', 'e3', 'true', 'false', 'null', 'a', 'kids',
              'pt', 'x', '\\', '\\n', '\\u00e9', 'é', '☃', ' ', '],[', '},{"', ']],[[', '"a":', '{"a":', '[1,', ',1]',
              '}]', ']}', '":{"', '":[', '{"pt":{"x":', '"x":1}', '"kids":[', 'x":1},"kids":[{"pt":']


def start_lm(rows):
    lm = np.zeros((rows, LM_PARTS, 2), dtype=np.uint32)
    lm[:, :, 0] = np.float32(3.0).view(np.uint32)
    lm[:, :, 1] = 7
    return lm


def token_table(vocab, seed=20):
    """A seeded byte table, shorter than the vocabulary: every single byte, the tokens the contract names (four and
    five live pushes, pops below the start depth followed by pushes, 0 and 40 bytes), then random runs of JSON
    fragments."""
    rng = random.Random(seed)
    n_tok = vocab - 37
    toks = [b"", b"", b"<eos>"] + [bytes([i]) for i in range(256)]
    toks += [b"[[[[", b"[[[[[", b'{"a":{"a":{"a":{"a":', b'{"a":{"a":{"a":{"a":{', b"]]]]", b"]]]]]", b"]],[[", b"]]],[[[",
             b'},"b":{"c":[', b"]]]],[[[[", b"]]]]],[[[[[", b"", b"x" * 40, b'"' + b"y" * 31, b'"' + b"y" * 32,
             b"]" * 31 + b"}", b"1]]" + b"]" * 29, b'{"pt":{"x":7},"kids":[{"pt":{"x":', b'}],"kids":[]}', b"}}]}",
             b'},"kids":[{"pt":{"x":']
    while len(toks) < n_tok:
        k = rng.randint(1, 6)
        t = "".join(rng.choice(_FRAGMENTS) for _ in range(k)).encode("utf-8")
        toks.append(t[:40] if rng.random() < 0.98 else b"")
    return toks[:n_tok]


@functools.lru_cache(maxsize=None)
def build_case(vocab):
    """Tables, start configurations, advance tokens and logits bits for ``vocab``; numpy arrays, never modified."""
    from src import guided

    eos = 2
    toks = token_table(vocab)
    off = np.zeros(len(toks) + 1, dtype=np.int32)
    np.cumsum([len(t) for t in toks], out=off[1:])
    data = np.frombuffer(b"".join(toks), dtype=np.uint8).copy()
    trans = np.full((ARENA, 256), -1, dtype=np.int32)
    accept = np.zeros(ARENA, dtype=np.uint8)
    tables = []
    for base, schema in zip(BASES, (SCHEMA_ANY, SCHEMA_TREE)):
        t, a = guided.schema_to_pda(schema)
        assert base + len(t) <= ARENA and (not tables or base >= BASES[0] + len(tables[0][0]))
        trans[base:base + len(t)] = t
        accept[base:base + len(t)] = a
        tables.append((t, a))
    desc = np.zeros((SLOTS, 4), dtype=np.int32)
    cur = np.zeros(SLOTS, dtype=np.int32)
    sdep = np.zeros(SLOTS, dtype=np.int32)
    sstk = np.full((SLOTS, DEPTH_CAP), 0x5A5A & 0x3FFF, dtype=np.int16)   # above the depth: never read
    for slot in range(SLOTS):
        g, text = STARTS[slot] if slot < len(STARTS) else (0, "{}")
        t, a = tables[g]
        desc[slot] = (BASES[g], len(t), eos, 0)
        state, stack = text_config(t, len(t), text)
        if slot == SLOT_SINK:
            state = len(t)
        elif slot == SLOT_ACCEPT_DEEP:
            stack = [1]
        cur[slot], sdep[slot] = state, len(stack)
        sstk[slot, :len(stack)] = stack
    rng = np.random.default_rng(vocab)
    bits = rng.integers(0, 1 << 16, size=(5, vocab), dtype=np.uint16)
    bits[0, :64] = 0x7FC0                      # NaNs: never the best candidate
    bits[2, 5:9] = 0x7F80                      # +inf, tied: the lowest allowed index wins
    tid = {t: i for i, t in reversed(list(enumerate(toks)))}
    # rows 0..4 advance slots ROW_SLOT_ADV: ']' in a number of an object frame (no edge, the configuration is kept);
    # row 1 is at slot -1; a 32-byte token that ends a number and pops 31 levels from depth 32; EOS from the
    # accepting state at depth 0; a token that closes an inlined container, opens an inlined array and pushes a frame
    # (its held push is written back to the stack)
    advance = np.array([tid[b"]"], 0, tid[b"1]]" + b"]" * 29], eos, tid[b'},"kids":[{"pt":{"x":']], dtype=np.int64)
    return {"vocab": vocab, "eos": eos, "tokens": toks, "tok_off": off, "tok_bytes": data, "trans": trans,
            "accept": accept, "desc": desc, "cur": cur, "sdep": sdep, "sstk": sstk, "bits": bits, "advance": advance,
            "tables": tables, "tid": tid}


def corruptions(c):
    """(name, {array name: corrupted copy}, slots that must report a table error) — every corrupt value lies outside
    the guide's region but inside the allocated arena, stack or byte table, so a missed check shows up as a
    mismatch, never as an access outside an allocation. The configurations used read the corrupted entry."""
    base, ns = int(c["desc"][1][0]), int(c["desc"][1][1])
    state1 = int(c["cur"][1])
    out = []

    def with_entry(name, value, slot=1, byte=ord('"')):
        t = c["trans"].copy()
        t[int(c["desc"][slot][0]) + int(c["cur"][slot]), byte] = value
        out.append((name, {"trans": t}, (slot,)))

    good = int(c["trans"][base + state1, ord('"')])
    assert good >= 0
    with_entry("next state beyond the region", ns + 3)
    with_entry("return state beyond the region", (good & 0x3FFF) | ((ns + 1) << 14) | (1 << 28))
    with_entry("action 3", good | (3 << 28))
    with_entry("bit 30", good | (1 << 30))
    with_entry("negative but not -1", -2)
    with_entry("pop at depth 0", 2 << 28, slot=0, byte=ord("{"))
    for name, slot, arr, value in (("state beyond the region", 1, "cur", ns + 1), ("negative state", 1, "cur", -1),
                                   ("depth 33", 1, "sdep", 33), ("negative depth", 1, "sdep", -1)):
        a = c[arr].copy()
        a[slot] = value
        out.append((name, {arr: a}, (slot,)))
    s = c["sstk"].copy()
    s[4, 17] = ns + 2
    out.append(("a live stack entry beyond the region", {"sstk": s}, (4,)))
    s = c["sstk"].copy()
    s[4, 3] = -1
    out.append(("a negative live stack entry", {"sstk": s}, (4,)))
    for name, col, value in (("region beyond the arena", 0, ARENA - ns + 1), ("negative base", 0, -1),
                             ("no states", 1, 0), ("eos beyond the vocabulary", 2, c["vocab"])):
        d = c["desc"].copy()
        d[1, col] = value
        out.append((name, {"desc": d}, (1,)))
    o = c["tok_off"].copy()
    o[300] = o[301] + 1                      # descending, still inside the byte table
    out.append(("descending offsets", {"tok_off": o}, (1, 4)))
    return out


def dumps(v):
    return json.dumps(v, separators=(",", ":"), ensure_ascii=False)
