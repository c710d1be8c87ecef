"""The plain-Python oracle of ops.json_guide (csrc/kernels/json_guide.hip, src/ops/reference.py json_guide_rows).

The recogniser below is written straight from the grammar of guided_json_object, independently of the table in
src/guided.py: an explicit stack of container kinds and a named mode, one byte at a time.

    doc     := object                      then only EOS
    object  := '{' '}' | '{' member (',' sp? member)* '}'
    member  := string ':' sp? value
    array   := '[' ']' | '[' value (',' sp? value)* ']'
    value   := object | array | string | number | 'true' | 'false' | 'null'
    sp      := one byte 0x20
    string  := '"' ( char | escape )* '"'      char: well-formed UTF-8 >= U+0020 but '"' and '\\'
    escape  := '\\' one of " \\ / b f n r t  |  '\\u' four hex digits
    number  := -? (0 | [1-9][0-9]*) (\\.[0-9]+)? ([eE][+-]?[0-9]+)?

At most MAX_DEPTH containers are open at once; a '{' or '[' at the cap is not legal.

The op's oracle (json_guide) works on PREFIXES: a slot's configuration is named by the bytes read so far (and whether
EOS was read), from which the recogniser derives the allowed set, the error word, the depth and the stack bits on its
own. Only the number of the resulting control state is taken from the table under test (a state's number is the
builder's choice; tests/test_json_guide_reference_cpu.py checks table and recogniser against each other byte by byte).
Also the seeded case the kernel and CPU tests share (build_case)."""

import numpy as np

NINF_BF16 = 0xFF80
NINF_F32 = 0xFF800000
NO_INDEX = 0x7FFFFFFF
ERR_NO_EDGE, ERR_TABLE = 1, 2
MAX_TOKEN_BYTES = 32      # GUIDE_MAX_TOKEN_BYTES
MAX_DEPTH = 32            # GUIDE_JSON_MAX_DEPTH

_DIGITS = frozenset(b"0123456789")
_HEX = frozenset(b"0123456789abcdefABCDEF")
_NUM_END = ("zero", "int", "frac", "exp")     # modes in which a number may end


# ------------------------------------------------------------------ the recogniser
# A configuration is (mode, aux, stack): stack a tuple of "o" / "a", innermost last. None: the prefix is not legal.
START = ("doc", None, ())


def _close(stack, kind):
    if not stack or stack[-1] != kind:
        return None
    stack = stack[:-1]
    return ("after" if stack else "done", None, stack)


def _value(b, stack):
    """A value starts with byte b."""
    if b in (0x7B, 0x5B):                     # { [
        if len(stack) >= MAX_DEPTH:
            return None
        return ("obj_first", None, stack + ("o",)) if b == 0x7B else ("arr_first", None, stack + ("a",))
    if b == 0x22:
        return ("str", "val", stack)
    if b == 0x2D:
        return ("minus", None, stack)
    if b == 0x30:
        return ("zero", None, stack)
    if b in _DIGITS:
        return ("int", None, stack)
    for word in (b"true", b"false", b"null"):
        if b == word[0]:
            return ("lit", word[1:], stack)
    return None


def _after(b, stack):
    """Byte b after a complete value."""
    if b == 0x2C:
        return ("comma", None, stack)
    if b == 0x7D:
        return _close(stack, "o")
    if b == 0x5D:
        return _close(stack, "a")
    return None


def feed(cfg, b):
    """The configuration after byte b, or None."""
    mode, aux, stack = cfg
    if mode == "doc":
        return ("obj_first", None, ("o",)) if b == 0x7B else None
    if mode == "done":
        return None
    if mode == "obj_first":
        if b == 0x22:
            return ("str", "key", stack)
        return _close(stack, "o") if b == 0x7D else None
    if mode == "arr_first":
        return _close(stack, "a") if b == 0x5D else _value(b, stack)
    if mode == "key_done":
        return ("colon", None, stack) if b == 0x3A else None
    if mode == "colon":
        return ("value", None, stack) if b == 0x20 else _value(b, stack)
    if mode == "value":
        return _value(b, stack)
    if mode == "after":
        return _after(b, stack)
    if mode == "comma":
        if stack[-1] == "o":
            if b == 0x20:
                return ("key_sp", None, stack)
            return ("str", "key", stack) if b == 0x22 else None
        return ("value", None, stack) if b == 0x20 else _value(b, stack)
    if mode == "key_sp":
        return ("str", "key", stack) if b == 0x22 else None
    if mode == "lit":
        if b != aux[0]:
            return None
        return ("lit", aux[1:], stack) if len(aux) > 1 else ("after", None, stack)
    # ---- strings: aux is the role ("key" / "val"), or (role, ...) inside an escape or a character
    if mode == "str":
        if b == 0x22:
            return ("key_done" if aux == "key" else "after", None, stack)
        if b == 0x5C:
            return ("esc", aux, stack)
        if 0x20 <= b < 0x80:
            return cfg
        # a leading byte: (continuation bytes to go, the range of the next one)
        if 0xC2 <= b <= 0xDF:
            return ("utf", (aux, 1, 0x80, 0xBF), stack)
        if b == 0xE0:
            return ("utf", (aux, 2, 0xA0, 0xBF), stack)       # no overlongs
        if b == 0xED:
            return ("utf", (aux, 2, 0x80, 0x9F), stack)       # no surrogates
        if 0xE1 <= b <= 0xEF:
            return ("utf", (aux, 2, 0x80, 0xBF), stack)
        if b == 0xF0:
            return ("utf", (aux, 3, 0x90, 0xBF), stack)       # no overlongs
        if 0xF1 <= b <= 0xF3:
            return ("utf", (aux, 3, 0x80, 0xBF), stack)
        if b == 0xF4:
            return ("utf", (aux, 3, 0x80, 0x8F), stack)       # nothing above U+10FFFF
        return None
    if mode == "utf":
        role, left, lo, hi = aux
        if not lo <= b <= hi:
            return None
        return ("str", role, stack) if left == 1 else ("utf", (role, left - 1, 0x80, 0xBF), stack)
    if mode == "esc":
        if b in b'"\\/bfnrt':
            return ("str", aux, stack)
        return ("hex", (aux, 4), stack) if b == 0x75 else None
    if mode == "hex":
        role, left = aux
        if b not in _HEX:
            return None
        return ("str", role, stack) if left == 1 else ("hex", (role, left - 1), stack)
    # ---- numbers
    if mode == "minus":
        if b == 0x30:
            return ("zero", None, stack)
        return ("int", None, stack) if b in _DIGITS else None
    if mode in ("zero", "int"):
        if mode == "int" and b in _DIGITS:
            return cfg
        if b == 0x2E:
            return ("dot", None, stack)
        if b in b"eE":
            return ("e", None, stack)
        return _after(b, stack)
    if mode == "dot":
        return ("frac", None, stack) if b in _DIGITS else None
    if mode == "frac":
        if b in _DIGITS:
            return cfg
        return ("e", None, stack) if b in b"eE" else _after(b, stack)
    if mode == "e":
        if b in b"+-":
            return ("esign", None, stack)
        return ("exp", None, stack) if b in _DIGITS else None
    if mode == "esign":
        return ("exp", None, stack) if b in _DIGITS else None
    if mode == "exp":
        return cfg if b in _DIGITS else _after(b, stack)
    raise AssertionError(mode)


def feed_all(cfg, data):
    for b in data:
        cfg = feed(cfg, b)
        if cfg is None:
            return None
    return cfg


def config_of(prefix: bytes):
    cfg = feed_all(START, prefix)
    assert cfg is not None, prefix
    return cfg


def accepts_prefix(data: bytes) -> bool:
    return feed_all(START, data) is not None


def accepts(data: bytes) -> bool:
    cfg = feed_all(START, data)
    return cfg is not None and cfg[0] == "done"


def legal_next(cfg) -> frozenset:
    return frozenset(b for b in range(256) if feed(cfg, b) is not None)


def depth_bits(cfg):
    stack = cfg[2]
    return len(stack), sum(1 << i for i, kind in enumerate(stack) if kind == "a")


# ------------------------------------------------------------------ the op
def bf16_value(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << 16).view(np.float32)


def best_allowed(bits_row: np.ndarray, allowed: np.ndarray):
    """(fp32 bit pattern, index) of the largest allowed value, the lowest index among equals; NaN never wins;
    (-inf, 0x7fffffff) when nothing qualifies."""
    vals = bf16_value(bits_row)
    idx = np.nonzero(allowed & ~np.isnan(vals))[0]
    if not len(idx):
        return NINF_F32, NO_INDEX
    top = vals[idx].max()
    first = int(idx[vals[idx] == top][0])
    return int(vals[first:first + 1].view(np.uint32)[0]), first


def token_feed(cfg, t, table):
    """The configuration after token t's bytes, or None: no bytes, beyond the table, over the cap, or not legal."""
    bs = table[t] if 0 <= t < len(table) else None
    if not bs or len(bs) > MAX_TOKEN_BYTES:
        return None
    return feed_all(cfg, bs)


_ALLOWED = {}


def allowed_set(prefix, in_sink, eos, vocab, table, memo=None):
    """bool [vocab]: the tokens allowed after `prefix` (in_sink: EOS was read after it)."""
    key = None if memo is None else (memo, prefix, in_sink)
    if key is not None and key in _ALLOWED:
        return _ALLOWED[key]
    allowed = np.zeros(vocab, dtype=bool)
    if in_sink:
        allowed[eos] = True
    else:
        cfg = config_of(prefix)
        first = legal_next(cfg)
        for t in range(min(vocab, len(table))):
            bs = table[t]
            allowed[t] = bool(bs) and bs[0] in first and token_feed(cfg, t, table) is not None
        allowed[eos] = cfg[0] == "done"
    if key is not None:
        _ALLOWED[key] = allowed
    return allowed


def device_config(trans, n_states, prefix, in_sink):
    """(state, depth, bits) of a prefix: depth and bits from the recogniser, the state's number from the table."""
    from src.guided import json_step

    c = (0, 0, 0)
    for b in prefix:
        c = json_step(trans, c, b)
    depth, bits = depth_bits(config_of(prefix))
    assert (c[1], c[2]) == (depth, bits), prefix
    return (n_states if in_sink else c[0]), depth, bits


def json_guide(bits, slot, starts, trans, eos, table, vocab, err, advance=None, lm=None, memo=None):
    """The op on rows of raw uint16 bits, in place. starts[slot] = (prefix, in_sink) is modified in place too (the
    configuration after the advance). err int32 [slots]."""
    lim = min(vocab, len(table))
    for r in range(bits.shape[0]):
        s = int(slot[r])
        if s < 0 or s >= len(starts):
            continue
        prefix, in_sink = starts[s]
        if advance is not None:
            tok = int(advance[r])
            cfg = config_of(prefix)
            if tok == eos:
                if in_sink or cfg[0] == "done":
                    in_sink = True
                else:
                    err[s] |= ERR_NO_EDGE
            elif in_sink or not 0 <= tok < lim or token_feed(cfg, tok, table) is None:
                err[s] |= ERR_NO_EDGE
            else:
                prefix = prefix + table[tok]
        starts[s] = (prefix, in_sink)
        allowed = allowed_set(prefix, in_sink, eos, vocab, table, memo)
        row = bits[r, :vocab]
        row[~allowed] = NINF_BF16
        if lm is not None:
            lm[r, :, 0] = NINF_F32
            lm[r, :, 1] = NO_INDEX
            lm[r, 0, 0], lm[r, 0, 1] = best_allowed(row, allowed)


# ------------------------------------------------------------------ the shared test case
PARTS = 5
EOS = 1
FIRST_BYTE_ID = 2             # ids 2..257 are the 256 single bytes
KEY = b'{"k":'
# the chosen multi-byte tokens, ids 258...
SPECIAL = (KEY, b"}}", b"[[", b"[{", b'"},{"', b'y":', b"a" * MAX_TOKEN_BYTES, b"a" * (MAX_TOKEN_BYTES + 1), b"",
           b'":[', b"]}", b"1,", b"\xf0\x9f\x98\x80", b"\x82\xac", b"e+5", b'{"a":{"b":[[{}]]}}', b"true}", b".5e-3]")
ID_KEY, ID_CLOSE2, ID_ARR2, ID_ARR_OBJ, ID_POP_PUSH, ID_KEY_END, ID_CAP, ID_OVER, ID_EMPTY = range(258, 267)


def byte_id(ch) -> int:
    return FIRST_BYTE_ID + (ch if isinstance(ch, int) else ord(ch))


# every start configuration of the kernel test: name -> (prefix, EOS was read)
STARTS = (
    ("start", b"", False),
    ("in_key", b'{"ke', False),
    ("after_backslash", b'{"k":"a\\', False),
    ("in_u", b'{"k":["\\u0a', False),
    ("utf3_1", b'{"k":"\xe2', False),
    ("utf3_2", b'{"k":["\xe2\x82', False),
    ("utf4_1", b'{"k":"\xf0', False),
    ("utf4_3", b'{"\xf0\x9f\x98', False),
    ("after_minus", b'{"k":-', False),
    ("after_zero", b'{"k":[0', False),
    ("in_fraction", b'{"k":[1.5', False),
    ("in_exponent", b'{"k":1e+2', False),
    ("after_value_object", b'{"k":"v"', False),
    ("after_value_array", b'{"k":[{"a":"x"}', False),
    ("in_string_in_object_in_array", b'{"k":[{"a":"x', False),
    ("done", b"{}", False),
    ("sink", b'{"k":[]}', True),
    ("depth32_value", KEY * 32, False),
    ("depth31_value", KEY * 31, False),
    ("depth32_array_value", KEY + b"[" * 31, False),
    ("depth1_number", b'{"k":1', False),
    ("in_literal", b'{"k":[tr', False),
    ("after_colon_space", b'{"k": ', False),
)
SLOTS = len(STARTS)
SLOT = {name: i for i, (name, _, _) in enumerate(STARTS)}
# the grid's rows: row r -> slot; row 1 is not guided. Without an advance the rows are masked inside a key, in the
# sink, at depth 31 before a value and after a value in an array. With one they read 'y":' inside a key (three bytes,
# into the colon state), EOS in DONE (-> the sink), '{"k":' at depth 31 (a push: depth 32) and EOS after a value
# (GUIDE_ERR_NO_EDGE, the configuration is kept).
ROW_SLOT_PLAIN = (SLOT["in_key"], -1, SLOT["sink"], SLOT["depth31_value"], SLOT["after_value_array"])
ROW_SLOT_ADV = (SLOT["in_key"], -1, SLOT["done"], SLOT["depth31_value"], SLOT["after_value_object"])


def build_vocab(vocab: int, rng):
    """id -> bytes for ids [0, vocab - 40): the table is SHORTER than the vocabulary. 0 (pad) and 1 (EOS) have no
    bytes; 2..257 the single bytes; then SPECIAL; the rest 0..40 bytes over an alphabet rich in JSON punctuation
    (short ones more often, so that many survive a few transitions)."""
    n_tok = vocab - 40
    alphabet = b'{}[]",:: 00123456789-.eEtruefalsn\\uabk""' + b"\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80"
    table = [b"", b""] + [bytes([b]) for b in range(256)] + list(SPECIAL)
    while len(table) < n_tok:
        n = int(rng.integers(0, 41)) if len(table) % 5 == 0 else int(rng.integers(1, 6))
        table.append(bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=n)))
    off = np.zeros(n_tok + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(b) for b in table])
    data = np.frombuffer(b"".join(table), dtype=np.uint8).copy()
    return table, off, data


def build_case(vocab: int):
    """The seeded byte table, logits bit patterns and the start configurations (STARTS), the same for every
    vocabulary. The table under test is src.guided's (the op's argument); desc / cur / jstk are derived from it by
    device_config. Returns a dict; nothing in it is modified by the tests (they copy)."""
    from src.guided import build_json_table

    rng = np.random.default_rng(vocab)
    table, off, data = build_vocab(vocab, rng)
    trans, done = build_json_table()
    n = trans.shape[0]
    desc = np.zeros((SLOTS, 4), dtype=np.int32)
    desc[:] = (n, done, EOS, 0)
    cur = np.zeros(SLOTS, dtype=np.int32)
    jstk = np.zeros((SLOTS, 2), dtype=np.int32)
    for i, (_, prefix, in_sink) in enumerate(STARTS):
        c, d, k = device_config(trans, n, prefix, in_sink)
        cur[i], jstk[i, 0] = c, d
        jstk[i, 1] = np.array([k], dtype=np.uint32).view(np.int32)[0]
    advance = np.array([ID_KEY_END, 12345 % vocab, EOS, ID_KEY, EOS], dtype=np.int64)
    x = rng.integers(-3, 5, size=(5, vocab)).astype(np.float32)   # integers: ties
    x[:, 40] = -0.0
    x[3, 41] = np.nan
    x[0, byte_id("a")] = -np.inf
    bits = (x.view(np.uint32) >> 16).astype(np.uint16)            # exact in bf16
    return {"vocab": vocab, "bits": bits, "desc": desc, "trans": trans, "done": done, "tok_off": off,
            "tok_bytes": data, "table": table, "cur": cur, "jstk": jstk, "advance": advance}


def start_lm(rows: int) -> np.ndarray:
    """Candidates as an LM head might leave them: something in every part, so that every part must be rewritten."""
    lm = np.zeros((rows, PARTS, 2), dtype=np.uint32)
    lm[:, :, 0] = np.float32(3.5).view(np.uint32)
    lm[:, :, 1] = np.arange(PARTS, dtype=np.uint32)[None, :] + 17
    return lm


def expected_state(case, starts):
    """(cur, jstk) of the configurations in `starts`."""
    n = case["trans"].shape[0]
    cur = np.zeros(len(starts), dtype=np.int32)
    jstk = np.zeros((len(starts), 2), dtype=np.int32)
    for i, (prefix, in_sink) in enumerate(starts):
        c, d, k = device_config(case["trans"], n, prefix, in_sink)
        cur[i], jstk[i, 0] = c, d
        jstk[i, 1] = np.array([k], dtype=np.uint32).view(np.int32)[0]
    return cur, jstk


def run_oracle(case, rows, stride: int, with_advance: bool, with_lm: bool, row_slot=None, bits=None, advance=None):
    """The oracle's outputs for `rows` rows of the case at row stride `stride`: (bits [rows, stride], cur, jstk, err,
    lm or None). The padding beyond the vocabulary holds 0x447A (1000.0) and must stay. row_slot defaults to the
    grid's mapping."""
    vocab = case["vocab"]
    if row_slot is None:
        row_slot = (ROW_SLOT_ADV if with_advance else ROW_SLOT_PLAIN)[:rows]
    src = case["bits"] if bits is None else bits
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = src[:rows]
    starts = [(p, s) for _, p, s in STARTS]
    err = np.zeros(SLOTS, dtype=np.int32)
    lm = start_lm(rows) if with_lm else None
    adv = (case["advance"][:rows] if advance is None else advance) if with_advance else None
    json_guide(buf, row_slot, starts, case["trans"], EOS, case["table"], vocab, err, advance=adv, lm=lm,
               memo=("case", vocab))
    cur, jstk = expected_state(case, starts)
    return buf, cur, jstk, err, lm


def engine_table(vocab: int, seed: int = 5):
    """A multi-byte byte table for engine tests, ByteTokenizer's ids kept (0..2 pad / BOS / EOS without bytes, 3..258
    the single bytes), then '{"k":' (ENGINE_KEY) and tokens of 2..8 bytes rich in JSON punctuation; every 89th one
    has no bytes."""
    rng = np.random.default_rng(seed)
    alphabet = b'{}[]",: 0123456789-.eEtruefalsnabk""::,,'
    table = [None, None, None] + [bytes([b]) for b in range(256)] + [KEY]
    while len(table) < vocab:
        if len(table) % 89 == 0:
            table.append(None)
            continue
        n = int(rng.integers(2, 9))
        table.append(bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=n)))
    return table


ENGINE_KEY = 259


def spell(table, ids) -> bytes:
    return b"".join(table[t] or b"" for t in ids)


# every way an advance can fail, and the ones that succeed: (start name, token, expected prefix grows, err)
ADVANCE_KINDS = (
    ("in_key", byte_id(0x0A), False, ERR_NO_EDGE),            # a dead transition: a control character in a string
    ("in_key", ID_EMPTY, False, ERR_NO_EDGE),                 # a token without bytes
    ("in_key", ID_OVER, False, ERR_NO_EDGE),                  # one byte over the cap, in a state that reads them all
    ("in_key", ID_CAP, True, 0),                              # exactly the cap
    ("sink", byte_id("}"), False, ERR_NO_EDGE),               # not EOS, in the sink
    ("sink", EOS, False, 0),                                  # EOS keeps the sink
    ("in_key", ID_KEY_END, True, 0),                          # 'y":': three bytes
    ("after_value_object", EOS, False, ERR_NO_EDGE),          # EOS from a state that is not DONE
    ("done", EOS, False, 0),                                  # EOS from DONE (-> the sink)
    ("start", -1, False, ERR_NO_EDGE),                        # not an id
    ("in_string_in_object_in_array", ID_POP_PUSH, True, 0),   # '"},{"': closes a string, pops, pushes, opens a key
    ("depth32_value", byte_id("{"), False, ERR_NO_EDGE),      # a push at the cap
    ("depth32_value", byte_id("7"), True, 0),                 # every other value is legal there
    ("depth31_value", ID_ARR2, False, ERR_NO_EDGE),           # two pushes from depth 31
    ("depth31_value", byte_id("["), True, 0),                 # one push
    ("depth1_number", ID_CLOSE2, False, ERR_NO_EDGE),         # '}}' at depth 1: the second '}' has nothing to close
    ("depth1_number", byte_id("}"), True, 0),                 # '}' ends the number and the document
)
