"""The plain-Python / numpy oracle of ops.byte_guide (csrc/kernels/byte_guide.hip, src/ops/reference.py
byte_guide_rows): written from the contract, on the rows' raw uint16 bits, one token and one byte at a time, sharing
no code with either implementation.

    byte_guide(bits, slot, desc, trans, accept, tok_off, tok_bytes, cur, err, vocab, advance=None, lm=None)

bits uint16 [rows, stride] (bf16 patterns), slot int [rows], desc int32 [slots, 4] = (state_base, n_states, eos, 0),
trans int16 [A, 256] (-1: no transition), accept uint8 [A], tok_off int32 [n_tok + 1], tok_bytes uint8 [B], cur / err
int32 [slots], lm uint32 [rows, parts, 2]. Everything is modified in place, as the op does. State n_states is the
sink. Also the seeded case the kernel and CPU tests share (build_case)."""

import numpy as np

NINF_BF16 = 0xFF80
NINF_F32 = 0xFF800000
NO_INDEX = 0x7FFFFFFF
ERR_NO_EDGE, ERR_TABLE = 1, 2
MAX_TOKEN_BYTES = 32      # GUIDE_MAX_TOKEN_BYTES
LDS_STATES = 208          # GUIDE_BYTE_LDS_STATES: the kernel walks a guide of up to this many states from LDS


class TableError(Exception):
    """A table value out of its bounds was read."""


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


def token_walk(tr, n_states, state, t, off, data, bytes_len):
    """The state after token t's bytes from `state`, or None: no bytes, over the cap, or a dead transition.
    TableError for an offset or a trans value out of bounds."""
    lo, hi = int(off[t]), int(off[t + 1])
    if not 0 <= lo <= hi <= bytes_len:
        raise TableError
    if hi == lo or hi - lo > MAX_TOKEN_BYTES:
        return None
    s = state
    for p in range(lo, hi):
        s = int(tr[s][data[p]])
        if s < -1 or s >= n_states:
            raise TableError
        if s < 0:
            return None
    return s


_ALLOWED = {}


def allowed_set(tr, ac, n_states, c, eos, vocab, off, data, bytes_len, memo=None):
    """bool [vocab]: the tokens allowed next in state c. memo: a hashable name of (tables, state), for the shared
    cases only (the oracle's answer for them is computed once)."""
    if memo is not None and memo in _ALLOWED:
        return _ALLOWED[memo]
    allowed = np.zeros(vocab, dtype=bool)
    if c == n_states:
        allowed[eos] = True
    else:
        for t in range(min(vocab, len(off) - 1)):
            allowed[t] = token_walk(tr, n_states, c, t, off, data, bytes_len) is not None
        allowed[eos] = bool(ac[c])
    if memo is not None:
        _ALLOWED[memo] = allowed
    return allowed


def byte_guide(bits, slot, desc, trans, accept, tok_off, tok_bytes, cur, err, vocab, advance=None, lm=None, memo=None):
    arena = min(len(trans), len(accept))
    n_tok, bytes_len = len(tok_off) - 1, len(tok_bytes)
    off, data = tok_off.tolist(), tok_bytes.tolist()
    for r in range(bits.shape[0]):
        s = int(slot[r])
        if s < 0 or s >= desc.shape[0]:
            continue
        state_base, n_states, eos = (int(v) for v in desc[s, :3])
        c = int(cur[s])
        if (state_base < 0 or n_states < 1 or state_base + n_states > arena or c < 0 or c > n_states or eos < 0
                or eos >= vocab):
            err[s] |= ERR_TABLE
            continue
        tr = trans[state_base:state_base + n_states].tolist()
        ac = accept[state_base:state_base + n_states]
        flags = 0
        try:
            if advance is not None:
                tok = int(advance[r])
                if tok == eos:
                    if c == n_states or ac[c]:
                        c = n_states
                    else:
                        flags = ERR_NO_EDGE
                elif c == n_states or tok < 0 or tok >= min(vocab, n_tok):
                    flags = ERR_NO_EDGE
                else:
                    nxt = token_walk(tr, n_states, c, tok, off, data, bytes_len)
                    if nxt is None:
                        flags = ERR_NO_EDGE
                    else:
                        c = nxt
            allowed = allowed_set(tr, ac, n_states, c, eos, vocab, off, data, bytes_len,
                                  None if memo is None else (memo, state_base, c))
        except TableError:
            err[s] |= ERR_TABLE
            continue
        cur[s] = c
        err[s] |= flags
        row = bits[r, :vocab]
        row[~allowed] = NINF_BF16
        if lm is not None:
            lm[r, :, 0] = NINF_F32
            lm[r, :, 1] = NO_INDEX
            lm[r, 0, 0], lm[r, 0, 1] = best_allowed(row, allowed)


# ------------------------------------------------------------------ the shared test case
SLOTS = 7
ROW_SLOT = (3, -1, 0, 6, 2)   # row r -> slot; row 1 is not guided
BASE_A, BASE_B = 5, 19        # the regions do not start at the arenas' origin
PARTS = 5
EOS = 1
N_B = 300                     # guide B's states: above LDS_STATES, read through L2; guide A (6) is walked from LDS
FIRST_BYTE_ID = 2             # ids 2..257 are the 256 single bytes
ID_LEN2, ID_LEN16, ID_CAP, ID_OVER, ID_EMPTY = 258, 259, 260, 261, 262


def byte_id(ch) -> int:
    return FIRST_BYTE_ID + (ch if isinstance(ch, int) else ord(ch))


def build_vocab(vocab: int, rng):
    """id -> bytes for ids [0, vocab - 40): the table is SHORTER than the vocabulary, the last 40 ids have no entry.
    0 (pad) and 1 (EOS) have no bytes; 2..257 the single bytes; 258 'ab' (2 bytes), 259 'abcdabcdabcdabcd' (16), 260
    'a' * 32 (exactly the cap), 261 'a' * 33 (one over), 262 no bytes; the rest 2..16 bytes over a small alphabet
    (so that many survive a few transitions), every 97th one without bytes."""
    n_tok = vocab - 40
    alphabet = b"abcd 0123456789-z"
    table = [b"", b""] + [bytes([b]) for b in range(256)] + [b"ab", b"abcd" * 4, b"a" * MAX_TOKEN_BYTES,
                                                              b"a" * (MAX_TOKEN_BYTES + 1), b""]
    while len(table) < n_tok:
        if len(table) % 97 == 0:
            table.append(b"")
            continue
        n = int(rng.integers(2, 17))
        table.append(bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=n)))
    off = np.zeros(n_tok + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(b) for b in table])
    data = np.frombuffer(b"".join(table), dtype=np.uint8).copy()
    return table, off, data


def guide_a():
    """6 states. 0: 'a' -> 1, 'z' -> 2;  1 (accepting): every byte -> 1 (the full vocabulary);  2 (accepting): no
    transition (nothing but EOS);  3: [a-d] -> 3, ' ' -> 4;  4: [0-9] -> 5;  5 (accepting): [0-9] -> 5, '-' -> 3."""
    tr = np.full((6, 256), -1, dtype=np.int16)
    tr[0, ord("a")], tr[0, ord("z")] = 1, 2
    tr[1, :] = 1
    tr[3, ord("a"):ord("d") + 1] = 3
    tr[3, ord(" ")] = 4
    tr[4, ord("0"):ord("9") + 1] = 5
    tr[5, ord("0"):ord("9") + 1] = 5
    tr[5, ord("-")] = 3
    return tr, np.array([0, 1, 1, 0, 0, 1], dtype=np.uint8)


def guide_b():
    """N_B states, a counter: [a-d] -> min(i + 1, N_B - 1), a digit keeps i; every seventh state accepts."""
    tr = np.full((N_B, 256), -1, dtype=np.int16)
    for i in range(N_B):
        tr[i, ord("a"):ord("d") + 1] = min(i + 1, N_B - 1)
        tr[i, ord("0"):ord("9") + 1] = i
    return tr, (np.arange(N_B) % 7 == 0).astype(np.uint8)


def build_case(vocab: int):
    """Two guides in one arena and the states the rows stand in, the same for every vocabulary.
    Without an advance the rows are masked in A1 (the full vocabulary), the sink, B10 and A2 (nothing but EOS);
    with one they start in A0, A5, B10 and A3 and read 'a' (-> A1), EOS from the accepting A5 (-> the sink), the
    16-byte token (-> B26) and EOS from A3, which does not accept (GUIDE_ERR_NO_EDGE, the state is kept).
    Returns a dict of numpy arrays; nothing in it is modified by the tests (they copy)."""
    rng = np.random.default_rng(vocab)
    table, off, data = build_vocab(vocab, rng)
    (ta, aa), (tb, ab) = guide_a(), guide_b()
    n_arena = BASE_B + N_B + 3
    trans = np.full((n_arena, 256), -12345, dtype=np.int16)   # junk outside the regions
    accept = np.full(n_arena, 1, dtype=np.uint8)
    trans[BASE_A:BASE_A + 6], accept[BASE_A:BASE_A + 6] = ta, aa
    trans[BASE_B:BASE_B + N_B], accept[BASE_B:BASE_B + N_B] = tb, ab
    desc = np.zeros((SLOTS, 4), dtype=np.int32)
    desc[:] = (BASE_A, 6, EOS, 0)
    desc[6] = (BASE_B, N_B, EOS, 0)
    cur_plain = np.full(SLOTS, 4, dtype=np.int32)             # slots no row maps to: must stay as they are
    cur_plain[3], cur_plain[0], cur_plain[6], cur_plain[2] = 1, 6, 10, 2
    cur_adv = cur_plain.copy()
    cur_adv[3], cur_adv[0], cur_adv[6], cur_adv[2] = 0, 5, 10, 3
    advance = np.array([byte_id("a"), 12345 % vocab, EOS, ID_LEN16, EOS], dtype=np.int64)
    x = rng.integers(-3, 5, size=(len(ROW_SLOT), vocab)).astype(np.float32)   # integers: ties
    x[:, 40] = -0.0
    x[3, 41] = np.nan
    x[0, byte_id("a")] = -np.inf
    bits = (x.view(np.uint32) >> 16).astype(np.uint16)                        # exact in bf16
    return {"vocab": vocab, "bits": bits, "desc": desc, "trans": trans, "accept": accept, "tok_off": off,
            "tok_bytes": data, "table": table, "cur_plain": cur_plain, "cur_adv": cur_adv, "advance": advance}


def start_lm(rows: int) -> np.ndarray:
    """Candidates as an LM head might leave them: something in every part, so that every part must be rewritten."""
    lm = np.zeros((rows, PARTS, 2), dtype=np.uint32)
    lm[:, :, 0] = np.float32(3.5).view(np.uint32)
    lm[:, :, 1] = np.arange(PARTS, dtype=np.uint32)[None, :] + 17
    return lm


def run_oracle(case, rows: int, stride: int, with_advance: bool, with_lm: bool):
    """The oracle's outputs for the first `rows` rows of the case at row stride `stride`: (bits [rows, stride],
    cur, err, lm or None). The padding beyond the vocabulary holds 0x447A (1000.0) and must stay."""
    vocab = case["vocab"]
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = case["bits"][:rows]
    cur = case["cur_adv" if with_advance else "cur_plain"].copy()
    err = np.zeros(SLOTS, dtype=np.int32)
    lm = start_lm(rows) if with_lm else None
    byte_guide(buf, ROW_SLOT[:rows], case["desc"], case["trans"], case["accept"], case["tok_off"], case["tok_bytes"],
               cur, err, vocab, advance=case["advance"][:rows] if with_advance else None, lm=lm,
               memo=("case", vocab))
    return buf, cur, err, lm


ENGINE_AB, ENGINE_CD = 259, 260


def engine_table(vocab: int, seed: int = 5):
    """A multi-byte byte table for engine tests, ByteTokenizer's ids kept (0..2 pad / BOS / EOS without bytes, 3..258
    the single bytes), then tokens of 2..8 bytes over letters, digits, a space and some punctuation; every 89th
    one has no bytes."""
    rng = np.random.default_rng(seed)
    alphabet = b'abcdefghijklmnopqrstuvwxyz 0123456789-{}":,x'
    table = [None, None, None] + [bytes([b]) for b in range(256)] + [b"ab", b"cd"]     # ENGINE_AB, ENGINE_CD
    while len(table) < vocab:
        if len(table) % 89 == 0:
            table.append(None)
            continue
        n = int(rng.integers(2, 9))
        table.append(bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=n)))
    return table


def spell(table, ids) -> bytes:
    return b"".join(table[t] or b"" for t in ids)


# every way an advance can fail, and the ones that succeed: (start state in guide A, token, expected state, err)
ADVANCE_KINDS = (
    (0, byte_id("q"), 0, ERR_NO_EDGE),      # a dead transition
    (0, ID_EMPTY, 0, ERR_NO_EDGE),          # a token without bytes
    (1, ID_OVER, 1, ERR_NO_EDGE),           # one byte over the cap, in the state that reads every byte
    (1, ID_CAP, 1, 0),                      # exactly the cap
    (6, byte_id("a"), 6, ERR_NO_EDGE),      # not EOS, in the sink
    (6, EOS, 6, 0),                         # EOS keeps the sink
    (0, ID_LEN2, 1, 0),                     # 'ab': two bytes
    (3, EOS, 3, ERR_NO_EDGE),               # EOS from a state that does not accept
    (5, EOS, 6, 0),                         # EOS from one that does
    (0, -1, 0, ERR_NO_EDGE),                # not an id
)
