"""The numpy oracle of ops.token_guide (csrc/kernels/token_guide.hip, src/ops/reference.py token_guide_rows): written
from the contract, on the rows' raw uint16 bits, sharing no code with either implementation.

    token_guide(bits, slot, desc, rowptr, edges, cur, err, vocab, advance=None, lm=None)

bits uint16 [rows, stride] (bf16 patterns), slot int [rows], desc int32 [slots, 4] = (state_base, n_states,
edge_base, n_edges), rowptr int32 [R], edges int32 [E, 2] = (tok, next), cur / err int32 [slots], lm uint32 [rows,
parts, 2]. Everything is modified in place, as the op does."""

import numpy as np

NINF_BF16 = 0xFF80
NINF_F32 = 0xFF800000
NO_INDEX = 0x7FFFFFFF
ERR_NO_EDGE, ERR_TABLE = 1, 2


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
    first = int(idx[vals[idx] == top][0])  # idx ascends: the lowest index among equals
    return int(vals[first:first + 1].view(np.uint32)[0]), first  # that entry's own bits (-0.0 equals +0.0)


def token_guide(bits, slot, desc, rowptr, edges, cur, err, vocab, advance=None, lm=None):
    for r in range(bits.shape[0]):
        s = int(slot[r])
        if s < 0 or s >= desc.shape[0]:
            continue
        state_base, n_states, edge_base, n_edges = (int(v) for v in desc[s])
        c = int(cur[s])
        if (state_base < 0 or n_states < 1 or state_base + n_states + 1 > len(rowptr) or edge_base < 0 or n_edges < 0
                or edge_base + n_edges > len(edges) or c < 0 or c >= n_states):
            err[s] |= ERR_TABLE
            continue

        def edge_range(state):
            lo, hi = int(rowptr[state_base + state]), int(rowptr[state_base + state + 1])
            return (lo, hi) if 0 <= lo <= hi <= n_edges else None

        flags = 0
        if advance is not None:
            rng = edge_range(c)
            if rng is None:
                err[s] |= ERR_TABLE
                continue
            nxt = None
            for e in range(rng[0], rng[1]):
                if int(edges[edge_base + e, 0]) == int(advance[r]):
                    nxt = int(edges[edge_base + e, 1])
                    break
            if nxt is None:
                flags = ERR_NO_EDGE
            elif not 0 <= nxt < n_states:
                err[s] |= ERR_TABLE
                continue
            else:
                c = nxt
        rng = edge_range(c)
        if rng is None:
            err[s] |= ERR_TABLE
            continue
        toks = edges[edge_base + rng[0]: edge_base + rng[1], 0].astype(np.int64)
        if ((toks < 0) | (toks >= vocab)).any():
            err[s] |= ERR_TABLE
            continue
        cur[s] = c
        err[s] |= flags
        allowed = np.zeros(vocab, dtype=bool)
        allowed[toks] = True
        row = bits[r, :vocab]
        row[~allowed] = NINF_BF16
        if lm is not None:
            lm[r, :, 0] = NINF_F32
            lm[r, :, 1] = NO_INDEX
            lm[r, 0, 0], lm[r, 0, 1] = best_allowed(row, allowed)


# ------------------------------------------------------------------ the shared test case
SLOTS = 7
ROW_SLOT = (3, -1, 0, 6, 2)   # row r -> slot; row 1 is not guided
STATE_BASE, EDGE_BASE = 11, 37  # the region does not start at the arenas' origin
PARTS = 5


def build_case(vocab: int):
    """One automaton that holds every edge-list shape the kernel meets, the same for every vocabulary:
        state 0: 1 edge            (token 7 -> 1)
        state 1: ids {0, vocab-1}  (-> 2, -> 3)
        state 2: 1025 edges        (random ids -> 4): one more than the workgroup has threads; a 1024-entry
                                   vocabulary cannot hold 1025 distinct ids: 1000 there
        state 3: the whole vocabulary (token t -> t % 5)
        state 4: 1 edge            (vocab - 1 -> 0)
    Slots 3, 0, 6, 2 stand in states 0, 1, 3, 2; the rows' advance ids move them to states 1, 3, 2 and — a token
    state 2 has no edge for — nowhere (GUIDE_ERR_NO_EDGE). So the rows are masked by 1 edge, {0, vocab-1}, the whole
    vocabulary and 1025 edges without an advance, and by {0, vocab-1}, the whole vocabulary, 1025 and 1025 edges
    with one. Returns a dict of numpy arrays; nothing in it is modified by the tests (they copy)."""
    rng = np.random.default_rng(vocab)
    n_many = min(1025, vocab - 24)
    many = np.sort(rng.choice(np.arange(1, vocab - 1), size=n_many, replace=False)).astype(np.int32)
    per_state = [(np.array([7], np.int32), np.array([1], np.int32)),
                 (np.array([0, vocab - 1], np.int32), np.array([2, 3], np.int32)),
                 (many, np.full(n_many, 4, np.int32)),
                 (np.arange(vocab, dtype=np.int32), (np.arange(vocab) % 5).astype(np.int32)),
                 (np.array([vocab - 1], np.int32), np.array([0], np.int32))]
    n_states = len(per_state)
    n_edges = sum(len(t) for t, _ in per_state)
    rowptr = np.full(STATE_BASE + n_states + 1 + 5, -12345, dtype=np.int32)   # junk outside the region
    edges = np.full((EDGE_BASE + n_edges + 9, 2), -54321, dtype=np.int32)
    at = 0
    for s, (t, n) in enumerate(per_state):
        rowptr[STATE_BASE + s] = at
        edges[EDGE_BASE + at: EDGE_BASE + at + len(t), 0] = t
        edges[EDGE_BASE + at: EDGE_BASE + at + len(t), 1] = n
        at += len(t)
    rowptr[STATE_BASE + n_states] = at
    desc = np.zeros((SLOTS, 4), dtype=np.int32)
    desc[:] = (STATE_BASE, n_states, EDGE_BASE, n_edges)
    cur = np.zeros(SLOTS, dtype=np.int32)
    cur[3], cur[0], cur[6], cur[2] = 0, 1, 3, 2
    cur[1] = cur[4] = cur[5] = 4            # slots no row maps to: must stay as they are
    absent = int(np.setdiff1d(np.arange(1, vocab - 1), many)[3])
    advance = np.array([7, 12345 % vocab, vocab - 1, 5 * 91 + 2, absent], dtype=np.int64)
    x = rng.integers(-3, 5, size=(len(ROW_SLOT), vocab)).astype(np.float32)   # integers: ties
    x[0, 7] = 2.0
    x[:, 40] = -0.0
    x[3, 41] = np.nan
    x[4, int(many[0])] = -np.inf
    bits = (x.view(np.uint32) >> 16).astype(np.uint16)                        # exact in bf16
    return {"vocab": vocab, "bits": bits, "desc": desc, "rowptr": rowptr, "edges": edges, "cur": cur,
            "advance": advance, "many": many}


def run_oracle(case, rows: int, stride: int, with_advance: bool, with_lm: bool):
    """The oracle's outputs for the first `rows` rows of the case at row stride `stride`: (bits [rows, stride],
    cur, err, lm or None). The padding beyond the vocabulary holds 0x447A (1000.0) and must stay."""
    vocab = case["vocab"]
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = case["bits"][:rows]
    cur, err = case["cur"].copy(), np.zeros(SLOTS, dtype=np.int32)
    lm = start_lm(rows) if with_lm else None
    token_guide(buf, ROW_SLOT[:rows], case["desc"], case["rowptr"], case["edges"], cur, err, vocab,
                advance=case["advance"][:rows] if with_advance else None, lm=lm)
    return buf, cur, err, lm


def start_lm(rows: int) -> np.ndarray:
    """Candidates as an LM head might leave them: something in every part, so that every part must be rewritten."""
    lm = np.zeros((rows, PARTS, 2), dtype=np.uint32)
    lm[:, :, 0] = np.float32(3.5).view(np.uint32)
    lm[:, :, 1] = np.arange(PARTS, dtype=np.uint32)[None, :] + 17
    return lm
