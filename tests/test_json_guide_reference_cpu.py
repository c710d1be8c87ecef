"""guided_json_object on the host: the recogniser of tests/json_guide_reference.py (written from the grammar) against
Python's json module, against the pushdown table of src/guided.py byte by byte, and the host implementation of
ops.json_guide (src/ops/reference.py json_guide_rows, the CPU engine's path) against the oracle bit for bit, over the
parameter grid of tests/test_json_guide_kernel_gpu.py. Corrupted tables are checked here for the host implementation
and in the kernel test for the device."""

import functools
import json
import random

import numpy as np
import pytest
import torch

from src import guided
from src.ops import reference

from tests import json_guide_reference as oracle


@functools.lru_cache(maxsize=None)
def table():
    return guided.build_json_table()


def single_byte_guide():
    tb = [None, None, None] + [bytes([b]) for b in range(256)]
    return guided.compile_json_guide(tb, 2), tb


def table_accepts(data: bytes) -> bool:
    trans, done = table()
    c = (0, 0, 0)
    for b in data:
        c = guided.json_step(trans, c, b)
        if c is None:
            return False
    return c[0] == done


# ------------------------------------------------------------------ the corpus
_STR_CHARS = ["a", "Z", " ", "\"", "\\", "/", "\n", "\t", "\x00", "\x1f", "\x7f", "é", "€", "퟿", "", "😀",
              "\U0010ffff", "{", "}", "[", "]", ",", ":"]


def rand_str(rng):
    return "".join(rng.choice(_STR_CHARS) for _ in range(rng.randrange(0, 6)))


def rand_scalar(rng):
    kind = rng.randrange(7)
    if kind == 0:
        return rand_str(rng)
    if kind == 1:
        return rng.choice([0, -1, 7, 10, -120, 2 ** 63, -(10 ** 20)])
    if kind == 2:
        return rng.choice([0.0, -0.0, 1.5, -2.25e-7, 1e22, 3.0e-310, 1.7976931348623157e308, 0.1])
    if kind == 3:
        return True
    if kind == 4:
        return False
    if kind == 5:
        return None
    return [rand_scalar(rng) for _ in range(rng.randrange(0, 3))]


def rand_dict(rng, depth):
    """A dict whose deepest container sits at `depth` (dicts and lists both count)."""
    d = {rand_str(rng): rand_scalar(rng) for _ in range(rng.randrange(0, 3))}
    if depth > 1:
        if depth > 2 and rng.random() < 0.4:
            d[rand_str(rng)] = [rand_scalar(rng), rand_dict(rng, depth - 2)]
        else:
            d[rand_str(rng)] = rand_dict(rng, depth - 1)
    return d


def depth_of(v):
    if isinstance(v, dict):
        return 1 + max([depth_of(x) for x in v.values()] or [0])
    if isinstance(v, list):
        return 1 + max([depth_of(x) for x in v] or [0])
    return 0


@functools.lru_cache(maxsize=None)
def corpus():
    rng = random.Random(20)
    docs = []
    for i in range(400):
        v = rand_dict(rng, 1 + i % 32)
        if depth_of(v) > 32:      # a scalar list at the bottom adds a level
            continue
        for sep in (None, (",", ":")):
            for ascii_ in (True, False):
                docs.append(json.dumps(v, separators=sep, ensure_ascii=ascii_).encode("utf-8"))
    return tuple(docs)


def test_the_corpus_covers_every_depth_and_is_a_few_hundred_values():
    assert len(corpus()) >= 4 * 200
    seen = {oracle_max_depth(d) for d in corpus()}
    assert seen >= set(range(1, 33))


def oracle_max_depth(data):
    cfg, top = oracle.START, 0
    for b in data:
        cfg = oracle.feed(cfg, b)
        top = max(top, len(cfg[2]))
    return top


def test_completeness_every_dump_is_accepted():
    g, tb = single_byte_guide()
    for doc in corpus():
        assert oracle.accepts(doc), doc
        ids = [3 + b for b in doc]
        c = guided.walk_json(g, (0, 0, 0), ids, tb)
        assert c == (g.done, 0, 0), doc
        assert guided.walk_json(g, c, [2], tb)[0] == g.sink
        assert guided.walk(g, 0, ids + [2, 2])[0] == g.sink


def test_soundness_an_accepted_mutant_parses_to_a_dict():
    rng = random.Random(21)
    docs = [d for d in corpus() if len(d) <= 120]
    docs = rng.sample(docs, 24)
    alphabet = b'{}[]",: 0123456789-.eEtruefalsn\\u\x00\x1f\x7f\x80\xc3\xa9\xed\xa0\xf4\x90\xc0'
    accepted = 0
    for doc in docs:
        mutants = []
        for i in range(len(doc) + 1):
            if i < len(doc):
                mutants.append(doc[:i] + doc[i + 1:])
            for b in alphabet:
                if i < len(doc):
                    mutants.append(doc[:i] + bytes([b]) + doc[i + 1:])
                mutants.append(doc[:i] + bytes([b]) + doc[i:])
        for m in mutants:
            if oracle.accepts(m):
                accepted += 1
                assert isinstance(json.loads(m.decode("utf-8")), dict), m
                assert table_accepts(m), m
            else:
                assert not table_accepts(m), m
    assert accepted > 100          # the property was exercised


def test_depth_33_is_refused_and_32_is_not():
    for ok, bad in ((b'{"k":' * 32 + b"0" + b"}" * 32, b'{"k":' * 33 + b"0" + b"}" * 33),
                    (b'{"k":' + b"[" * 31 + b"]" * 31 + b"}", b'{"k":' + b"[" * 32 + b"]" * 32 + b"}")):
        assert oracle.accepts(ok) and table_accepts(ok)
        assert not oracle.accepts_prefix(bad) and not table_accepts(bad)
        assert isinstance(json.loads(ok), dict) and isinstance(json.loads(bad), dict)   # only the cap refuses it
    # the cap creates no dead end: at depth 32 every other value is still legal
    cfg = oracle.config_of(b'{"k":' * 32)
    nxt = oracle.legal_next(cfg)
    assert ord("{") not in nxt and ord("[") not in nxt
    assert {ord(c) for c in '"-0123456789tfn '} <= nxt


def agree_along(data: bytes):
    """Table and recogniser agree on the legal next bytes and on (depth, bits) after every prefix of data (up to the
    first byte that is not legal)."""
    trans, done = table()
    cfg, c = oracle.START, (0, 0, 0)
    for b in list(data) + [None]:
        legal_t = frozenset(x for x in range(256) if guided.json_step(trans, c, x) is not None)
        assert legal_t == oracle.legal_next(cfg), (data, c)
        assert (c[1], c[2]) == oracle.depth_bits(cfg)
        assert (c[0] == done) == (cfg[0] == "done")
        if b is None or b not in legal_t:
            return
        cfg, c = oracle.feed(cfg, b), guided.json_step(trans, c, b)


def test_agreement_on_all_prefixes_of_the_corpus_and_on_random_bytes():
    rng = random.Random(22)
    for doc in rng.sample(corpus(), 80):
        agree_along(doc)
    alphabet = b'{}[]",: 0123456789-.eEtruefalsn\\u\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80\xed\xa0'
    for _ in range(200):
        # a random walk that mostly follows legal bytes, so that it gets deep into the grammar
        cfg, out = oracle.START, bytearray()
        for _ in range(rng.randrange(1, 80)):
            nxt = sorted(oracle.legal_next(cfg))
            if not nxt:
                break
            cand = [b for b in alphabet if b in nxt] or nxt
            b = rng.choice(cand) if rng.random() < 0.95 else rng.randrange(256)
            out.append(b)
            cfg = oracle.feed(cfg, b)
            if cfg is None:
                break
        agree_along(bytes(out))


def test_the_table_is_what_the_issue_asks_for():
    trans, done = table()
    assert trans.dtype == np.int16 and trans.shape[1] == 256 and 80 <= trans.shape[0] <= guided.GUIDE_JSON_MAX_STATES
    assert (trans[done] == -1).all()                      # DONE reads nothing: only EOS follows
    live = trans[trans >= 0]
    assert ((live & 0xFF) < trans.shape[0]).all() and (live >> 10 == 0).all()
    pops = live[(live >> 8) == guided.JSON_ACT_POP] & 0xFF
    assert len(pops) and ((pops + 2) == done).all()        # after_o, after_a, DONE are consecutive
    # no state is a dead end at the cap: some transition does not push (DONE reads nothing, and the start state
    # exists at depth 0 only)
    for s in range(1, trans.shape[0]):
        if s != done:
            row = trans[s][trans[s] >= 0]
            assert ((row >> 8 == 0) | (row >> 8 == 3)).any(), s


# ------------------------------------------------------------------ the host kernel against the oracle
@functools.lru_cache(maxsize=None)
def case(vocab: int):
    return oracle.build_case(vocab)


def run_host(c, rows, stride, with_advance, with_lm, row_slot=None, cur=None, jstk=None, desc=None, trans=None,
             tok_off=None, advance=None):
    vocab = c["vocab"]
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = c["bits"][:rows]
    logits = torch.from_numpy(buf.view(np.int16)).view(torch.bfloat16)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy())
    cur_t = t(c["cur"] if cur is None else cur)
    jstk_t = t(c["jstk"] if jstk is None else jstk)
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32)
    lm = t(oracle.start_lm(rows).view(np.int32)) if with_lm else None
    if row_slot is None:
        row_slot = (oracle.ROW_SLOT_ADV if with_advance else oracle.ROW_SLOT_PLAIN)[:rows]
    adv = None
    if with_advance:
        adv = t(c["advance"][:rows] if advance is None else advance)
    reference.json_guide_rows(logits[:, :vocab], torch.tensor(row_slot, dtype=torch.int32),
                              t(c["desc"] if desc is None else desc), t(c["trans"] if trans is None else trans),
                              t(c["tok_off"] if tok_off is None else tok_off), t(c["tok_bytes"]), cur_t, jstk_t, err,
                              advance_ids=adv, lm_part=lm)
    bits = logits.contiguous().view(torch.int16).numpy().view(np.uint16)
    return bits, cur_t.numpy(), jstk_t.numpy(), err.numpy(), None if lm is None else lm.numpy().view(np.uint32)


@pytest.mark.parametrize("with_lm", [False, True], ids=["no_lm_part", "lm_part"])
@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
@pytest.mark.parametrize("pad", [0, 8], ids=["stride_eq_vocab", "stride_gt_vocab"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("vocab", [1024, 128256])
def test_host_rows_match_the_oracle_bit_for_bit(vocab, rows, pad, with_advance, with_lm):
    c = case(vocab)
    want, w_cur, w_jstk, w_err, w_lm = oracle.run_oracle(c, rows, vocab + pad, with_advance, with_lm)
    got, cur, jstk, err, lm = run_host(c, rows, vocab + pad, with_advance, with_lm)
    assert np.array_equal(got, want)
    assert np.array_equal(cur, w_cur) and np.array_equal(jstk, w_jstk) and np.array_equal(err, w_err)
    if with_lm:
        assert np.array_equal(lm, w_lm)
    if rows == 5:
        assert np.array_equal(got[1, :vocab], c["bits"][1])       # slot -1: byte-identical before and after
        assert int(w_err.sum()) == (oracle.ERR_NO_EDGE if with_advance else 0)


def test_host_every_start_configuration():
    c = case(1024)
    vocab, n = 1024, oracle.SLOTS
    rng = np.random.default_rng(3)
    bits = (rng.integers(-3, 5, size=(n, vocab)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    c2 = dict(c, bits=bits)
    slots = tuple(range(n))
    want, w_cur, w_jstk, w_err, w_lm = oracle.run_oracle(c2, n, vocab, False, True, row_slot=slots, bits=bits)
    got, cur, jstk, err, lm = run_host(c2, n, vocab, False, True, row_slot=slots)
    assert np.array_equal(got, want) and np.array_equal(lm, w_lm)
    assert np.array_equal(cur, c["cur"]) and np.array_equal(jstk, c["jstk"]) and not err.any()
    allowed = want[:, :vocab] != oracle.NINF_BF16
    tok = lambda name, t: bool(allowed[oracle.SLOT[name], t])
    bid = oracle.byte_id
    # the cap: every pushing token barred, '"' and digits allowed
    for name in ("depth32_value", "depth32_array_value"):
        assert not tok(name, bid("{")) and not tok(name, bid("[")) and not tok(name, oracle.ID_KEY)
        assert tok(name, bid('"')) and all(tok(name, bid(d)) for d in "0123456789")
    # depth 31: one push allowed, two barred
    assert tok("depth31_value", bid("[")) and tok("depth31_value", bid("{")) and tok("depth31_value", oracle.ID_KEY)
    assert not tok("depth31_value", oracle.ID_ARR2) and not tok("depth31_value", oracle.ID_ARR_OBJ)
    # depth 1: '}}' barred, '}' allowed
    assert tok("depth1_number", bid("}")) and not tok("depth1_number", oracle.ID_CLOSE2)
    # after 0 no digit may follow
    assert not any(tok("after_zero", bid(d)) for d in "0123456789") and tok("after_zero", bid("."))
    assert allowed[oracle.SLOT["sink"]].sum() == 1 and allowed[oracle.SLOT["done"]].sum() == 1
    assert tok("in_string_in_object_in_array", oracle.ID_POP_PUSH)
    assert all(allowed[i].any() for i in range(n))            # no configuration is a dead end


def test_host_every_kind_of_advance():
    c = case(1024)
    vocab = 1024
    kinds = oracle.ADVANCE_KINDS + (("in_key", vocab - 3, False, oracle.ERR_NO_EDGE),)   # an id beyond the table
    for name, tok, grows, want_err in kinds:
        s = oracle.SLOT[name]
        adv = np.array([tok], dtype=np.int64)
        want, w_cur, w_jstk, w_err, _ = oracle.run_oracle(c, 1, vocab, True, False, row_slot=(s,), advance=adv)
        assert int(w_err[s]) == want_err, (name, tok)
        if not grows and (name, tok) != ("done", oracle.EOS):     # a refused advance keeps the configuration
            assert (int(w_cur[s]), *w_jstk[s].tolist()) == (int(c["cur"][s]), *c["jstk"][s].tolist()), (name, tok)
        got, cur, jstk, err, _ = run_host(c, 1, vocab, True, False, row_slot=(s,), advance=adv)
        assert np.array_equal(got, want), (name, tok)
        assert np.array_equal(cur, w_cur) and np.array_equal(jstk, w_jstk) and np.array_equal(err, w_err), (name, tok)


def corruptions(c):
    """(name, overrides): every out-of-bounds descriptor, state, depth, stray stack bit, tok_off pair and table entry.
    Each is seen by the row of slot `in_key` (a string state: nearly every byte is read), without an advance unless
    the override carries one."""
    s = oracle.SLOT["in_key"]
    n = c["trans"].shape[0]
    state = int(c["cur"][s])

    def arr(key, idx, value):
        a = c[key].copy()
        a[idx] = value
        return {key: a}

    out = [
        ("n_states_zero", arr("desc", (s, 0), 0)),
        ("n_states_above_table", arr("desc", (s, 0), n + 1)),
        ("n_states_negative", arr("desc", (s, 0), -5)),
        ("done_negative", arr("desc", (s, 1), -1)),
        ("done_at_n_states", arr("desc", (s, 1), n)),
        ("eos_negative", arr("desc", (s, 2), -1)),
        ("eos_at_vocab", arr("desc", (s, 2), c["vocab"])),
        ("state_negative", arr("cur", s, -1)),
        ("state_above_sink", arr("cur", s, n + 1)),
        ("depth_negative", arr("jstk", (s, 0), -1)),
        ("depth_33", arr("jstk", (s, 0), 33)),
        ("stray_stack_bit", arr("jstk", (s, 1), 1 << 5)),
        ("stray_top_bit", arr("jstk", (s, 1), -(1 << 31))),
        ("tok_off_negative", arr("tok_off", 300, -4)),
        ("tok_off_descending", arr("tok_off", 301, int(c["tok_off"][300]) - 1)),
        ("tok_off_beyond_bytes", arr("tok_off", len(c["tok_off"]) - 1, len(c["tok_bytes"]) + 1)),
        ("entry_state_at_n", arr("trans", (state, ord("a")), n)),
        ("entry_below_minus_one", arr("trans", (state, ord("b")), -2)),
        ("entry_action_bits_above", arr("trans", (state, ord("c")), state | (1 << 10))),
        ("entry_pop_lands_beyond", arr("trans", (state, ord("d")), (n - 2) | (3 << 8))),
    ]
    # a pop at depth 0: the start state's '{' made a pop
    s0 = oracle.SLOT["start"]
    out.append(("pop_at_depth_0", dict(arr("trans", (0, ord("{")), 1 | (3 << 8)), row_slot=(s0,))))
    # a bad pair under the advanced token itself
    bad_off = c["tok_off"].copy()
    bad_off[oracle.ID_KEY_END + 1] = bad_off[oracle.ID_KEY_END] - 1
    out.append(("tok_off_of_the_advanced_token", {"tok_off": bad_off,
                                                  "advance": np.array([oracle.ID_KEY_END], dtype=np.int64)}))
    out.append(("entry_under_the_advance", dict(arr("trans", (state, ord("y")), 0x7FFF),
                                                advance=np.array([oracle.ID_KEY_END], dtype=np.int64))))
    return s, out


def test_host_every_out_of_bounds_value_is_a_table_error_and_nothing_is_touched():
    c = case(1024)
    vocab = 1024
    s, kinds = corruptions(c)
    for name, over in kinds:
        over = dict(over)
        row_slot = over.pop("row_slot", (s,))
        adv = over.pop("advance", None)
        cur0 = over.get("cur", c["cur"])
        jstk0 = over.get("jstk", c["jstk"])
        got, cur, jstk, err, lm = run_host(c, 1, vocab, adv is not None, True, row_slot=row_slot, advance=adv, **over)
        assert int(err[row_slot[0]]) == oracle.ERR_TABLE and int(err.sum()) == oracle.ERR_TABLE, name
        assert np.array_equal(got[0, :vocab], c["bits"][0]), name
        assert np.array_equal(cur, cur0) and np.array_equal(jstk, jstk0), name
        assert np.array_equal(lm, oracle.start_lm(1)), name
