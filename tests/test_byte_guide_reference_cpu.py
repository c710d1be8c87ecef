"""The host side of guided_regex over multi-byte vocabularies, and the oracle the kernel is judged by
(tests/byte_guide_reference.py) checked first: against the shipped CSR form state by state, against
reference.byte_guide_rows on the shared cases, and on corrupted tables (which never go to a GPU)."""

import functools
import types

import numpy as np
import pytest
import torch

from src import guided, ops
from src.guided import (Automaton, ByteGuide, byte_table, compile_byte_guide, compile_guide, compile_regex,
                        hf_token_bytes, walk)
from src.ops import reference
from tests import byte_guide_reference as oracle

EOS = 1
PATTERNS = (r"(ab|cd){4}x", r"\d{4}-\d{2}-\d{2}", r'\{"a": "[a-d ]{1,6}", "n": \d{1,3}\}', r"[a-d]+( [a-d]+){0,3}")


def sp(**kw):
    base = dict(allowed_token_ids=None, guided_choice=None, guided_regex=None, ignore_eos=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


@functools.lru_cache(maxsize=None)
def mixed_vocab():
    """4,104 entries: 0 None (pad), 1 EOS (no bytes), 2..257 the single bytes, then 2..16 bytes over an alphabet the
    patterns use."""
    rng = np.random.default_rng(4104)
    alphabet = b'abcdx 0123456789-{}":,n'
    table = [None, b""] + [bytes([b]) for b in range(256)]
    while len(table) < 4104:
        n = int(rng.integers(2, 17))
        table.append(bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=n)))
    return table


@functools.lru_cache(maxsize=None)
def lowercase_vocab():
    """4,104 entries: pad, EOS, the 256 single bytes, then 2..8 lowercase letters and spaces."""
    rng = np.random.default_rng(7)
    alphabet = b"abcdefghijklmnopqrstuvwxyz "
    table = [None, b""] + [bytes([b]) for b in range(256)]
    while len(table) < 4104:
        n = int(rng.integers(2, 9))
        table.append(bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=n)))
    return table


def device_tables(table):
    off = np.zeros(len(table) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(b or b"") for b in table])
    return off, np.frombuffer(b"".join(b or b"" for b in table) or b"\0", dtype=np.uint8).copy()


# ------------------------------------------------------------------ equivalence with the shipped form
@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_state_allows_what_the_csr_automaton_allows(pattern):
    table = mixed_vocab()
    vocab = len(table)
    auto = compile_regex(pattern, table, EOS, vocab)
    g = compile_byte_guide(pattern, table, EOS, vocab)
    n = g.n_states
    assert auto.n_states == n + 1                                   # the sink is state n, the numbering identical
    off, data = device_tables(table)
    tr, offl, datal = g.trans.tolist(), off.tolist(), data.tolist()
    for c in range(n + 1):
        want_tok, want_next = auto.edges(c)
        allowed = oracle.allowed_set(tr, g.accept, n, c, EOS, vocab, offl, datal, len(data))
        assert np.array_equal(np.nonzero(allowed)[0], want_tok), c
        nxt = [n if int(t) == EOS else oracle.token_walk(tr, n, c, int(t), offl, datal, len(data)) for t in want_tok]
        assert nxt == want_next.tolist(), c
        assert [walk(g, c, [int(t)]) for t in want_tok[:50]] == want_next[:50].tolist()


def test_a_pattern_over_the_edge_cap_compiles_to_a_byte_guide():
    table = lowercase_vocab()
    with pytest.raises(ValueError, match="more than 262144 edges"):
        compile_regex(r"[a-z ]{0,200}", table, EOS, len(table))      # what the CSR form still does with it
    g = compile_guide(sp(guided_regex=r"[a-z ]{0,200}"), len(table), EOS, table)
    assert isinstance(g, ByteGuide) and g.n_states == 201
    assert g.trans.dtype == np.int16 and g.trans.shape == (201, 256) and g.accept.dtype == np.uint8
    assert g.eos == EOS and g.key[0] == "regex"
    assert compile_guide(sp(guided_regex=r"[a-z ]{0,200}"), len(table), EOS, table) is g   # the LRU


# ------------------------------------------------------------------ host paths
def test_selection_rule_single_byte_tables_keep_the_csr_form():
    tb = byte_table(512)
    a = compile_guide(sp(guided_regex=r"\d{2}"), 512, 2, tb)
    assert isinstance(a, Automaton)
    b = compile_regex(r"\d{2}", tb, 2, 512)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("row_ptr", "edge_tok", "edge_next"))
    assert isinstance(compile_guide(sp(allowed_token_ids=[3, 4]), len(mixed_vocab()), EOS, mixed_vocab()), Automaton)
    assert isinstance(compile_guide(sp(guided_choice=[[5, 6]]), len(mixed_vocab()), EOS, mixed_vocab()), Automaton)
    assert isinstance(compile_guide(sp(guided_regex=r"\d{2}"), len(mixed_vocab()), EOS, mixed_vocab()), ByteGuide)


def test_a_byte_without_a_single_byte_token_is_refused():
    table = list(mixed_vocab())
    table[2 + ord("7")] = None
    with pytest.raises(ValueError, match="0x37"):
        compile_byte_guide(r"\d+", table, EOS, len(table))
    with pytest.raises(ValueError, match="0x37"):
        compile_guide(sp(guided_regex=r"\d+"), len(table), EOS, table)
    only_eos = list(mixed_vocab())
    only_eos[2 + ord("7")] = None
    only_eos[EOS] = b"7"                                            # EOS does not count as the byte's token
    with pytest.raises(ValueError, match="0x37"):
        compile_byte_guide(r"\d+", only_eos, EOS, len(only_eos))
    compile_byte_guide(r"[a-c]+", table, EOS, len(table))           # the pattern does not use the byte: fine


def test_host_walk_follows_the_device_rules():
    table = list(mixed_vocab()) + [b"1" * 33]
    g = compile_byte_guide(r"\d{2}(-\d{2})?", table, EOS, len(table))
    n = g.n_states
    d = lambda ch: 2 + ord(ch)
    two = table.index(b"12") if b"12" in table else None
    s = walk(g, 0, [d("1"), d("2")])
    assert g.accept[s]
    if two is not None:
        assert walk(g, 0, [two]) == s
    assert walk(g, s, [EOS]) == n and walk(g, n, [EOS, EOS]) == n   # the sink keeps itself
    assert walk(g, 0, [d("1"), d("2"), d("-"), d("3"), d("4"), EOS]) == n
    for state, toks in ((0, [EOS]),             # EOS where the state does not accept
                        (0, [d("x")]),          # a dead transition
                        (0, [0]),               # a token without bytes
                        (n, [d("1")]),          # anything but EOS in the sink
                        (0, [len(table) - 1]),  # over the length cap
                        (0, [len(table) + 5])):
        with pytest.raises(ValueError):
            walk(g, state, toks)


# ------------------------------------------------------------------ reference.byte_guide_rows against the oracle
def run_reference(case, rows, stride, with_advance, with_lm, cur=None, slot=None, advance=None, tables=None):
    vocab = case["vocab"]
    t = tables or case
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = case["bits"][:rows]
    logits = torch.from_numpy(buf.view(np.int16)).view(torch.bfloat16)
    cur = torch.from_numpy((case["cur_adv" if with_advance else "cur_plain"] if cur is None else cur).copy())
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32)
    lm = torch.from_numpy(oracle.start_lm(rows).view(np.int32).copy()) if with_lm else None
    adv = case["advance"][:rows] if advance is None else advance
    ops.byte_guide(logits[:, :vocab], torch.tensor(oracle.ROW_SLOT[:rows] if slot is None else slot, dtype=torch.int32),
                   *(torch.from_numpy(t[k].copy()) for k in ("desc", "trans", "accept", "tok_off", "tok_bytes")),
                   cur, err, advance_ids=torch.from_numpy(adv.copy()) if with_advance else None, lm_part=lm)
    bits = logits.contiguous().view(torch.int16).numpy().view(np.uint16)
    return bits, cur.numpy(), err.numpy(), None if lm is None else lm.numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(vocab):
    return oracle.build_case(vocab)


@pytest.mark.parametrize("with_lm", [False, True], ids=["no_lm_part", "lm_part"])
@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
@pytest.mark.parametrize("vocab,pad", [(1024, 0), (8200, 8)])
def test_cpu_path_matches_the_oracle_bit_for_bit(vocab, pad, with_advance, with_lm):
    c = case(vocab)
    want, w_cur, w_err, w_lm = oracle.run_oracle(c, 5, vocab + pad, with_advance, with_lm)
    got, cur, err, lm = run_reference(c, 5, vocab + pad, with_advance, with_lm)
    assert np.array_equal(got, want) and np.array_equal(cur, w_cur) and np.array_equal(err, w_err)
    if with_lm:
        assert np.array_equal(lm, w_lm)
    # what the case promises to hold
    assert np.array_equal(got[1], np.concatenate([c["bits"][1], np.full(pad, 0x447A, np.uint16)]))   # slot -1
    allowed = got[:, :vocab] != oracle.NINF_BF16
    n_tok = vocab - 40
    lens = np.diff(c["tok_off"])
    assert not allowed[[0, 2, 3, 4], n_tok:].any()                  # beyond the table
    assert np.array_equal(np.nonzero(allowed[2])[0], [EOS])         # the sink
    full = (lens >= 1) & (lens <= oracle.MAX_TOKEN_BYTES)
    full[EOS] = True                                                # A1 accepts
    full[oracle.byte_id("a")] = False                               # allowed, but the case's own logit there is -inf
    assert np.array_equal(allowed[0, :n_tok], full)                 # the full vocabulary: all but empty and over-cap
    assert allowed[0, oracle.ID_CAP] and not allowed[0, oracle.ID_OVER] and not allowed[0, oracle.ID_EMPTY]
    if with_advance:
        assert w_cur[[3, 0, 6, 2]].tolist() == [1, 6, 26, 3] and w_err.tolist() == [0, 0, oracle.ERR_NO_EDGE, 0, 0, 0, 0]
    else:
        assert np.array_equal(np.nonzero(allowed[4])[0], [EOS])     # A2: nothing but EOS
        assert not w_err.any()


def test_every_kind_of_advance():
    vocab = 1024
    c = case(vocab)
    kinds = oracle.ADVANCE_KINDS + ((0, vocab - 3, 0, oracle.ERR_NO_EDGE),)    # an id beyond the table
    for start, tok, want_state, want_err in kinds:
        cur = c["cur_plain"].copy()
        cur[3] = start
        adv = np.array([tok], dtype=np.int64)
        got, g_cur, g_err, _ = run_reference(c, 1, vocab, True, False, cur=cur, advance=adv)
        buf = c["bits"][:1].copy()
        o_cur, o_err = cur.copy(), np.zeros(oracle.SLOTS, dtype=np.int32)
        oracle.byte_guide(buf, oracle.ROW_SLOT[:1], c["desc"], c["trans"], c["accept"], c["tok_off"], c["tok_bytes"],
                          o_cur, o_err, vocab, advance=adv)
        assert (int(o_cur[3]), int(o_err[3])) == (want_state, want_err), (start, tok)
        assert np.array_equal(got, buf) and np.array_equal(g_cur, o_cur) and np.array_equal(g_err, o_err), (start, tok)


def corrupt(c, what):
    t = {k: c[k].copy() for k in ("desc", "trans", "accept", "tok_off", "tok_bytes")}
    if what == "offset":
        t["tok_off"][500] = len(t["tok_bytes"]) + 7                 # past the bytes, and descending behind it
    elif what == "negative_offset":
        t["tok_off"][0] = -4
    elif what == "trans":
        t["trans"][oracle.BASE_A + 1, ord("b")] = 6                 # >= n_states, in the state that reads every byte
    elif what == "trans_low":
        t["trans"][oracle.BASE_A + 1, ord("c")] = -2
    elif what == "descriptor":
        t["desc"][:, 0] = len(t["accept"]) - 3                      # state_base + n_states past the arena
    elif what == "eos":
        t["desc"][:, 2] = c["vocab"]
    return t


@pytest.mark.parametrize("what", ["offset", "negative_offset", "trans", "trans_low", "descriptor", "eos"])
@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
def test_corrupted_tables_set_the_error_and_leave_everything_else(what, with_advance):
    vocab = 1024
    c = case(vocab)
    t = corrupt(c, what)
    cur = c["cur_plain"].copy()
    cur[3] = 1                                                      # A1 reads every byte: it meets each corruption
    adv = np.array([oracle.byte_id("b")], dtype=np.int64)
    got, g_cur, g_err, g_lm = run_reference(c, 1, vocab, with_advance, True, cur=cur, advance=adv, tables=t)
    buf = c["bits"][:1].copy()
    o_cur, o_err, o_lm = cur.copy(), np.zeros(oracle.SLOTS, dtype=np.int32), oracle.start_lm(1)
    oracle.byte_guide(buf, oracle.ROW_SLOT[:1], t["desc"], t["trans"], t["accept"], t["tok_off"], t["tok_bytes"],
                      o_cur, o_err, vocab, advance=adv if with_advance else None, lm=o_lm)
    assert int(o_err[3]) == oracle.ERR_TABLE
    assert np.array_equal(buf, c["bits"][:1]) and np.array_equal(o_cur, cur) and np.array_equal(o_lm, oracle.start_lm(1))
    assert np.array_equal(got, buf) and np.array_equal(g_cur, o_cur) and np.array_equal(g_err, o_err)
    assert np.array_equal(g_lm, o_lm)


def test_constants_are_mirrored():
    assert ops.GUIDE_MAX_TOKEN_BYTES == guided.GUIDE_MAX_TOKEN_BYTES == oracle.MAX_TOKEN_BYTES >= 32
    assert ops.GUIDE_BYTE_LDS_STATES == oracle.LDS_STATES
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "csrc", "kernels", "launchers.h")).read()
    for name in ("GUIDE_MAX_TOKEN_BYTES", "GUIDE_BYTE_STATE_ARENA", "GUIDE_BYTE_LDS_STATES", "GUIDE_TOK_TABLE_MAX",
                 "GUIDE_TOK_BYTES_MAX"):
        m = re.search(r"constexpr int %s = ([^;]+);" % name, hdr)
        assert m and eval(m.group(1)) == getattr(ops, name), name
    assert oracle.guide_a()[0].shape[0] <= ops.GUIDE_BYTE_LDS_STATES < oracle.N_B   # a guide on each side


# ------------------------------------------------------------------ hf_token_bytes
TEXTS = ("plain ASCII text, 123!", "café au lait", "a ☃ in the snow", "  two spaces\nnewline\ttab")


def bytelevel_tokenizer():
    import tokenizers
    import transformers
    from tokenizers import decoders, models, pre_tokenizers, trainers

    tok = tokenizers.Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=400, special_tokens=["<|endoftext|>"], show_progress=False,
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet())
    corpus = ["the quick brown fox jumps over the lazy dog", "hello world hello there", "café ☃ 12345",
              '{"name": "value", "age": 42}'] * 8
    tok.train_from_iterator(corpus, trainer)
    return transformers.PreTrainedTokenizerFast(tokenizer_object=tok, eos_token="<|endoftext|>")


def byte_fallback_tokenizer():
    import tokenizers
    import transformers
    from tokenizers import decoders, models, normalizers

    pieces = ["<unk>", "<s>", "</s>"] + ["<0x%02X>" % b for b in range(256)]
    pieces += ["▁"] + list("abcdefghijklmnopqrstuvwxyzACIS0123456789,.!") + ["▁t", "he", "▁the", "in", "é"]
    vocab = {p: i for i, p in enumerate(pieces)}
    merges = [("▁", "t"), ("h", "e"), ("▁t", "he"), ("i", "n")]
    tok = tokenizers.Tokenizer(models.BPE(vocab=vocab, merges=merges, unk_token="<unk>", byte_fallback=True))
    tok.normalizer = normalizers.Replace(" ", "▁")
    tok.decoder = decoders.Sequence([decoders.Replace("▁", " "), decoders.ByteFallback(), decoders.Fuse()])
    return transformers.PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="<unk>", bos_token="<s>",
                                                eos_token="</s>")


@pytest.mark.parametrize("make", [bytelevel_tokenizer, byte_fallback_tokenizer], ids=["bytelevel_bpe", "byte_fallback"])
def test_hf_token_bytes_spells_what_the_tokenizer_encodes(make):
    tok = make()
    vocab = len(tok) + 13                                           # a model vocabulary padded beyond the tokenizer
    table = hf_token_bytes(tok, vocab)
    assert table is not None and len(table) == vocab
    assert all(b is None for b in table[len(tok):])
    assert table[tok.eos_token_id] is None                          # special tokens have no bytes
    for text in TEXTS:
        ids = tok.encode(text, add_special_tokens=False)
        assert b"".join(table[i] for i in ids) == text.encode()
    singles = {b for b in table if b is not None and len(b) == 1}
    assert len(singles) == 256                                      # every byte has a single-byte token
    g = compile_guide(sp(guided_regex=r"[a-z]+ \d{1,3}"), vocab, tok.eos_token_id, table)
    assert isinstance(g, ByteGuide)


def test_hf_token_bytes_refuses_what_it_does_not_recognise():
    class Opaque:
        def get_vocab(self):
            return {"一丁": 0, "foo": 1}                    # neither alphabet nor byte pieces

        def encode(self, text, add_special_tokens=False):
            return [0]

    assert hf_token_bytes(Opaque(), 16) is None
    assert hf_token_bytes(object(), 16) is None

    class Lying(Opaque):                                            # the layout fits, the round trip does not
        def get_vocab(self):
            return {"a": 0, "b": 1}

    assert hf_token_bytes(Lying(), 16) is None
