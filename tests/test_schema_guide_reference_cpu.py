"""reference.schema_guide_rows (the host fallback of ops.schema_guide, and the op's written contract) against the
independent oracle of tests/schema_guide_reference.py, bit for bit: the shared kernel case, every start configuration
with an advance chosen for it, and the corrupted tables. guided.walk_schema, which rebuilds a slot after a
preemption, is held to the same simulator."""

import random

import numpy as np
import pytest
import torch

from src import guided, ops

from tests import schema_guide_reference as oracle

ADV_TOKENS = {0: b"{", 1: b"}", 2: b"n", 3: b"}", 4: b"[[[[", 5: b"[", 6: b"]]],[[[", 7: None, 8: b"}", 9: b"]",
              10: b"{", 11: b"\x98", oracle.SLOT_SINK: None, oracle.SLOT_ACCEPT_DEEP: None}   # None: EOS


def host(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy())


def launch(vocab, rows, stride, with_advance, with_lm, row_slot=None, advance=None, **over):
    c = oracle.build_case(vocab)
    buf = np.full((rows, stride), 0x447A, dtype=np.uint16)
    buf[:, :vocab] = c["bits"][:rows]
    logits = torch.from_numpy(buf.view(np.int16)).view(torch.bfloat16)
    get = lambda k: host(over.get(k, c[k]))
    cur, sdep, sstk = get("cur"), get("sdep"), get("sstk")
    err = torch.zeros(oracle.SLOTS, dtype=torch.int32)
    lm = host(oracle.start_lm(rows).view(np.int32)) if with_lm else None
    if row_slot is None:
        row_slot = (oracle.ROW_SLOT_ADV if with_advance else oracle.ROW_SLOT_PLAIN)[:rows]
    adv = None
    if with_advance:
        adv = host(c["advance"][:rows] if advance is None else advance)
    ops.schema_guide(logits[:, :vocab], torch.tensor(row_slot, dtype=torch.int32), get("desc"), get("trans"),
                     get("accept"), get("tok_off"), get("tok_bytes"), cur, sdep, sstk, err, advance_ids=adv, lm_part=lm)
    return logits, cur, sdep, sstk, err, lm


def check(got, want, rows, with_lm):
    logits, cur, sdep, sstk, err, lm = got
    w_bits, w_cur, w_sdep, w_sstk, w_err, w_lm = want
    bits = logits.contiguous().view(torch.int16).numpy().view(np.uint16)
    for r in range(rows):
        bad = np.nonzero(bits[r] != w_bits[r])[0]
        assert bad.size == 0, (r, bad[:5].tolist())
    assert np.array_equal(cur.numpy(), w_cur) and oracle.live_equal(sdep.numpy(), sstk.numpy(), w_sdep, w_sstk)
    assert np.array_equal(err.numpy(), w_err)
    if with_lm:
        assert np.array_equal(lm.numpy().view(np.uint32), w_lm)
    return bits


@pytest.mark.parametrize("with_lm", [False, True], ids=["no_lm_part", "lm_part"])
@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
@pytest.mark.parametrize("vocab,rows,pad", [(1024, 1, 0), (1024, 5, 8), (128256, 5, 0)])
def test_the_shared_case_matches_the_oracle(vocab, rows, pad, with_advance, with_lm):
    c = oracle.build_case(vocab)
    want = oracle.run_oracle(c, rows, vocab + pad, with_advance, with_lm)
    bits = check(launch(vocab, rows, vocab + pad, with_advance, with_lm), want, rows, with_lm)
    if rows == 5:
        assert np.array_equal(bits[1, :vocab], c["bits"][1])    # slot -1
        assert int(want[4].sum()) == (ops.GUIDE_ERR_NO_EDGE if with_advance else 0)
        assert bits[4, vocab:].tolist() == [0x447A] * pad       # nothing beyond the vocabulary


def test_the_case_holds_what_the_contract_names():
    c = oracle.build_case(1024)
    toks = c["tokens"]
    assert len(toks) < 1024 and b"" in toks[3:] and any(len(t) == 40 for t in toks)
    t0, a0 = c["tables"][0]
    assert len(t0) < len(c["tables"][1][0]) <= oracle.ARENA - oracle.BASES[1]       # two guides of different sizes
    deep = oracle.text_config(t0, len(t0), oracle.DEEP31)
    assert len(deep[1]) == 31
    assert oracle.feed(t0, len(t0), *deep, b"[") not in (oracle.DEAD, oracle.BAD)
    assert oracle.feed(t0, len(t0), *deep, b"[[") == oracle.DEAD                   # the depth cap
    one = oracle.text_config(t0, len(t0), '{"k":')
    assert oracle.feed(t0, len(t0), *one, b"[[[[") not in (oracle.DEAD, oracle.BAD)
    assert oracle.feed(t0, len(t0), *one, b"[[[[[") == oracle.DEAD                 # five live pushes
    six = oracle.text_config(t0, len(t0), '{"k":[[[[[[1')
    state, stack = oracle.feed(t0, len(t0), *six, b"]]]],[[[[")                   # pops below its start, pushes back
    assert len(stack) == 7 and oracle.feed(t0, len(t0), *six, b"]]]]],[[[[[") == oracle.DEAD
    assert b"]]]],[[[[" in toks and b"]]]]],[[[[[" in toks
    assert c["sdep"].tolist()[:12] == [0, 1, 3, 1, 31, 32, 32, 0, 1, 1, 1, 1]
    assert a0[c["cur"][7]] and a0[c["cur"][oracle.SLOT_ACCEPT_DEEP]] and c["sdep"][oracle.SLOT_ACCEPT_DEEP] == 1
    assert c["cur"][oracle.SLOT_SINK] == len(t0)


@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
def test_every_start_configuration(with_advance):
    vocab = 1024
    c = oracle.build_case(vocab)
    eos = c["eos"]
    slots, flags = oracle.ALL_SLOTS, 0
    for at in range(0, len(slots), 5):
        rs = slots[at:at + 5]
        adv = np.array([eos if ADV_TOKENS[s] is None else c["tid"][ADV_TOKENS[s]] for s in rs], dtype=np.int64)
        want = oracle.run_oracle(c, len(rs), vocab, with_advance, True, row_slot=rs, advance=adv)
        check(launch(vocab, len(rs), vocab, with_advance, True, row_slot=rs, advance=adv), want, len(rs), True)
        flags += int((want[4] != 0).sum())
    # '[[[[' at depth 31, '[' at depth 32 and EOS at depth 1 have no edge; everything else advances
    assert flags == (3 if with_advance else 0)
    w = oracle.run_oracle(c, 2, vocab, False, False, row_slot=(oracle.SLOT_ACCEPT_DEEP, 7))[0]
    assert w[0, eos] == 0xFF80 and w[1, eos] == c["bits"][1, eos]   # EOS barred at depth 1, allowed at depth 0


@pytest.mark.parametrize("with_advance", [False, True], ids=["no_advance", "advance"])
def test_corrupted_tables_report_a_table_error_and_write_nothing(with_advance):
    vocab = 1024
    c = oracle.build_case(vocab)
    tid = c["tid"]
    cases = oracle.corruptions(c)
    assert len(cases) >= 16
    for name, over, slots in cases:
        adv = np.array([tid[b'"'] if s else tid[b"{"] for s in slots], dtype=np.int64)
        bad = dict(c, **over)
        want = oracle.run_oracle(bad, len(slots), vocab, with_advance, True, row_slot=slots, advance=adv)
        assert all(want[4][s] == ops.GUIDE_ERR_TABLE for s in slots), name
        got = launch(vocab, len(slots), vocab, with_advance, True, row_slot=slots, advance=adv, **over)
        bits = check(got, want, len(slots), True)
        assert np.array_equal(bits[:, :vocab], c["bits"][:len(slots)]), name
        assert np.array_equal(got[3].numpy(), bad["sstk"]) and np.array_equal(got[1].numpy(), bad["cur"]), name


def test_walk_schema_follows_the_simulator():
    c = oracle.build_case(1024)
    toks = c["tokens"]
    rng = random.Random(4)
    for g, schema in enumerate((oracle.SCHEMA_ANY, oracle.SCHEMA_TREE)):
        t, a = c["tables"][g]
        guide = guided.SchemaGuide(t, a, c["eos"], ("test", 0))
        trie = oracle.make_trie(toks, len(toks))
        for _ in range(20):
            state, stack, ids = 0, [], []
            for _ in range(40):
                ok, bad = oracle.allowed_tokens(t, len(t), state, stack, trie)
                assert not bad
                if not ok:                                 # no dead end: only the finished document has no token
                    assert a[state] and not stack
                    break
                tok = rng.choice(sorted(ok))
                ids.append(tok)
                state, stack = oracle.feed(t, len(t), state, stack, toks[tok])
                assert guided.walk_schema(guide, (0, 0, ()), ids, toks) == (state, len(stack), tuple(stack))
        with pytest.raises(ValueError):
            guided.walk_schema(guide, (0, 0, ()), [c["tid"][b"[[[[["]], toks)
        with pytest.raises(ValueError):
            guided.walk_schema(guide, (0, 0, ()), [c["eos"]], toks)
