"""The JSON Schema compiler of guided_json (src/guided_schema.py) on a fixed list of schemas: seeded random byte
walks to the end parse and validate, hand-written documents are accepted and near misses rejected, every reachable
configuration can be completed, {"type": "object"} is JSON mode's language byte for byte, every refusal names its
keyword or case, and a schema with its keys reordered hits the compile cache. The walks use the simulator and the
validator of tests/schema_guide_reference.py, not the compiler's own helpers."""

import json
import random

import numpy as np
import pytest

from src import guided
from src.preproc import SamplingParams

from tests import schema_guide_reference as oracle

EOS = 2
TABLE = guided.byte_table(1024)

LIST = {"type": "object", "properties": {"v": {"type": "number"}, "next": {"anyOf": [{"$ref": "#"}, {"type": "null"}]}},
        "required": ["v", "next"]}
TREE = {"$defs": {"node": {"type": "object",
                           "properties": {"name": {"type": "string", "maxLength": 3},
                                          "kids": {"type": "array", "items": {"$ref": "#/$defs/node"}, "maxItems": 2}},
                           "required": ["name"]}},
        "$ref": "#/$defs/node"}
# (name, schema, valid documents in canonical form, near misses)
SCHEMAS = [
    ("flat", {"type": "object", "title": "t",
              "properties": {"a": {"type": "integer"}, "b": {"type": "string"}, "c": {"type": "boolean"},
                             "d": {"type": "null"}},
              "required": ["b"], "additionalProperties": False},
     ['{"b":""}', '{"a":-7,"b":"x"}', '{"a":0, "b": "\\u00e9\\n", "c":true,"d":null}', '{"b":"é☃","d":null}'],
     ['{}', '{"a":1}', '{"b":"x","a":1}', '{"b":"x","e":1}', '{"a":1.5,"b":"x"}', '{"a":01,"b":"x"}', '{"b":"x",}',
      '{"b":"x"}}', '{ "b":"x"}', '{"b":"x","b":"y"}']),
    ("all_optional", {"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "integer"},
                                                       "c": {"type": "integer"}}},
     ['{}', '{"a":1}', '{"b":1}', '{"c":1}', '{"a":1,"c":3}', '{"a":1,"b":2,"c":3}', '{"b":2, "c":3}'],
     ['{,"a":1}', '{"a":1,}', '{"c":3,"a":1}', '{"a":1 ,"b":2}', '{"a":1,,"c":3}']),
    ("nested", {"type": "object",
                "properties": {"rows": {"type": "array", "minItems": 1, "maxItems": 3,
                                        "items": {"type": "object",
                                                  "properties": {"id": {"type": "integer"},
                                                                 "tags": {"type": "array", "items": {"type": "string"}}},
                                                  "required": ["id"]}}},
                "required": ["rows"]},
     ['{"rows":[{"id":1}]}', '{"rows":[{"id":1,"tags":[]},{"id":2,"tags":["a", "b"]},{"id":3}]}'],
     ['{"rows":[]}', '{"rows":[{"id":1},{"id":2},{"id":3},{"id":4}]}', '{"rows":[{"tags":[]}]}', '{"rows":[{"id":1},]}',
      '{"rows":[{"id":1,"tags":[1]}]}']),
    ("enum_const", {"type": "object",
                    "properties": {"k": {"enum": ["red", "green", 3, None, {"a": [1, 2]}, "é\n"]}, "v": {"const": 1.5}},
                    "required": ["k", "v"]},
     ['{"k":"red","v":1.5}', '{"k":3,"v":1.5}', '{"k":null,"v":1.5}', '{"k":{"a":[1,2]},"v":1.5}', '{"k":"é\\n","v":1.5}'],
     ['{"k":"blue","v":1.5}', '{"k":"red","v":1.50}', '{"k":{"a":[1, 2]},"v":1.5}', '{"k":"re","v":1.5}',
      '{"k":4,"v":1.5}']),
    ("bounds", {"type": "object",
                "properties": {"s": {"type": "string", "minLength": 2, "maxLength": 4},
                               "p": {"type": "string", "pattern": "^[a-z]+-\\d{2}$"},
                               "m": {"type": "string", "minLength": 1}},
                "required": ["s"]},
     ['{"s":"ab"}', '{"s":"abcd"}', '{"s":"é\\n☃𝄞"}', '{"s":"ab","p":"x-12"}', '{"s":"ab","m":"x"}',
      '{"s":"ab","m":"' + "y" * 50 + '"}'],
     ['{"s":"a"}', '{"s":"abcde"}', '{"s":"\\u00e9b"}', '{"s":"ab","p":"x-1"}', '{"s":"ab","p":"X-12"}',
      '{"s":"ab","p":"x-123"}', '{"s":"ab","m":""}']),
    ("nullable", {"type": "object", "properties": {"x": {"anyOf": [{"type": "integer"}, {"type": "null"}]},
                                                   "y": {"type": ["string", "null"]}},
                  "required": ["x", "y"]},
     ['{"x":null,"y":null}', '{"x":5,"y":"s"}'], ['{"x":"5","y":null}', '{"x":null,"y":5}', '{"x":nul,"y":null}']),
    ("list", LIST,
     ['{"v":1,"next":null}', '{"v":1e3,"next":{"v":-0.5,"next":{"v":2,"next":null}}}'],
     ['{"v":1}', '{"v":1,"next":{}}', '{"next":null,"v":1}', '{"v":1,"next":{"v":2,"next":null}']),
    ("tree", TREE,
     ['{"name":"a"}', '{"name":"abc","kids":[]}', '{"name":"a","kids":[{"name":"b","kids":[{"name":"c"}]},{"name":""}]}'],
     ['{"name":"abcd"}', '{"kids":[]}', '{"name":"a","kids":[{"name":"b"},{"name":"c"},{"name":"d"}]}',
      '{"name":"a","kids":[{}]}']),
    ("metadata", {"type": "object", "properties": {"id": {"type": "integer"}, "metadata": {"type": "object"},
                                                   "extra": {}},
                  "required": ["id", "metadata"]},
     ['{"id":1,"metadata":{}}', '{"id":1,"metadata":{"a":[1,{"b":null}],"c":"d"},"extra":[[], {}, 1.5e-3, "x"]}',
      '{"id":1,"metadata":{"k": {"k": {}}},"extra":null}'],
     ['{"id":1}', '{"id":1,"metadata":[]}', '{"id":1,"metadata":{"a"}}', '{"id":1,"metadata":{},"extra":}',
      '{"id":1,"metadata":{} }']),
    ("anything", {}, ['{}', '[]', '1', '"s"', 'null', '[1, {"a":[true]}]', '-0.5e+7'],
     ['', '[', '01', '[1,]', '{"a"}', ' 1', 'nul']),
    ("top_array", {"type": "array", "items": {"type": ["integer", "boolean"]}, "minItems": 2},
     ['[1,2]', '[true, 0,false]'], ['[1]', '[]', '[1,"2"]', '[1,2', '[1,2]]']),
    ("all_of_ref", {"definitions": {"n": {"type": "integer"}},
                    "allOf": [{"type": "object", "properties": {"n": {"$ref": "#/definitions/n"}}, "required": ["n"]}]},
     ['{"n":12}'], ['{}', '{"n":1.0}']),
]
IDS = [s[0] for s in SCHEMAS]


def pda(schema):
    return guided.schema_to_pda(schema)


def finish_costs(trans, accept):
    """(pop[s], acc[s]): the fewest bytes from state s to a pop (inclusive), and to an accepting state with nothing
    on the stack; a push costs its byte, the frame's way to its pop and then the return state's own cost."""
    n = len(trans)
    inf = 10 ** 6
    live = trans >= 0
    act = np.where(live, trans >> 28, -1)
    nxt, ret = trans & 0x3FFF, (trans >> 14) & 0x3FFF
    pop = np.full(n, inf, dtype=np.int64)
    acc = np.where(accept != 0, 0, inf).astype(np.int64)
    for _ in range(4 * n + 8):
        via = np.full(trans.shape, inf, dtype=np.int64)
        via[act == 2] = 1
        via[act == 0] = 1 + pop[nxt[act == 0]]
        via[act == 1] = 1 + pop[nxt[act == 1]] + pop[ret[act == 1]]
        new_pop = np.minimum(via.min(axis=1), inf)
        via = np.full(trans.shape, inf, dtype=np.int64)
        via[act == 0] = 1 + acc[nxt[act == 0]]
        via[act == 1] = 1 + pop[nxt[act == 1]] + acc[ret[act == 1]]
        new_acc = np.minimum(np.minimum(via.min(axis=1), acc), inf)
        if np.array_equal(new_pop, pop) and np.array_equal(new_acc, acc):
            break
        pop, acc = new_pop, new_acc
    return pop, acc


def legal_groups(trans, state, depth):
    """The legal bytes of a configuration, grouped by table entry (a string's ninety plain bytes are one choice)."""
    groups = {}
    for b in np.nonzero(trans[state] >= 0)[0]:
        v = int(trans[state, b])
        if v >> 28 == 1 and depth >= oracle.DEPTH_CAP:
            continue
        groups.setdefault(v, []).append(int(b))
    return groups


def random_document(trans, accept, costs, rng, wander):
    """A seeded walk: ``wander`` random legal bytes, then the cheapest way to the end."""
    pop, acc = costs
    ns = len(trans)
    state, stack, out = 0, [], bytearray()

    def remaining(s, stk):
        return (acc[s] if not stk else pop[s] + sum(pop[r] for r in stk[1:]) + acc[stk[0]])

    for step in range(wander + 4096):
        groups = legal_groups(trans, state, len(stack))
        if accept[state] and not stack and (step >= wander or not groups):
            return bytes(out)
        assert groups, "a configuration without a legal byte"
        if step < wander:
            b = rng.choice(groups[rng.choice(sorted(groups))])
        else:
            best = None
            for v, bs in groups.items():
                r = oracle.byte_step(trans, ns, state, stack, 0, bs[0])
                cost = remaining(r[0], r[1])
                if best is None or cost < best[0]:
                    best = (cost, bs[0])
            b = best[1]
        state, stack, _ = oracle.byte_step(trans, ns, state, stack, 0, b)
        out.append(b)
    raise AssertionError("the walk did not end")


@pytest.mark.parametrize("name,schema,valid,invalid", SCHEMAS, ids=IDS)
def test_random_walks_to_the_end_parse_and_validate(name, schema, valid, invalid):
    trans, accept = pda(schema)
    costs = finish_costs(trans, accept)
    rng = random.Random(name)
    for i in range(40):
        text = random_document(trans, accept, costs, rng, wander=rng.choice((0, 5, 20, 60, 150)))
        doc = json.loads(text.decode("utf-8"))              # well-formed UTF-8, and it parses
        assert oracle.validate(doc, schema), (name, text)
        assert oracle.accepts(trans, accept, text)


@pytest.mark.parametrize("name,schema,valid,invalid", SCHEMAS, ids=IDS)
def test_documents_are_accepted_and_near_misses_rejected(name, schema, valid, invalid):
    trans, accept = pda(schema)
    for text in valid:
        assert oracle.validate(json.loads(text), schema), (name, text)      # the list itself is right
        assert oracle.accepts(trans, accept, text), (name, text)
    for text in invalid:
        assert not oracle.accepts(trans, accept, text), (name, text)


@pytest.mark.parametrize("name,schema,valid,invalid", SCHEMAS, ids=IDS)
def test_every_reachable_configuration_can_be_completed(name, schema, valid, invalid):
    trans, accept = pda(schema)
    assert trans.dtype == np.int32 and trans.shape[1] == 256 and len(trans) <= guided.GUIDE_MAX_STATES
    assert accept.dtype == np.uint8 and accept.shape == (len(trans),)
    live = trans[trans >= 0]
    assert (live >> 30 == 0).all() and (live >> 28 <= 2).all() and ((live & 0x3FFF) < len(trans)).all()
    assert (((live >> 14) & 0x3FFF) < len(trans)).all()
    pops = live[live >> 28 == 2]
    assert (pops == 2 << 28).all()                                       # a pop's fields are written as 0
    assert ((live[live >> 28 == 0] >> 14) == 0).all()
    guided.schema_check_closable(trans, accept)
    reach, can = guided.schema_depth_sets(trans), guided.schema_closable_sets(trans, accept)
    act = np.where(trans >= 0, trans >> 28, -1)
    for d in range(oracle.DEPTH_CAP + 1):
        assert not (reach[d] & ~can[d]).any(), d
    assert not (reach[0] & (act == 2).any(axis=1)).any()                 # no pop at depth 0
    at_cap = np.nonzero(reach[oracle.DEPTH_CAP])[0]
    assert all(((act[s] == 0) | (act[s] == 2)).any() for s in at_cap)    # at depth 32 a byte that does not push
    if name in ("list", "tree", "metadata", "anything"):
        assert len(at_cap)                                               # these do get there
    # and the simulator agrees on a walk that nests to the cap: it can always go one byte further
    if name == "anything":
        state, stack = oracle.text_config(trans, len(trans), "[" * 32)
        assert len(stack) == 32 and oracle.feed(trans, len(trans), state, stack, b"[") == oracle.DEAD
        assert oracle.feed(trans, len(trans), state, stack, b"1") != oracle.DEAD


def json_legal(jt, cfg):
    s, d, _ = cfg
    row = jt[s].astype(np.int64)
    push = (row >> 8 == guided.JSON_ACT_PUSH_OBJECT) | (row >> 8 == guided.JSON_ACT_PUSH_ARRAY)
    return (row >= 0) & ~(push & (d >= guided.GUIDE_JSON_MAX_DEPTH))


def schema_legal(st, state, depth):
    row = st[state].astype(np.int64)
    return (row >= 0) & ~((row >> 28 == 1) & (depth >= oracle.DEPTH_CAP))


def test_type_object_is_json_mode_byte_for_byte():
    """1,000 seeded JSON-mode walks, nesting up to the cap: after every prefix the two guides allow the same bytes
    and agree on acceptance; then one-byte mutations of each walk are accepted or rejected alike."""
    jg = guided.compile_json_guide(TABLE, EOS)
    st, sa = pda({"type": "object"})
    rng = random.Random(11)
    deepest = 0

    def run(data):
        """(the prefix length both read, the JSON guide accepts, the schema guide accepts)."""
        jc, sc = (0, 0, 0), (0, [])
        for i, b in enumerate(data):
            lj, ls = json_legal(jg.trans, jc), schema_legal(st, sc[0], len(sc[1]))
            assert np.array_equal(lj, ls), (data[:i], np.nonzero(lj != ls)[0][:4])
            if not lj[b]:
                return i, False, False
            jc = guided.json_step(jg.trans, jc, b)
            sc = oracle.byte_step(st, len(st), sc[0], sc[1], 0, b)[:2]
        return len(data), jc[0] == jg.done, bool(sa[sc[0]]) and not sc[1]

    for walk in range(1000):
        greedy = rng.random() < 0.2                # some walks nest as deep as they can
        cfg, out = (0, 0, 0), bytearray()
        if greedy:                                 # ... from a prefix that is already near or at the cap
            out += b'{"k":' + b"[" * rng.choice((29, 30, 31))
            for x in out:
                cfg = guided.json_step(jg.trans, cfg, x)
        for _ in range(rng.choice((10, 40, 120, 300))):
            legal = np.nonzero(json_legal(jg.trans, cfg))[0]
            if not len(legal):
                break                              # DONE
            groups = {}
            for b in legal:
                groups.setdefault(int(jg.trans[cfg[0], b]), []).append(int(b))
            opens = [b for b in legal if b in (0x7B, 0x5B)]
            b = rng.choice(opens) if greedy and opens else rng.choice(groups[rng.choice(sorted(groups))])
            out.append(b)
            cfg = guided.json_step(jg.trans, cfg, b)
            deepest = max(deepest, cfg[1])
        n, aj, as_ = run(bytes(out))
        assert n == len(out) and aj == as_
        for _ in range(3):
            bad = bytearray(out)
            if not bad:
                break
            bad[rng.randrange(len(bad))] = rng.choice(b'{}[]",: 0-a\\\xe2\x80') if rng.random() < 0.7 else rng.randrange(256)
            n, aj, as_ = run(bytes(bad))
            assert aj == as_
    assert deepest == 32
    assert len(st) <= guided.GUIDE_JSON_MAX_STATES      # nothing was spent on the stack of return states


REFUSALS = [
    ({"type": "object", "oneOf": [{}]}, "oneOf"), ({"not": {}}, "not"), ({"if": {}, "then": {}}, "if"),
    ({"type": "object", "patternProperties": {"a": {}}}, "patternProperties"),
    ({"type": "array", "prefixItems": [{}]}, "prefixItems"), ({"type": "integer", "minimum": 0}, "minimum"),
    ({"type": "number", "multipleOf": 2}, "multipleOf"), ({"type": "array", "uniqueItems": True}, "uniqueItems"),
    ({"type": "object", "properties": {"a": False}}, "false"), ({"type": "object", "frobnicate": 1}, "frobnicate"),
    ({"type": "object", "properties": {"a": {"type": "integer", "maximum": 3}}}, "#/properties/a/maximum"),
    ({"type": "object", "properties": {"a": {}}, "additionalProperties": True}, "additionalProperties"),
    ({"type": "object", "properties": {"a": {}}, "additionalProperties": {"type": "string"}}, "additionalProperties"),
    ({"type": "object", "properties": {"a": {}}, "required": ["b"]}, "required"),
    ({"type": "array", "minItems": 3, "maxItems": 2}, "minItems"), ({"type": "array", "maxItems": 257}, "maxItems"),
    ({"type": "string", "maxLength": 300}, "maxLength"), ({"type": "string", "minLength": -1}, "minLength"),
    ({"type": "string", "pattern": "a+"}, "pattern"), ({"type": "string", "pattern": "^a+$", "maxLength": 3}, "pattern"),
    ({"type": "string", "pattern": '^"+$'}, "pattern"), ({"type": "string", "pattern": "^(?=a)a$"}, "pattern"),
    ({"type": "integer", "minLength": 1}, "minLength"), ({"type": "float"}, "type"),
    ({"allOf": [{}, {}]}, "allOf"), ({"anyOf": []}, "anyOf"), ({"anyOf": [{}], "type": "object"}, "anyOf"),
    ({"$ref": "#/$defs/x"}, "\\$ref"), ({"$ref": "http://example.com/s.json"}, "\\$ref"),
    ({"$defs": {"x": {}}, "$ref": "#/$defs/x", "type": "object"}, "next to \\$ref"),
    # recursion: the target must be an object or an array in every alternative
    ({"anyOf": [{"type": "integer"}, {"type": "array", "items": {"$ref": "#"}}]}, "recursive"),
    # a required member that refers to its own object has no finite document
    ({"type": "object", "properties": {"self": {"$ref": "#"}}, "required": ["self"]}, "dead end"),
    # at the depth cap a required free-form member of a recursive object could not be written
    ({"type": "object", "properties": {"m": {"type": "object"}, "n": {"anyOf": [{"$ref": "#"}, {"type": "null"}]}},
      "required": ["m", "n"]}, "dead end"),
    # one byte that could open an inlined object and a free-form one
    ({"anyOf": [{"type": "object", "properties": {"a": {}}}, {"type": "object"}]}, "could open"),
    # two different frames on '{'
    ({"$defs": {"a": {"type": "object", "properties": {"x": {"anyOf": [{"$ref": "#/$defs/a"}, {"type": "null"}]}}},
                "b": {"type": "object", "properties": {"y": {"anyOf": [{"$ref": "#/$defs/b"}, {"type": "null"}]}}}},
      "anyOf": [{"$ref": "#/$defs/a"}, {"$ref": "#/$defs/b"}]}, "could open"),
    # more states than the cap
    ({"type": "array", "maxItems": 200, "items": {"type": "string", "maxLength": 200}}, "more than 16384 states"),
]


@pytest.mark.parametrize("schema,what", REFUSALS, ids=[f"{i}-{w}" for i, (_, w) in enumerate(REFUSALS)])
def test_refusals_name_the_keyword_or_the_case(schema, what):
    with pytest.raises(ValueError, match=what):
        guided.schema_to_pda(schema)
    with pytest.raises(ValueError, match=what):
        SamplingParams(guided_json=schema)                  # the same refusal, early


def test_a_byte_without_a_single_byte_token_is_named():
    schema = {"type": "object", "properties": {"a": {"type": "integer"}}, "required": ["a"]}
    g = guided.compile_schema_guide(schema, TABLE, EOS)
    assert isinstance(g, guided.SchemaGuide) and g.eos == EOS and g.key[0] == "json_schema"
    for ch in ('"', "}", "7", "a", ":"):
        short = list(TABLE)
        short[3 + ord(ch)] = None
        with pytest.raises(ValueError, match="0x%02X" % ord(ch)):
            guided.compile_schema_guide(schema, short, EOS)
    only_eos = list(TABLE)
    only_eos[3 + ord("{")] = None
    only_eos[EOS] = b"{"
    with pytest.raises(ValueError, match="0x7B"):
        guided.compile_schema_guide(schema, only_eos, EOS)
    no_e = list(TABLE)                                       # an integer needs no 'e': the byte is on no transition
    no_e[3 + ord("e")] = None
    guided.compile_schema_guide(schema, no_e, EOS)


def test_compile_guide_caches_by_the_canonical_schema_and_refuses_like_json_mode():
    a = {"type": "object", "properties": {"x": {"type": "integer"}, "y": {"type": "string"}}, "required": ["x"]}
    b = {"required": ["x"], "properties": {"x": {"type": "integer"}, "y": {"type": "string"}}, "type": "object"}
    assert list(a) != list(b) and json.dumps(a) != json.dumps(b)
    g = guided.compile_guide(SamplingParams(guided_json=a), 1024, EOS, TABLE)
    assert isinstance(g, guided.SchemaGuide) and g.key[0] == "json_schema" and g.key[-1] == guided.id_of(TABLE)
    assert guided.compile_guide(SamplingParams(guided_json=b), 1024, EOS, TABLE) is g
    assert guided.compile_guide(SamplingParams(guided_json=json.dumps(b)), 1024, EOS, TABLE) is g
    other = dict(a, required=["x", "y"])
    assert guided.compile_guide(SamplingParams(guided_json=other), 1024, EOS, TABLE) is not g
    assert guided.walk(g, 0, [3 + ord(ch) for ch in '{"x":1']) [1:] == (0, ())
    sp = SamplingParams(guided_json=a)
    with pytest.raises(ValueError, match="end-of-sequence"):
        guided.compile_guide(sp, 1024, None, TABLE)
    with pytest.raises(ValueError, match="byte table"):
        guided.compile_guide(sp, 1024, EOS, None)
    for bad in ({"guided_json": a, "ignore_eos": True}, {"guided_json": a, "guided_regex": "a"},
                {"guided_json": a, "guided_json_object": True}, {"guided_json": a, "allowed_token_ids": [5]},
                {"guided_json": a, "guided_choice": [[5]]}, {"guided_json": a, "pooling": "last"},
                {"guided_json": "{"}, {"guided_json": "[1]"}, {"guided_json": 5}, {"guided_json": ["a"]}):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    assert SamplingParams(guided_json=json.dumps(a)).guided_json == a and SamplingParams(guided_json=a).guided
    assert not SamplingParams().guided and SamplingParams().guided_json is None
