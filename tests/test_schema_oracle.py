"""The JSON-schema -> DFA compiler and the host grammar (aios_amd.runtime.json_schema) on the CPU: random walks
through each DFA give texts that parse and validate, hand-written invalid texts are rejected at the right byte,
every refusal names its path, the caps refuse, and SchemaGrammar.mask equals token-by-token stepping."""
import numpy as np
import pytest

import schema_oracle as SO
from aios_amd.runtime import json_schema as JS


@pytest.fixture(scope="module")
def dfas():
    return {k: JS.compile_schema(s) for k, s in SO.SCHEMAS.items()}


@pytest.mark.parametrize("name", list(SO.SCHEMAS))
def test_random_walks_parse_and_validate(dfas, name):
    dfa, schema = dfas[name], SO.SCHEMAS[name]
    rng = np.random.default_rng(hash(name) % 1000)
    seen = set()
    for _ in range(60):
        text = SO.random_walk(dfa, rng)
        assert dfa.rejects_at(text) is None
        assert SO.parse_and_validate(text.decode("utf-8"), schema), text
        seen.add(text)
    assert len(seen) > 1 or name == "const"


def test_table_invariants(dfas):
    for name, d in dfas.items():
        S, C = d.trans.shape
        assert d.byte_class.shape == (256,) and d.byte_class.max() == C - 1 and d.accept.shape == (S,)
        assert d.trans.dtype == np.uint16 and d.trans.max() < S and not d.trans[0].any() and not d.accept[0], name
        # trimmed: every live state is reachable from the initial one and reaches an accepting one
        fwd, todo = {d.INITIAL}, [d.INITIAL]
        while todo:
            for t in set(d.trans[todo.pop()].tolist()) - fwd - {0}:
                fwd.add(t)
                todo.append(t)
        assert fwd == set(range(1, S)), name
        back = set(np.nonzero(d.accept)[0].tolist())
        grew = True
        while grew:
            more = {s for s in range(1, S) if s not in back and back & set(d.trans[s].tolist())}
            grew = bool(more)
            back |= more
        assert back == set(range(1, S)), name
        assert ((d.terminal == 1) == ((d.accept == 1) & ~d.trans.any(axis=1))).all()


def test_longest_path(dfas):
    assert dfas["boolean"].longest_path() == 5
    assert dfas["const"].longest_path() == len(b'{"k":"v","n":1.5}')
    assert dfas["array_bounds"].longest_path() == len(b"[false, false, false]")
    assert dfas["string_bounds"].longest_path() == 2 + 5 * 12         # five escaped surrogate pairs
    for name in ("string", "array_open"):
        assert dfas[name].longest_path() is None
    for name, s in SO.BOUNDED.items():
        assert JS.compile_schema(s).longest_path() is not None, name


REJECTS = [  # (schema, text, index of the first byte that cannot follow; len(text): a prefix that is not accepted)
    ("boolean", b"True", 0), ("boolean", b"true ", 4), ("boolean", b" true", 0), ("boolean", b"tru", 3),
    ("null_or_int", b"01", 1), ("null_or_int", b"-", 1), ("null_or_int", b"1.0", 1), ("null_or_int", b"nul", 3),
    ("number", b"1.", 2), ("number", b"1e", 2), ("number", b"1.5e+", 5), ("number", b".5", 0), ("number", b"NaN", 0),
    ("string", b'"a\nb"', 2), ("string", b'"\\x"', 2), ("string", b'"\\u12g4"', 5), ("string", b'"\xc0\x80"', 1),
    ("string", b'"\xed\xa0\x80"', 2), ("string", b'"\xf4\x90\x80\x80"', 2), ("string", b'"\xe4\xb8"', 3),
    ("string", b'"ab', 3), ("string", b'"a" ', 3),
    # surrogate escapes: a pair is ONE character (what a JSON parser returns), a lone one is refused
    ("string", b'"\\ud83dx"', 7), ("string", b'"\\ud83d\\u0041"', 9), ("string", b'"\\ude00"', 4),
    ("string", b'"\\uDC00"', 4), ("string_bounds", b'"\\ud83d\\ude00"', 13),
    ("string_bounds", b'"\\ud83d\\ude00\\uD83D\\uDE00\\ud83d\\ude00"x', 38),
    ("string_bounds", b'"a"', 2), ("string_bounds", b'"abcdef"', 6), ("string_bounds", b'"\xc3\xa9\xc3\xa9"x', 6),
    ("array_bounds", b"[]", 1), ("array_bounds", b"[true,true,true,true]", 15), ("array_bounds", b"[true ,true]", 5),
    ("array_bounds", b"[true,  true]", 7), ("array_bounds", b"[ true]", 1), ("array_bounds", b"[true,]", 6),
    ("object", b'{"age":1}', 2), ("object", b'{"name":"x"}', 11), ("object", b'{"name":"x","ok":true,"age":1}', 21),
    ("object", b'{"name":"x","tags":["c"]}', 21), ("object", b'{"name":"x","other":1}', 14),
    ("object", b'{"name":"123456789"', 17), ("object", b'{"name" :"x"', 7), ("object", b'{"name":  "x"', 9),
    ("all_optional", b'{"b":true,"a":null}', 11), ("all_optional", b'{"c":2}', 5), ("all_optional", b"{,", 1),
    ("enum", b'"blue"', 1), ("enum", b"4", 0), ("enum", b'{"a":[1, 2]}', 8), ("const", b'{"n":1.5}', 2),
    ("ref", b'{"p":[1]}', 7), ("ref", b'{"p":[1,2,3]}', 9), ("ref", b'{"q":true}', 2),
]


@pytest.mark.parametrize("name,text,at", REJECTS)
def test_invalid_texts_are_rejected_at_the_right_byte(dfas, name, text, at):
    assert dfas[name].rejects_at(text) == at


ACCEPTS = [
    ("object", b'{"name":"x","ok":true}'), ("object", b'{"name": "x", "age": -12, "tags": ["a", "b"], "ok": false}'),
    ("all_optional", b"{}"), ("all_optional", b'{"a":null,"c":1}'), ("all_optional", b'{"b":false}'),
    ("string", '"é中\U0001f600 \\" \\u00e9 \\n"'.encode("utf-8")), ("string", b'""'), ("number", b"-0.25e-3"),
    ("string", b'"\\ud83d\\ude00 \\uD7ff \\ue000 \\udbff\\uDFFF"'), ("string_bounds", b'"\\ud83d\\ude00\\u00e9"'),
    ("string_bounds", b'"' + b"\\ud83d\\ude00" * 5 + b'"'),
    ("number", b"10"), ("enum", '"café"'.encode("utf-8")), ("enum", b'{"a":[1,2]}'), ("enum", b"null"),
    ("ref", b'{"p":[1,-2],"q":true}'), ("one_of", b'{"x":1.5}'), ("one_of", b"7"), ("any_of", b"[null,null]"),
]


@pytest.mark.parametrize("name,text", ACCEPTS)
def test_valid_texts_are_accepted(dfas, name, text):
    assert dfas[name].rejects_at(text) is None
    assert SO.parse_and_validate(text.decode("utf-8"), SO.SCHEMAS[name])


REFUSED = [
    ({}, "$"), ({"type": "object", "properties": {"a": {}}}, "$.properties.a"),
    ({"type": "array"}, "$.items"), ({"type": "array", "items": {}}, "$.items"),
    ({"type": "string", "pattern": "^a"}, "$.pattern"), ({"type": "string", "format": "date"}, "$.format"),
    ({"type": "integer", "minimum": 0}, "$.minimum"), ({"type": "number", "exclusiveMaximum": 1}, "$.exclusiveMaximum"),
    ({"not": {"type": "null"}}, "$.not"), ({"allOf": [{"type": "null"}]}, "$.allOf"),
    ({"type": "object", "patternProperties": {"^a": {"type": "null"}}}, "$.patternProperties"),
    ({"type": "object", "properties": {"a": {"type": "object", "properties": {"b": {"type": "string", "pattern": "x"}}}}},
     "$.properties.a.properties.b.pattern"),
    ({"type": "array", "items": {"anyOf": [{"type": "null"}, {"type": "integer", "multipleOf": 2}]}},
     "$.items.anyOf[1].multipleOf"),
    ({"type": "object", "properties": {"n": {"$ref": "#/$defs/node"}},
      "$defs": {"node": {"type": "object", "properties": {"next": {"$ref": "#/$defs/node"}}}}},
     "$.properties.n.properties.next.$ref"),
    ({"$ref": "#/$defs/missing"}, "$.$ref"), ({"$ref": "http://example.com/s.json"}, "$.$ref"),
    ({"type": "float"}, "$.type"), ({"type": "string", "maxLength": JS.MAX_LENGTH_CAP + 1}, "$.maxLength"),
    ({"type": "string", "minLength": 3, "maxLength": 2}, "$.maxLength"), ({"type": "string", "maxLength": -1}, "$.maxLength"),
    ({"type": "array", "items": {"type": "null"}, "maxItems": JS.MAX_ITEMS_CAP + 1}, "$.maxItems"),
    ({"type": "object", "properties": {"a": {"type": "null"}}, "required": ["b"]}, "$.required"),
    ({"type": "object", "properties": {"a": {"type": "null"}}, "additionalProperties": {"type": "null"}},
     "$.additionalProperties"),
    ({"enum": []}, "$.enum"), ("string", "$"),
]


@pytest.mark.parametrize("schema,path", REFUSED, ids=[p + "#" + str(i) for i, (_, p) in enumerate(REFUSED)])
def test_every_refusal_names_its_path(schema, path):
    with pytest.raises(JS.SchemaError) as e:
        JS.compile_schema(schema)
    assert e.value.path == path and str(e.value).startswith(path + ":")


def test_the_state_cap_refuses_and_never_truncates(monkeypatch):
    schema = {"type": "array", "items": {"type": "string", "maxLength": 40}, "maxItems": 8}
    full = JS.compile_schema(schema)
    assert full.n_states > 300
    monkeypatch.setattr(JS, "MAX_STATES", full.n_states - 1)
    with pytest.raises(JS.SchemaError, match="DFA states") as e:
        JS.compile_schema(schema)
    assert e.value.path == "$"
    monkeypatch.setattr(JS, "MAX_STATES", full.n_states)
    again = JS.compile_schema(schema)  # exactly at the cap: the whole language, the same table
    assert again.n_states == full.n_states and (again.trans == full.trans).all()
    assert JS.MAX_STATES <= 65535 and np.iinfo(full.trans.dtype).max >= JS.MAX_STATES


def test_mask_agrees_with_token_by_token_stepping(dfas):
    tokens, eos = SO.make_vocab(300, eos=(2, 7))
    assert max(len(t) for t in tokens) == 70 and tokens[2] == tokens[7] == b""
    vocab = JS.Vocab(tokens, eos)
    for name in ("object", "string", "enum", "ref"):
        d = dfas[name]
        g = JS.SchemaGrammar(d, vocab)
        states = range(d.n_states) if d.n_states <= 120 else np.random.default_rng(1).choice(d.n_states, 120, False)
        for s in states:
            assert g.mask_of(int(s)) == SO.brute_mask(d, tokens, eos, int(s)), (name, s)
        assert g.memo_bytes == len(list(states)) * 38
        st = g.initial()
        assert g.mask(st) == g.mask_of(1) and not g.complete(st)
    # accept_token walks the state; a rejected or empty token changes nothing
    g = JS.SchemaGrammar(dfas["boolean"], vocab)
    st = g.initial()
    assert not g.accept_token(st, 0) and not g.accept_token(st, 3 + ord("x")) and st.s == 1
    assert g.accept_token(st, tokens.index(b"tru")) and not g.complete(st) and not g.accepting(st)
    assert g.accept_token(st, tokens.index(b"e")) and g.complete(st) and g.accepting(st)
    assert g.token_dead_states() == []
    # a vocabulary without the letter "u" cannot spell true or null: those states are token-dead
    bare = JS.Vocab([b"", b"t", b"r", b"e", b"f", b"a", b"l", b"s"], [0])
    assert JS.SchemaGrammar(dfas["boolean"], bare).token_dead_states() != []
