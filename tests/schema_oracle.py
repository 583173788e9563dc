"""What the schema tests share: the rule for a grammar mask by brute force (one token at a time through
Dfa.step -- aios_amd.runtime.json_schema.SchemaGrammar.mask is the vectorised form the GPU kernel is held to), a
small JSON-schema validator for the accepted subset, random walks through a DFA, schemas and vocabularies."""
import json

import numpy as np

from aios_amd.runtime import json_schema as JS


# ---- the mask rule, token by token ----------------------------------------------------------------------
def brute_mask(dfa, tokens, eos_ids, state: int) -> bytes:
    ok = np.zeros(len(tokens), np.uint8)
    for t, data in enumerate(tokens):
        if t in eos_ids:
            ok[t] = bool(dfa.accept[state])
        elif data:
            ok[t] = dfa.step(state, data) != 0
    return np.packbits(ok, bitorder="little").tobytes()


# ---- validator for the accepted subset ------------------------------------------------------------------
def validate(v, sch, root=None) -> bool:
    root = sch if root is None else root
    if "$ref" in sch:
        _, table, name = sch["$ref"].split("/")
        return validate(v, root[table][name], root)
    if "const" in sch:
        return type(v) is type(sch["const"]) and v == sch["const"]
    if "enum" in sch:
        return any(type(v) is type(e) and v == e for e in sch["enum"])
    for key in ("anyOf", "oneOf"):
        if key in sch:
            return any(validate(v, s, root) for s in sch[key])
    t = sch.get("type", "object" if "properties" in sch else "array")
    if isinstance(t, list):
        return any(validate(v, dict(sch, type=one), root) for one in t)
    if t == "null":
        return v is None
    if t == "boolean":
        return isinstance(v, bool)
    if t == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    if t == "number":
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    if t == "string":
        return (isinstance(v, str) and sch.get("minLength", 0) <= len(v) and
                ("maxLength" not in sch or len(v) <= sch["maxLength"]))
    if t == "array":
        return (isinstance(v, list) and sch.get("minItems", 0) <= len(v) and
                ("maxItems" not in sch or len(v) <= sch["maxItems"]) and
                all(validate(x, sch["items"], root) for x in v))
    props = sch.get("properties", {})
    return (isinstance(v, dict) and all(k in props for k in v) and all(k in v for k in sch.get("required", [])) and
            [k for k in props if k in v] == list(v) and all(validate(x, props[k], root) for k, x in v.items()))


def parse_and_validate(text: str, schema) -> bool:
    """the text is JSON (strictly: no NaN / Infinity) and an instance of the schema, keys in declared order"""
    def bad(_):
        raise ValueError("constant")
    return validate(json.loads(text, parse_constant=bad), schema)


# ---- walks ----------------------------------------------------------------------------------------------
def random_walk(dfa, rng, max_bytes: int = 4000) -> bytes:
    """random bytes from the initial state until an accepting state is left for good; past max_bytes / 2 the
    walk takes the shortest way to acceptance"""
    S = dfa.n_states
    dist = np.full(S, 1 << 30)
    dist[dfa.accept.astype(bool)] = 0
    changed = True
    while changed:  # (Bellman-Ford over a few thousand states: fine for a test)
        nd = np.minimum(dist, 1 + np.where(dfa.trans != 0, dist[dfa.trans], 1 << 30).min(axis=1))
        nd[0] = 1 << 30
        changed = bool((nd != dist).any())
        dist = nd
    cls_bytes = [np.nonzero(dfa.byte_class == c)[0] for c in range(dfa.n_classes)]
    s, out = dfa.INITIAL, bytearray()
    while True:
        live = [c for c in range(dfa.n_classes) if dfa.trans[s, c] != 0]
        if dfa.accept[s] and (not live or rng.random() < 0.3 or len(out) > max_bytes // 2):
            return bytes(out)
        if len(out) > max_bytes // 2:
            live = [c for c in live if dist[dfa.trans[s, c]] < dist[s]]
        c = live[int(rng.integers(len(live)))]
        out.append(int(rng.choice(cls_bytes[c])))
        s = int(dfa.trans[s, c])
        assert len(out) <= max_bytes


# ---- schemas --------------------------------------------------------------------------------------------
SCHEMAS = {
    "enum": {"enum": ["red", "green", 3, None, True, {"a": [1, 2]}, "café"]},
    "const": {"const": {"k": "v", "n": 1.5}},
    "boolean": {"type": "boolean"},
    "null_or_int": {"type": ["null", "integer"]},
    "number": {"type": "number"},
    "string": {"type": "string"},
    "string_bounds": {"type": "string", "minLength": 2, "maxLength": 5},
    "array_bounds": {"type": "array", "items": {"type": "boolean"}, "minItems": 1, "maxItems": 3},
    "array_open": {"type": "array", "items": {"type": "integer"}},
    "object": {"type": "object", "properties": {"name": {"type": "string", "maxLength": 8},
                                                "age": {"type": "integer"},
                                                "tags": {"type": "array", "items": {"enum": ["a", "b"]}, "maxItems": 2},
                                                "ok": {"type": "boolean"}},
               "required": ["name", "ok"], "additionalProperties": False},
    "all_optional": {"type": "object", "properties": {"a": {"type": "null"}, "b": {"type": "boolean"},
                                                      "c": {"const": 1}}},
    "any_of": {"anyOf": [{"type": "string", "maxLength": 3}, {"type": "array", "items": {"type": "null"}, "maxItems": 2}]},
    "one_of": {"oneOf": [{"type": "integer"}, {"type": "object", "properties": {"x": {"type": "number"}}, "required": ["x"]}]},
    "ref": {"type": "object", "properties": {"p": {"$ref": "#/$defs/point"}, "q": {"$ref": "#/definitions/flag"}},
            "required": ["p"], "$defs": {"point": {"type": "array", "items": {"type": "integer"}, "minItems": 2, "maxItems": 2}},
            "definitions": {"flag": {"type": "boolean"}}},
}

# finite languages for the runtime tests (longest_path() is not None): enums, booleans, short strings and arrays
BOUNDED = {
    "tool_call": {"type": "object", "properties": {"tool": {"enum": ["fs.read", "fs.write", "net.get"]},
                                                   "dry_run": {"type": "boolean"},
                                                   "path": {"type": "string", "maxLength": 3}},
                  "required": ["tool", "path"]},
    "flags": {"type": "array", "items": {"type": "boolean"}, "minItems": 1, "maxItems": 3},
    "choice": {"enum": ["yes", "no", None, 7]},
}


# ---- vocabularies ---------------------------------------------------------------------------------------
def make_vocab(V: int, seed: int = 0, eos=(2,)):
    """V byte strings: control tokens (empty, the eos ids among them), every single byte, JSON punctuation and
    literals, multi-byte UTF-8 characters whole and split across tokens, a 70-byte token, random ASCII words"""
    rng = np.random.default_rng(seed)
    toks = [b"", b"", b""] + [bytes([c]) for c in range(256)]
    toks += [b'{"', b'":', b'": ', b'",', b'", "', b'"}', b"},", b"[", b"]", b"true", b"false", b"null", b"tru", b"e",
             b'{"name', b'{"tool":"', b"fs.", b"read", b'":"', b"\\u00", b"e9", b'\\"', b"12", b"-0", b".5e+", b"1.",
             b"x" * 70, b'"' + b"y" * 68 + b'"', b"a" * 64]
    for ch in ("é", "中", "\U0001f600", "߿", "퟿"):
        raw = ch.encode("utf-8")
        toks += [raw, b'"' + raw] + [raw[:i] for i in range(1, len(raw))] + [raw[i:] for i in range(1, len(raw))]
    toks += [b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80"]  # overlong, surrogate, too large, stray
    alphabet = np.frombuffer(b'abcdefghijklmnopqrstuvwxyz0123456789 {}[]:,."\\-_', np.uint8)
    while len(toks) < V:
        n = int(rng.integers(1, 9))
        toks.append(bytes(rng.choice(alphabet, n)))
    toks = toks[:V]
    for e in eos:
        toks[e] = b""
    return toks, sorted(eos)


# ---- runtime -------------------------------------------------------------------------------------------
class Spy:
    """an engine with its grammar-related calls recorded"""

    def __init__(self, eng):
        self._eng = eng
        self.grammar_rows, self.masks = [], []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def __dir__(self):
        return dir(self._eng)


def spy_on(eng):
    """Spy that forwards hasattr() faithfully: only the calls the engine has are wrapped"""
    spy = Spy(eng)
    if hasattr(eng, "set_grammar_rows"):
        def set_grammar_rows(gids, states):
            spy.grammar_rows.append((list(gids), list(states)))
            return eng.set_grammar_rows(gids, states)
        spy.set_grammar_rows = set_grammar_rows
    if hasattr(eng, "decode_sample"):
        def decode_sample(mask):
            spy.masks.append(len(mask))
            return eng.decode_sample(mask)
        spy.decode_sample = decode_sample
    return spy


def run_requests(sched, reqs, together=True, close=True):
    import threading

    evs, box = [threading.Event() for _ in reqs], {}
    try:
        for i, r in enumerate(reqs):
            r.on_done = lambda res, i=i: (box.__setitem__(i, res), evs[i].set())
        if together:
            with sched.cv:
                for r in reqs:
                    sched.submit(r)
            for e in evs:
                assert e.wait(120)
        else:
            for r, e in zip(reqs, evs):
                sched.submit(r)
                assert e.wait(120)
    finally:
        if close:
            sched.close()
    return [box[i] for i in range(len(reqs))]
