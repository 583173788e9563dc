"""JSON-schema constrained decoding: schema -> byte-level DFA, and the host grammar over it.

A schema without recursion describes a regular language, so the whole grammar is one table: the device walks
every vocabulary entry's bytes through it (csrc/kernels/grammar_mask.hip) and the host does the same in numpy
(SchemaGrammar.mask -- the rule the kernel is tested against, and the path of the CPU and tensor-parallel
tiers and of rows that combine a schema with banned tokens).

Accepted subset (everything else raises SchemaError naming the JSON path of the offending keyword):
  type (one of object / array / string / integer / number / boolean / null, or a list of them), properties +
  required (properties are emitted in DECLARED order, optional ones may be skipped, additionalProperties is
  treated as false: llama.cpp's converter rule), items + minItems / maxItems, enum / const (any JSON literal,
  emitted in its compact canonical spelling), minLength / maxLength (counted in code points, as a JSON
  parser returns them: a UTF-8 sequence, an escape, or an escaped surrogate pair count one each; a lone
  surrogate escape is refused), anyOf / oneOf (both a union), $ref into $defs / definitions when not recursive (inlined).
  Annotations (title, description, default, examples, $schema, $id, $comment) are ignored.

Text rules:
  * strings are valid UTF-8 (no overlongs, no surrogates, nothing above U+10FFFF) with JSON's escapes; control
    bytes below 0x20 must be escaped;
  * whitespace: ONE optional space after ':' and after ',' -- nowhere else, and none after the top-level value;
  * numbers: -?(0|[1-9][0-9]{0,15}), then for `number` an optional fraction of 1..16 digits and an optional
    exponent of 1..3 digits.  Bounded, so a schema of enums, booleans and bounded strings has no cycle.

Caps (a schema above one is refused, never truncated): maxLength <= MAX_LENGTH_CAP, maxItems <= MAX_ITEMS_CAP,
DFA states <= MAX_STATES.  The transition table's u16 entries would hold 65,535 states; the cap is lower because
the compiler is pure Python and its time grows with the states: measured 0.1 s at 1,064 states, 1.9 s at 10,274,
17 s at 41,026 (an array of 16 strings of up to 128 characters), so 16,384 keeps a compile, or a refusal, to a few
seconds.  The HTTP layer compiles in an executor, off its event loop, and compile_cached hands the table to the
scheduler, whose worker then does not compile it again.
"""
from __future__ import annotations

import json
import threading
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_LENGTH_CAP = 256
MAX_ITEMS_CAP = 64
MAX_STATES = 16384
MAX_NFA_STATES = 400_000
INT_DIGITS = 15   # digits after the first of an integer part
FRAC_DIGITS = 16
EXP_DIGITS = 3

_TYPES = ("object", "array", "string", "integer", "number", "boolean", "null")
_ANNOTATIONS = {"title", "description", "default", "examples", "$schema", "$id", "$comment", "$defs", "definitions"}
_KEYWORDS = {"type", "properties", "required", "additionalProperties", "items", "minItems", "maxItems", "enum", "const",
             "minLength", "maxLength", "anyOf", "oneOf", "$ref"}


class SchemaError(ValueError):
    """A schema outside the accepted subset; .path names the offending keyword."""

    def __init__(self, path: str, why: str):
        super().__init__(f"{path}: {why}")
        self.path = path
        self.why = why


# ------------------------------------------------------------------------------------------------ NFA
def _bits(*ranges) -> int:
    m = 0
    for r in ranges:
        lo, hi = (r, r) if isinstance(r, int) else r
        for c in range(lo, hi + 1):
            m |= 1 << c
    return m


_DIGIT = _bits((0x30, 0x39))
_DIGIT19 = _bits((0x31, 0x39))
_HEX = _bits((0x30, 0x39), (0x41, 0x46), (0x61, 0x66))
_D = _bits(0x44, 0x64)
_CONT = _bits((0x80, 0xBF))
_PLAIN = _bits((0x20, 0x7F)) & ~_bits(0x22, 0x5C)
_ESC1 = _bits(*b'"\\/bfnrt')


class _Nfa:
    """Thompson NFA: edges[s] = [(byte-set as a 256-bit int, target)], eps[s] = [target]."""

    def __init__(self):
        self.edges: List[List[Tuple[int, int]]] = []
        self.eps: List[List[int]] = []

    def new(self) -> int:
        if len(self.edges) >= MAX_NFA_STATES:
            raise SchemaError("$", f"the schema needs more than {MAX_NFA_STATES} NFA states")
        self.edges.append([])
        self.eps.append([])
        return len(self.edges) - 1

    # combinators: each takes the state to start from and returns the state it ends in
    def byte(self, a: int, mask: int) -> int:
        b = self.new()
        self.edges[a].append((mask, b))
        return b

    def lit(self, a: int, text: bytes) -> int:
        for c in text:
            a = self.byte(a, 1 << c)
        return a

    def opt_space(self, a: int) -> int:
        b = self.byte(a, 1 << 0x20)
        self.eps[a].append(b)
        return b

    def alt(self, a: int, builders) -> int:
        end = self.new()
        for f in builders:
            self.eps[f(a)].append(end)
        return end

    def repeat(self, a: int, f, lo: int, hi: Optional[int]) -> int:
        """f repeated lo..hi times (hi None: unbounded)."""
        for _ in range(lo):
            a = f(a)
        if hi is None:
            loop = self.new()
            self.eps[a].append(loop)
            self.eps[f(loop)].append(loop)
            return loop
        end = self.new()
        self.eps[a].append(end)
        for _ in range(hi - lo):
            a = f(a)
            self.eps[a].append(end)
        return end

    def char(self, a: int) -> int:
        """one string character: a plain byte, an escape, or a valid UTF-8 sequence"""
        end = self.byte(a, _PLAIN)
        e = self.byte(a, 1 << 0x5C)
        self.edges[e].append((_ESC1, end))
        # \uXXXX: one character.  D800..DBFF must be followed by \uDC00..\uDFFF and the pair is ONE character (the
        # code point a JSON parser returns); a lone surrogate escape is refused
        u = self.byte(e, 1 << 0x75)
        h3 = self.new()  # three hex digits left
        h2 = self.new()
        h1 = self.new()
        self.edges[u].append((_HEX & ~_D, h3))
        self.edges[h3].append((_HEX, h2))
        self.edges[h2].append((_HEX, h1))
        self.edges[h1].append((_HEX, end))
        d = self.byte(u, _D)
        self.edges[d].append((_bits((0x30, 0x37)), h2))
        hi = self.byte(self.byte(self.byte(d, _bits(0x38, 0x39, 0x41, 0x42, 0x61, 0x62)), _HEX), _HEX)
        lo = self.byte(self.byte(self.byte(hi, 1 << 0x5C), 1 << 0x75), _D)
        self.edges[self.byte(lo, _bits((0x43, 0x46), (0x63, 0x66)))].append((_HEX, h1))
        c1 = self.new()  # one continuation byte left
        self.edges[c1].append((_CONT, end))
        c2 = self.new()  # two left
        self.edges[c2].append((_CONT, c1))
        self.edges[a].append((_bits((0xC2, 0xDF)), c1))
        self.edges[self.byte(a, 1 << 0xE0)].append((_bits((0xA0, 0xBF)), c1))
        self.edges[a].append((_bits((0xE1, 0xEC), (0xEE, 0xEF)), c2))
        self.edges[self.byte(a, 1 << 0xED)].append((_bits((0x80, 0x9F)), c1))
        self.edges[self.byte(a, 1 << 0xF0)].append((_bits((0x90, 0xBF)), c2))
        self.edges[self.byte(a, _bits((0xF1, 0xF3)))].append((_CONT, c2))
        self.edges[self.byte(a, 1 << 0xF4)].append((_bits((0x80, 0x8F)), c2))
        return end

    def string(self, a: int, lo: int, hi: Optional[int]) -> int:
        a = self.byte(a, 1 << 0x22)
        a = self.repeat(a, self.char, lo, hi)
        return self.byte(a, 1 << 0x22)

    def integer(self, a: int) -> int:
        s = self.new()
        self.eps[a].append(s)
        self.edges[a].append((1 << 0x2D, s))
        end = self.byte(s, 1 << 0x30)
        d = self.byte(s, _DIGIT19)
        self.eps[self.repeat(d, lambda x: self.byte(x, _DIGIT), 0, INT_DIGITS)].append(end)
        return end

    def number(self, a: int) -> int:
        a = self.integer(a)
        digit = lambda x: self.byte(x, _DIGIT)  # noqa: E731
        a = self.repeat(a, lambda x: self.repeat(self.byte(x, 1 << 0x2E), digit, 1, FRAC_DIGITS), 0, 1)

        def exp(x):
            x = self.byte(x, _bits(0x45, 0x65))
            s = self.new()
            self.eps[x].append(s)
            self.edges[x].append((_bits(0x2B, 0x2D), s))
            return self.repeat(s, digit, 1, EXP_DIGITS)
        return self.repeat(a, exp, 0, 1)


def _literal(v) -> bytes:
    return json.dumps(v, separators=(",", ":"), ensure_ascii=False, sort_keys=False).encode("utf-8")


class _Builder:
    def __init__(self, root: dict):
        self.root = root
        self.nfa = _Nfa()

    def _bound(self, sch: dict, key: str, path: str, cap: int, default):
        if key not in sch:
            return default
        v = sch[key]
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise SchemaError(f"{path}.{key}", "must be a non-negative integer")
        if v > cap:
            raise SchemaError(f"{path}.{key}", f"above the cap of {cap}")
        return v

    def _resolve(self, ref, path: str):
        if not isinstance(ref, str) or not (ref.startswith("#/$defs/") or ref.startswith("#/definitions/")):
            raise SchemaError(f"{path}.$ref", "only #/$defs/NAME and #/definitions/NAME are supported")
        _, table, name = ref.split("/", 2)
        name = name.replace("~1", "/").replace("~0", "~")
        defs = self.root.get(table)
        if not isinstance(defs, dict) or name not in defs:
            raise SchemaError(f"{path}.$ref", f"{ref} does not resolve")
        return defs[name]

    def value(self, a: int, sch, path: str, refs: tuple = ()) -> int:
        n = self.nfa
        if not isinstance(sch, dict):
            raise SchemaError(path, "a schema must be an object")
        for k in sch:
            if k not in _KEYWORDS and k not in _ANNOTATIONS:
                raise SchemaError(f"{path}.{k}", "unsupported keyword")
        if "$ref" in sch:
            ref = sch["$ref"]
            if ref in refs:
                raise SchemaError(f"{path}.$ref", f"recursive reference {ref}")
            return self.value(a, self._resolve(ref, path), path, refs + (ref,))
        if "const" in sch:
            return n.lit(a, _literal(sch["const"]))
        if "enum" in sch:
            vals = sch["enum"]
            if not isinstance(vals, list) or not vals:
                raise SchemaError(f"{path}.enum", "must be a non-empty list")
            return n.alt(a, [lambda x, v=v: n.lit(x, _literal(v)) for v in vals])
        for key in ("anyOf", "oneOf"):
            if key in sch:
                subs = sch[key]
                if not isinstance(subs, list) or not subs:
                    raise SchemaError(f"{path}.{key}", "must be a non-empty list")
                return n.alt(a, [lambda x, i=i, s=s: self.value(x, s, f"{path}.{key}[{i}]", refs)
                                 for i, s in enumerate(subs)])
        t = sch.get("type")
        if t is None:
            t = "object" if "properties" in sch else "array" if "items" in sch else None
        if t is None:
            raise SchemaError(path, "untyped schema (unbounded nesting is not regular)")
        if isinstance(t, list):
            if not t:
                raise SchemaError(f"{path}.type", "must not be empty")
            return n.alt(a, [lambda x, one=one: self.typed(x, sch, one, path, refs) for one in t])
        return self.typed(a, sch, t, path, refs)

    def typed(self, a: int, sch: dict, t, path: str, refs: tuple) -> int:
        n = self.nfa
        if t not in _TYPES:
            raise SchemaError(f"{path}.type", f"unknown type {t!r}")
        if t == "string":
            lo = self._bound(sch, "minLength", path, MAX_LENGTH_CAP, 0)
            hi = self._bound(sch, "maxLength", path, MAX_LENGTH_CAP, None)
            if hi is not None and hi < lo:
                raise SchemaError(f"{path}.maxLength", "below minLength")
            return n.string(a, lo, hi)
        if t == "integer":
            return n.integer(a)
        if t == "number":
            return n.number(a)
        if t == "boolean":
            return n.alt(a, [lambda x: n.lit(x, b"true"), lambda x: n.lit(x, b"false")])
        if t == "null":
            return n.lit(a, b"null")
        if t == "array":
            return self.array(a, sch, path, refs)
        return self.object(a, sch, path, refs)

    def array(self, a: int, sch: dict, path: str, refs: tuple) -> int:
        n = self.nfa
        lo = self._bound(sch, "minItems", path, MAX_ITEMS_CAP, 0)
        hi = self._bound(sch, "maxItems", path, MAX_ITEMS_CAP, None)
        if hi is not None and hi < lo:
            raise SchemaError(f"{path}.maxItems", "below minItems")
        if "items" not in sch:
            if hi == 0:
                return n.lit(a, b"[]")
            raise SchemaError(f"{path}.items", "an array needs items (untyped elements are not regular)")
        item = lambda x: self.value(x, sch["items"], f"{path}.items", refs)  # noqa: E731
        a = n.byte(a, 1 << 0x5B)
        close = n.new()
        if lo == 0:
            n.eps[a].append(close)
        if hi != 0:
            more = lambda x: item(n.opt_space(n.byte(x, 1 << 0x2C)))  # noqa: E731
            n.eps[n.repeat(item(a), more, max(lo - 1, 0), None if hi is None else hi - 1)].append(close)
        return n.byte(close, 1 << 0x5D)

    def object(self, a: int, sch: dict, path: str, refs: tuple) -> int:
        n = self.nfa
        props = sch.get("properties", {})
        if not isinstance(props, dict):
            raise SchemaError(f"{path}.properties", "must be an object")
        ap = sch.get("additionalProperties", False)
        if not isinstance(ap, bool):
            raise SchemaError(f"{path}.additionalProperties", "only a boolean is supported (and treated as false)")
        req = sch.get("required", [])
        if not isinstance(req, list) or any(not isinstance(k, str) for k in req):
            raise SchemaError(f"{path}.required", "must be a list of names")
        names = list(props)
        for k in req:
            if k not in props:
                raise SchemaError(f"{path}.required", f"{k!r} is not a declared property")
        need = [k in req for k in names]
        # after[i]: property i - 1 was the last one emitted (after[0]: none yet); from there any later property
        # may follow as long as no required one is skipped, and the object may close once none is left
        after = [n.byte(a, 1 << 0x7B)] + [n.new() for _ in names]
        close = n.new()
        starts = [n.new() for _ in names]
        for j, k in enumerate(names):
            x = n.lit(starts[j], _literal(k))
            x = n.opt_space(n.byte(x, 1 << 0x3A))
            n.eps[self.value(x, props[k], f"{path}.properties.{k}", refs)].append(after[j + 1])
        for i in range(len(names) + 1):
            src = after[i] if i == 0 else None
            for j in range(i, len(names)):
                if src is None:
                    src = n.opt_space(n.byte(after[i], 1 << 0x2C))
                n.eps[src].append(starts[j])
                if need[j]:
                    break
            if not any(need[i:]):
                n.eps[after[i]].append(close)
        return n.byte(close, 1 << 0x7D)


# ------------------------------------------------------------------------------------------------ DFA
class Dfa:
    """byte_class[256] u8, trans[S][C] u16, accept[S] / terminal[S] u8; state 0 is dead, state 1 initial, every
    other state is reachable and reaches an accepting state."""

    INITIAL = 1

    def __init__(self, byte_class, trans, accept):
        self.byte_class = np.ascontiguousarray(byte_class, np.uint8)
        self.trans = np.ascontiguousarray(trans, np.uint16)
        self.accept = np.ascontiguousarray(accept, np.uint8)
        self.n_states, self.n_classes = self.trans.shape
        self.terminal = (self.accept.astype(bool) & ~self.trans.astype(bool).any(axis=1)).astype(np.uint8)

    def step(self, state: int, data: bytes) -> int:
        for c in data:
            if state == 0:
                break
            state = int(self.trans[state, self.byte_class[c]])
        return state

    def rejects_at(self, data: bytes) -> Optional[int]:
        """index of the first byte that leaves the language's prefixes; len(data) when the text is a proper
        prefix (not accepted yet); None when it is accepted"""
        s = self.INITIAL
        for i, c in enumerate(data):
            s = int(self.trans[s, self.byte_class[c]])
            if s == 0:
                return i
        return None if self.accept[s] else len(data)

    def longest_path(self) -> Optional[int]:
        """bytes of the longest accepted text, or None when the DFA has a cycle (unbounded texts)"""
        S = self.n_states
        succ = [np.unique(self.trans[s][self.trans[s] != 0]).tolist() for s in range(S)]
        depth = [-1] * S   # -1 unvisited, -2 on the stack
        stack = [(self.INITIAL, 0)]
        depth[self.INITIAL] = -2
        while stack:
            s, i = stack[-1]
            if i < len(succ[s]):
                stack[-1] = (s, i + 1)
                t = succ[s][i]
                if depth[t] == -2:
                    return None
                if depth[t] == -1:
                    depth[t] = -2
                    stack.append((t, 0))
            else:
                depth[s] = max([1 + depth[t] for t in succ[s]], default=0)
                stack.pop()
        return depth[self.INITIAL]


def _classes(nfa: _Nfa) -> Tuple[np.ndarray, List[int]]:
    """bytes that no edge set tells apart share a class; returns byte -> class and one byte per class"""
    order = sorted({m for es in nfa.edges for m, _ in es})
    key_of: Dict[tuple, int] = {}
    byte_class = np.zeros(256, np.uint8)
    reps: List[int] = []
    for c in range(256):
        key = tuple(i for i, m in enumerate(order) if (m >> c) & 1)
        if key not in key_of:
            key_of[key] = len(reps)
            reps.append(c)
        byte_class[c] = key_of[key]
    return byte_class, reps


def _determinize(nfa: _Nfa, start: int, final: int) -> Dfa:
    byte_class, reps = _classes(nfa)
    C = len(reps)

    def closure(states) -> frozenset:
        seen = set(states)
        todo = list(states)
        while todo:
            for t in nfa.eps[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return frozenset(seen)

    ids = {closure([start]): 0}
    order = [next(iter(ids))]
    rows: List[List[int]] = []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        row = [-1] * C
        edges = [e for s in cur for e in nfa.edges[s]]
        for ci, c in enumerate(reps):
            tgt = [t for m, t in edges if (m >> c) & 1]
            if not tgt:
                continue
            nxt = closure(tgt)
            j = ids.get(nxt)
            if j is None:
                j = ids[nxt] = len(order)
                order.append(nxt)
                if len(order) > 4 * MAX_STATES:
                    raise SchemaError("$", f"the schema needs more than {MAX_STATES} DFA states")
            row[ci] = j
        rows.append(row)
    n = len(order)
    trans = np.array(rows, np.int64).reshape(n, C)
    accept = np.array([final in s for s in order], bool)
    # trim: keep the states that reach an accepting one (all are reachable by construction)
    live = accept.copy()
    pred: List[List[int]] = [[] for _ in range(n)]
    for s in range(n):
        for t in set(rows[s]):
            if t >= 0:
                pred[t].append(s)
    todo = list(np.nonzero(accept)[0])
    while todo:
        for p in pred[todo.pop()]:
            if not live[p]:
                live[p] = True
                todo.append(p)
    if not live[0]:
        raise SchemaError("$", "the schema accepts no text")
    # minimise (Moore refinement over accept + successor blocks); block -1 stands for the dead state
    block = np.where(live, accept.astype(np.int64), -1)
    tr = np.where((trans >= 0) & live[np.maximum(trans, 0)], trans, -1)
    while True:
        succ = np.where(tr >= 0, block[np.maximum(tr, 0)], -1)
        sig = np.concatenate([block[:, None], succ], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = np.where(live, new.reshape(-1), -1)
        if len(np.unique(new)) == len(np.unique(block)):
            break
        block = new
    # number the blocks: dead 0, the initial state's block 1, the rest in order of first appearance
    number = {int(block[0]): 1}
    for s in range(n):
        if live[s] and int(block[s]) not in number:
            number[int(block[s])] = len(number) + 1
    S = len(number) + 1
    if S > MAX_STATES:
        raise SchemaError("$", f"the schema needs {S} DFA states, above the cap of {MAX_STATES}")
    out = np.zeros((S, C), np.uint16)
    acc = np.zeros(S, np.uint8)
    for s in range(n):
        if not live[s]:
            continue
        k = number[int(block[s])]
        acc[k] = accept[s]
        for ci in range(C):
            t = tr[s, ci]
            out[k, ci] = number[int(block[t])] if t >= 0 else 0
    # merge the classes whose columns are equal
    _, first, inv = np.unique(out.T, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    rank = np.argsort(np.argsort(first))  # keep classes in order of first appearance
    col = rank[inv]
    merged = np.zeros((S, len(first)), np.uint16)
    merged[:, col] = out
    return Dfa(col[byte_class].astype(np.uint8), merged, acc)


def canonical(schema) -> str:
    """the cache key of a schema: its canonical JSON text (property order is part of the language)"""
    return json.dumps(schema, separators=(",", ":"), ensure_ascii=False)


def compile_schema(schema) -> Dfa:
    """Schema (a dict) -> Dfa; SchemaError names the path of what is refused."""
    if not isinstance(schema, dict):
        raise SchemaError("$", "a schema must be an object")
    b = _Builder(schema)
    start = b.nfa.new()
    final = b.value(start, schema, "$")
    return _determinize(b.nfa, start, final)


_COMPILED: "OrderedDict[str, Dfa]" = OrderedDict()
_COMPILED_LOCK = threading.Lock()
_COMPILED_MAX = 32


def compile_cached(schema) -> Dfa:
    """compile_schema through a small process-wide LRU keyed by canonical(schema): the HTTP layer compiles a
    body's schema off the event loop to answer 400s, and the scheduler's per-tier cache then finds the Dfa here
    instead of compiling it again on the worker that steps every active row.  Refusals are not kept."""
    key = canonical(schema) if isinstance(schema, dict) else None
    if key is not None:
        with _COMPILED_LOCK:
            dfa = _COMPILED.get(key)
            if dfa is not None:
                _COMPILED.move_to_end(key)
                return dfa
    dfa = compile_schema(schema)
    with _COMPILED_LOCK:
        _COMPILED[key] = dfa
        while len(_COMPILED) > _COMPILED_MAX:
            _COMPILED.popitem(last=False)
    return dfa


# ------------------------------------------------------------------------------------------------ host grammar
class SchemaState:
    """a row's DFA state (mutable, like the native JsonState)"""
    __slots__ = ("s",)

    def __init__(self, s: int):
        self.s = int(s)

    def copy(self) -> "SchemaState":
        return SchemaState(self.s)


class Vocab:
    """The vocabulary's byte strings (b"" for a control token) as the padded matrix mask() walks, shared by every
    grammar of a tier."""

    def __init__(self, tokens: Sequence[bytes], eos_ids):
        self.tokens = [bytes(t) for t in tokens]
        self.eos = sorted({int(e) for e in eos_ids})
        self.V = len(self.tokens)
        self.length = np.array([len(t) for t in self.tokens], np.int32)
        L = int(self.length.max()) if self.V else 0
        self.bytes = np.zeros((self.V, max(L, 1)), np.uint8)
        for i, t in enumerate(self.tokens):
            if t:
                self.bytes[i, :len(t)] = np.frombuffer(t, np.uint8)
        # rows still walking at byte i, longest first, so that each step touches only those
        self.rows = [np.nonzero(self.length > i)[0] for i in range(L)]


class SchemaGrammar:
    """The host grammar of one compiled schema over one vocabulary: JsonGrammar's interface (initial, mask,
    accept_token, complete).  A token is allowed when its bytes keep the DFA out of the dead state; an empty
    (control) token never is; the end-of-sequence ids are allowed exactly in accepting states."""

    def __init__(self, dfa: Dfa, vocab: Vocab):
        self.dfa = dfa
        self.vocab = vocab
        # the V x longest-token class matrix and the int32 table are built by the first mask: accept_token and
        # complete need neither, and on a tier whose device computes the masks only a row with bans asks for one
        self._cls = self._trans = None
        self._memo: Dict[int, bytes] = {}

    def initial(self) -> SchemaState:
        return SchemaState(Dfa.INITIAL)

    def accept_token(self, st: SchemaState, token: int) -> bool:
        data = self.vocab.tokens[token] if 0 <= token < self.vocab.V else b""
        s = self.dfa.step(st.s, data) if data else 0
        if s == 0:
            return False
        st.s = s
        return True

    def complete(self, st: SchemaState) -> bool:
        """nothing can follow: the row finishes without waiting for an end-of-sequence token"""
        return bool(self.dfa.terminal[st.s])

    def accepting(self, st: SchemaState) -> bool:
        return bool(self.dfa.accept[st.s])

    def allowed(self, state: int) -> np.ndarray:
        v = self.vocab
        if self._cls is None:
            self._cls = self.dfa.byte_class[v.bytes]
            self._trans = self.dfa.trans.astype(np.int32)
        s = np.full(v.V, int(state), np.int32)
        for i, rows in enumerate(v.rows):
            rows = rows[s[rows] != 0]
            if not len(rows):
                break
            s[rows] = self._trans[s[rows], self._cls[rows, i]]
        ok = (s != 0) & (v.length > 0)
        for e in v.eos:
            if 0 <= e < v.V:
                ok[e] = bool(self.dfa.accept[state])
        return ok

    def mask_of(self, state: int) -> bytes:
        m = self._memo.get(state)
        if m is None:
            m = self._memo[state] = np.packbits(self.allowed(state), bitorder="little").tobytes()
        return m

    def mask(self, st) -> bytes:
        return self.mask_of(st.s if isinstance(st, SchemaState) else int(st))

    mask_open = mask  # (schema rows ignore min_tokens)

    @property
    def memo_bytes(self) -> int:
        return sum(len(m) for m in self._memo.values())

    def token_dead_states(self) -> List[int]:
        """live, non-terminal states in which no token is allowed: no tokenizer path leads on from there"""
        d = self.dfa
        return [s for s in range(1, d.n_states) if not d.terminal[s] and not self.allowed(s).any()]


class SchemaCache:
    """A tier's compiled schemas, least recently used first, keyed by canonical(schema).  An entry holds the Dfa,
    its host grammar and -- on a tier whose engine has grammar_load -- the device grammar id; on eviction the
    device tables are freed once no active sequence uses them (release())."""

    class Entry:
        __slots__ = ("key", "dfa", "grammar", "gid", "users", "evicted")

        def __init__(self, key, dfa, grammar, gid):
            self.key, self.dfa, self.grammar, self.gid = key, dfa, grammar, gid
            self.users = 0
            self.evicted = False

    def __init__(self, vocab: Vocab, engine=None, capacity: int = 16):
        self.vocab = vocab
        self.engine = engine if hasattr(engine, "grammar_load") else None
        self.capacity = capacity
        self.entries: "OrderedDict[str, SchemaCache.Entry]" = OrderedDict()
        self.compiles = 0

    def acquire(self, schema) -> "SchemaCache.Entry":
        key = canonical(schema)
        e = self.entries.get(key)
        if e is None:
            dfa = compile_cached(schema)
            self.compiles += 1
            gid = -1
            if self.engine is not None:
                # (the engine refuses a grammar with a live state that allows no token)
                try:
                    gid = int(self.engine.grammar_load(dfa.byte_class, dfa.trans, dfa.accept))
                except RuntimeError as err:
                    raise SchemaError("$", str(err)) from None
            e = self.entries[key] = self.Entry(key, dfa, SchemaGrammar(dfa, self.vocab), gid)
            while len(self.entries) > self.capacity:
                _, old = self.entries.popitem(last=False)
                old.evicted = True
                self._free(old)
        else:
            self.entries.move_to_end(key)
        e.users += 1
        return e

    def release(self, e: "SchemaCache.Entry"):
        e.users -= 1
        self._free(e)

    def clear(self):
        """drop every entry (the tier closes): device tables without a user are freed now"""
        while self.entries:
            _, old = self.entries.popitem(last=False)
            old.evicted = True
            self._free(old)

    def _free(self, e):
        if e.evicted and e.users <= 0 and e.gid >= 0 and self.engine is not None:
            self.engine.grammar_free(e.gid)
            e.gid = -1
