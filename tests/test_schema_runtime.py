"""JSON-schema requests through the runtime on the CPU backend (the host grammar's path): with max_tokens at the
schema's longest text every request finishes "grammar" or "stop" with a text that validates, over 16 seeds at
temperature 1 on random weights; a request cut short leaves a live prefix; a schema beside a ban still validates;
the three HTTP spellings answer 200, the bad ones 400 with the path, and a plain body is served as before."""
import asyncio
import json

import numpy as np
import pytest

import schema_oracle as SO
from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab, write_synthetic_gguf
from aios_amd.runtime import chat_template, service
from aios_amd.runtime import json_schema as JS
from aios_amd.runtime.cpu_engine import CpuEngine
from aios_amd.runtime.scheduler import GenRequest, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

PROMPT = [1, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49]
V, EOS, CTX = 512, 2, 256


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    p = tmp_path_factory.mktemp("schema") / "tiny.gguf"
    write_synthetic_gguf(str(p), get_preset("test-tiny"), "Q8_0", seed=5)
    t, s, ty = synthetic_vocab(V)
    return str(p), SpmTokenizer(t, s, ty, 1, EOS)


def _engine(path):
    return CpuEngine.from_gguf(path, max_ctx=CTX, max_slots=2, max_batch=2)


def _sched(eng, tok):
    return Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=CTX)


def check_finished(name, schema, res, tok):
    assert res.finish_reason in ("grammar", "stop"), (name, res.finish_reason, res.error, res.text)
    assert SO.parse_and_validate(res.text, schema), (name, res.text)
    assert res.text == tok.decode(res.token_ids)


@pytest.mark.parametrize("name", list(SO.BOUNDED))
def test_every_request_finishes_with_a_valid_text(setup, name):
    path, tok = setup
    schema = SO.BOUNDED[name]
    longest = JS.compile_schema(schema).longest_path()
    assert longest is not None and longest + len(PROMPT) < CTX
    sched = _sched(_engine(path), tok)
    reqs = [GenRequest(prompt_ids=list(PROMPT), max_tokens=longest, temperature=1.0, top_k=0, top_p=1.0, seed=seed,
                       json_schema=schema) for seed in range(1, 17)]
    res = SO.run_requests(sched, reqs)
    for r in res:
        check_finished(name, schema, r, tok)
    assert len({r.text for r in res}) > 1                       # sixteen seeds, more than one answer
    assert sched.stats["schema_requests"] == 16 and sched.stats["schema_compiles"] == 1
    assert sorted(sched.free_slots) == [0, 1]


def test_a_request_cut_short_leaves_a_live_prefix(setup):
    path, tok = setup
    schema = SO.BOUNDED["tool_call"]
    dfa = JS.compile_schema(schema)
    res, = SO.run_requests(_sched(_engine(path), tok), [GenRequest(prompt_ids=list(PROMPT), max_tokens=4, json_schema=schema)])
    assert res.finish_reason == "length" and len(res.token_ids) == 4
    raw = b"".join(tok.token_bytes(t) for t in res.token_ids)
    assert dfa.rejects_at(raw) == len(raw)                      # a prefix of the language, not yet a member


def test_schema_rows_ignore_min_tokens_and_json_mode_rows_keep_their_grammar(setup):
    path, tok = setup

    class OneToken:
        """a tier grammar that allows one token and completes behind it"""
        def initial(self):
            return []

        def accept_token(self, st, t):
            st.append(t)
            return True

        def complete(self, st):
            return bool(st)

        def mask(self, st):
            bits = np.zeros(V, np.uint8)
            bits[77] = 1
            return np.packbits(bits, bitorder="little").tobytes()

        mask_open = mask

    sched = Scheduler(_engine(path), tok, max_batch=2, max_slots=2, max_ctx=CTX, grammar=OneToken())
    schema = SO.BOUNDED["choice"]
    a, b = SO.run_requests(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=8, json_mode=True),
                                   GenRequest(prompt_ids=list(PROMPT), max_tokens=8, min_tokens=8, json_schema=schema)])
    assert a.token_ids == [77] and a.finish_reason == "grammar"  # the tier's grammar, beside a schema row
    check_finished("choice", schema, b, tok)


def test_a_schema_beside_a_ban_takes_the_host_masks_and_validates(setup):
    path, tok = setup
    schema = SO.BOUNDED["flags"]
    plain, = SO.run_requests(_sched(_engine(path), tok), [GenRequest(prompt_ids=list(PROMPT), max_tokens=30, json_schema=schema)])
    check_finished("flags", schema, plain, tok)
    # ban the row's second token: the answer changes there and still validates; ban "[" itself, the only opening the
    # schema has: the grammar wins for that step
    second, opener = plain.token_ids[1], plain.token_ids[0]
    sched = _sched(_engine(path), tok)
    moved, forced = SO.run_requests(sched, [
        GenRequest(prompt_ids=list(PROMPT), max_tokens=30, json_schema=schema, logit_bias={second: -np.inf}),
        GenRequest(prompt_ids=list(PROMPT), max_tokens=30, json_schema=schema,
                   logit_bias={t: -np.inf for t in range(V) if tok.token_bytes(t).lstrip()[:1] == b"["})], together=False)
    check_finished("flags", schema, moved, tok)
    assert second not in moved.token_ids and moved.token_ids[0] == opener
    check_finished("flags", schema, forced, tok)
    assert sched.stats["bias_overridden"] >= 1


def test_refused_schemas_finish_with_an_error_and_free_the_slot(setup):
    path, tok = setup
    sched = _sched(_engine(path), tok)
    bad, ok = SO.run_requests(sched, [
        GenRequest(prompt_ids=list(PROMPT), max_tokens=4, json_schema={"type": "string", "pattern": "a+"}),
        GenRequest(prompt_ids=list(PROMPT), max_tokens=4, json_schema=SO.BOUNDED["choice"])], together=False)
    assert bad.finish_reason == "error" and "$.pattern" in bad.error
    assert ok.finish_reason != "error" and not sched.failed and sorted(sched.free_slots) == [0, 1]


def test_the_cache_evicts_least_recently_used(setup):
    path, tok = setup
    vocab = JS.Vocab(tok.all_token_bytes(), [EOS])

    class Eng:
        def __init__(self):
            self.loaded, self.freed = [], []

        def grammar_load(self, bc, tr, ac):
            self.loaded.append(len(self.loaded))
            return self.loaded[-1]

        def grammar_free(self, gid):
            self.freed.append(gid)

    eng = Eng()
    cache = JS.SchemaCache(vocab, eng, capacity=2)
    schemas = [{"const": i} for i in range(3)]
    a = cache.acquire(schemas[0])
    b = cache.acquire(schemas[1])
    cache.release(b)
    assert cache.acquire(schemas[0]) is a and cache.compiles == 2   # a hit: no compile, and 0 is now the newest
    cache.release(a)
    c = cache.acquire(schemas[2])                                   # evicts schema 1, which nobody uses: freed at once
    assert eng.freed == [1] and b.gid == -1 and c.gid == 2
    cache.acquire(schemas[0])                                       # (in use again, and the newest)
    d = cache.acquire(schemas[1])                                   # evicts schema 2, still in use: kept
    assert eng.freed == [1] and c.evicted and c.gid == 2
    cache.release(c)                                                # its last user leaves: freed
    assert eng.freed == [1, 2] and d.gid == 3 and cache.compiles == 4


# ---- HTTP -------------------------------------------------------------------------------------------
def _manager(path, tok):
    from aios_amd.runtime import model_manager as mm

    class Mgr(mm.ModelManager):
        def _load_blocking(self, m, context_length):
            m.engine = _engine(path)
            m.tokenizer = tok
            m.template = chat_template.for_model("zephyr", tok)
            m.grammar = None
            m.context_length = CTX
            m.scheduler = Scheduler(m.engine, tok, 2, 2, CTX, None, m.name)

    return Mgr(base_port=19030)


def _serve(path, tok, port, calls):
    import aiohttp

    from aios_amd.runtime.service import AIRuntimeService

    async def run():
        mgr = _manager(path, tok)
        svc = AIRuntimeService(mgr, http=True)
        m = await mgr.load_model("tiny", "fake.gguf", port=port)
        await svc.start_http(m)
        try:
            async with aiohttp.ClientSession() as s:
                return await calls(s, f"http://127.0.0.1:{port}")
        finally:
            await svc.close()

    return asyncio.run(run())


async def _post(s, url, body):
    async with s.post(url, data=json.dumps(body), headers={"Content-Type": "application/json"}) as r:
        return r.status, await r.json()


SCHEMA = SO.BOUNDED["tool_call"]
LONGEST = JS.compile_schema(SCHEMA).longest_path()
CHAT = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": LONGEST, "temperature": 1.0, "seed": 3}
CMPL = {"prompt": PROMPT, "max_tokens": LONGEST, "temperature": 1.0, "seed": 3}
SPELLINGS = [
    {"response_format": {"type": "json_schema", "json_schema": {"name": "call", "schema": SCHEMA, "strict": True}}},
    {"response_format": {"type": "json_object", "schema": SCHEMA}},
    {"json_schema": SCHEMA},
]
BAD = [
    ({"response_format": {"type": "json_schema"}}, "response_format.json_schema must be an object"),
    ({"response_format": {"type": "json_schema", "json_schema": {"name": "x"}}},
     "response_format.json_schema.schema must be an object"),
    ({"response_format": {"type": "json_schema", "json_schema": {"schema": {
        "type": "object", "properties": {"a": {"type": "string", "pattern": "^x"}}}}}},
     "response_format.json_schema.schema: $.properties.a.pattern"),
    ({"response_format": {"type": "json_object", "schema": {"type": "array", "items": {}}}},
     "response_format.schema: $.items"),
    ({"json_schema": {"type": "object", "properties": {"n": {"$ref": "#/$defs/n"}},
                      "$defs": {"n": {"type": "object", "properties": {"n": {"$ref": "#/$defs/n"}}}}}},
     "json_schema: $.properties.n.properties.n.$ref"),
]


def test_schema_from_body():
    f = service.schema_from_body
    assert f({}) is None and f({"response_format": {"type": "json_object"}}) is None and f({"json_schema": None}) is None
    assert f({"response_format": {"type": "text"}}) is None
    for body in SPELLINGS:
        assert f(body) == SCHEMA
    assert LONGEST is not None and LONGEST + len(PROMPT) < CTX
    for body, word in BAD:
        with pytest.raises(ValueError) as e:
            f(body)
        assert word in str(e.value)
    with pytest.raises(ValueError, match="also names"):
        f(dict(SPELLINGS[0], json_schema=SCHEMA))


def test_http_serves_the_three_spellings_and_refuses_with_the_path(setup):
    path, tok = setup

    async def calls(s, base):
        out = {"ok": [], "bad": [], "plain": []}
        for url, body in ((base + "/v1/chat/completions", CHAT), (base + "/v1/completions", CMPL)):
            for extra in SPELLINGS:
                out["ok"].append((url, await _post(s, url, dict(body, **extra))))
            for extra, word in BAD:
                out["bad"].append((url, word, await _post(s, url, dict(body, **extra))))
            plain = dict(body, max_tokens=6, temperature=0)
            out["plain"].append((await _post(s, url, plain), await _post(s, url, plain)))
        return out

    out = _serve(path, tok, 19031, calls)
    texts = []
    for url, (status, js) in out["ok"]:
        assert status == 200, (url, js)
        choice = js["choices"][0]
        text = choice["message"]["content"] if "chat" in url else choice["text"]
        assert choice["finish_reason"] == "stop" and SO.parse_and_validate(text, SCHEMA), (url, text)
        texts.append(text)
    assert texts[0] == texts[1] == texts[2] and texts[3] == texts[4] == texts[5]  # one schema, one seed, three spellings
    for url, word, (status, js) in out["bad"]:
        assert status == 400 and js["error"]["type"] == "invalid_request_error" and word in js["error"]["message"], (url, js)
    # a body without the fields gets the body it always got, spelled out here field by field; its text and counts
    # are those of a request that carries none of the new fields, run through a scheduler directly
    chat_ids = tok.encode(chat_template.for_model("zephyr", tok).render(CHAT["messages"], add_generation_prompt=True))
    want_chat, want_cmpl = SO.run_requests(_sched(_engine(path), tok), [
        GenRequest(prompt_ids=chat_ids, max_tokens=6, temperature=0.0, seed=3),
        GenRequest(prompt_ids=list(PROMPT), max_tokens=6, temperature=0.0, seed=3)], together=False)

    def usage(r, **more):
        return dict({"prompt_tokens": r.prompt_tokens, "completion_tokens": r.completion_tokens,
                     "total_tokens": r.prompt_tokens + r.completion_tokens}, **more)

    def finish(r):
        return "length" if r.finish_reason == "length" else "stop"

    golden = [
        {"object": "chat.completion", "model": "tiny",
         "choices": [{"index": 0, "message": {"role": "assistant", "content": want_chat.text},
                      "finish_reason": finish(want_chat)}],
         "usage": usage(want_chat, completion_tokens_details={"accepted_prediction_tokens": 0,
                                                              "rejected_prediction_tokens": 0})},
        {"object": "text_completion", "model": "tiny",
         "choices": [{"text": want_cmpl.text, "index": 0, "logprobs": None, "finish_reason": finish(want_cmpl)}],
         "usage": usage(want_cmpl)},
    ]
    for ((sa, a), (sb, b)), want in zip(out["plain"], golden):
        assert sa == sb == 200
        for js in (a, b):
            assert isinstance(js.pop("id"), str) and isinstance(js.pop("created"), int)
            if "chat" in js["object"]:
                assert set(js.pop("timings")) == {"ttft_ms", "latency_ms", "cached_prompt_tokens"}
            assert js == want


# ---- tiers without the device calls ---------------------------------------------------------------------
class _NoVocab:
    """an engine whose grammar_vocab refuses (a vocabulary with more end-of-sequence ids than the kernel takes)"""

    def __init__(self, eng):
        self._eng = eng
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def grammar_vocab(self, tokens, eos):
        self.calls.append("grammar_vocab")
        raise RuntimeError("grammar_vocab: more than 8 end-of-sequence ids")

    def grammar_load(self, *a):
        self.calls.append("grammar_load")
        raise AssertionError("not reached")

    def set_grammar_rows(self, *a):
        self.calls.append("set_grammar_rows")
        raise AssertionError("not reached")


def test_a_tier_whose_grammar_vocab_refuses_serves_through_host_masks(setup):
    path, tok = setup
    eng = _NoVocab(_engine(path))
    sched = _sched(eng, tok)
    assert sched.can_device_grammar
    schema = SO.BOUNDED["flags"]
    res = SO.run_requests(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=30, json_schema=schema, seed=s,
                                             temperature=1.0) for s in (1, 2)])
    for r in res:
        check_finished("flags", schema, r, tok)
    assert eng.calls == ["grammar_vocab"] and not sched.can_device_grammar and not sched.failed


def test_a_tensor_parallel_tier_serves_through_host_masks(setup):
    """TPEngine hides the grammar calls of its shard's engine (they are not broadcast to the workers): the
    scheduler sees a tier without them, sends mask bytes with decode(), and the tier stays healthy"""
    from aios_amd.parallel.tp import TPEngine

    path, tok = setup

    class Shard:
        """a shard's engine as the native one looks on such a tier: the calls exist and throw"""

        def __init__(self, eng):
            self._eng = eng

        def __getattr__(self, name):
            return getattr(self._eng, name)

        def _refuse(self, *a):
            raise RuntimeError("not available on a tensor-parallel engine")

        grammar_vocab = grammar_load = grammar_free = grammar_masks = set_grammar_rows = _refuse

    sent = []
    eng = TPEngine(Shard(_engine(path)), comm=type("Comm", (), {"error": staticmethod(lambda: False)})(),
                   send=lambda msg: sent.append(msg[0]))
    for name in ("grammar_vocab", "grammar_load", "grammar_free", "grammar_masks", "set_grammar_rows"):
        assert not hasattr(eng, name)
    sched = _sched(eng, tok)
    assert not sched.can_device_grammar
    schema = SO.BOUNDED["choice"]
    res = SO.run_requests(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=8, json_schema=schema, seed=s,
                                             temperature=1.0) for s in (1, 2, 3)])
    for r in res:
        check_finished("choice", schema, r, tok)
    assert not sched.failed and sched.stats["errors"] == 0 and "decode" in sent
