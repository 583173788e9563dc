"""Text embeddings through the runtime on the CPU backend and a fake engine: CpuEngine.embed_prefill against
the float64 oracle, the scheduler's embedding requests (chunked between decode steps, slot and cache
afterwards, chat requests untouched), and /v1/embeddings' body forms, response shape and 400s."""
import asyncio
import base64
import threading

import numpy as np
import pytest

import embed_oracle as O
from aios_amd.models.config import ModelConfig, get_preset
from aios_amd.models.synthetic import synthetic_vocab, write_synthetic_gguf
from aios_amd.runtime import chat_template
from aios_amd.runtime.cpu_engine import CpuEngine
from aios_amd.runtime.scheduler import GenRequest, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

PROMPT = [1, 40, 41, 42, 43, 44, 45]
CTX = 128


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    p = tmp_path_factory.mktemp("emb") / "tiny.gguf"
    write_synthetic_gguf(str(p), get_preset("test-tiny"), "Q8_0", seed=5)
    t, s, ty = synthetic_vocab(512)
    return str(p), SpmTokenizer(t, s, ty, 1, 2)


def _engine(path):
    return CpuEngine.from_gguf(path, max_ctx=CTX, max_slots=2, max_batch=2)


def _run(sched, reqs, close=True):
    evs, box = [threading.Event() for _ in reqs], {}
    try:
        with sched.cv:
            for i, r in enumerate(reqs):
                r.on_done = lambda res, i=i: (box.__setitem__(i, res), evs[i].set())
                sched.submit(r)
        for e in evs:
            assert e.wait(60)
    finally:
        if close:
            sched.close()
    return [box[i] for i in range(len(reqs))]


def _oracle(eng, ids, pooling):
    x = eng.model.hidden(list(ids)).double().numpy()
    return O.embed(x, eng.model.w["output_norm.weight"].double().numpy(), eng.cfg.norm_eps, pooling)


# ---- CpuEngine ------------------------------------------------------------------------------------------
def test_cpu_engine_follows_the_rule_and_the_call_contract(setup):
    path, _ = setup
    eng = _engine(path)
    for pooling, code in (("mean", 1), ("last", 3), ("none", 0)):
        got = eng.embed_prefill(0, PROMPT, 0, code, True)
        assert np.asarray(got, np.float64) == pytest.approx(_oracle(eng, PROMPT, pooling), abs=1e-6)
        assert eng.embed_tokens() == len(PROMPT)
    # chunks: nothing until final, then the single call's vector
    assert len(eng.embed_prefill(1, PROMPT[:3], 0, 1, False)) == 0
    with pytest.raises(ValueError, match="start_pos"):
        eng.embed_prefill(1, PROMPT[4:], 4, 1, True)          # a chunk skipped
    two = eng.embed_prefill(1, PROMPT[3:], 3, 1, True)
    assert np.asarray(two, np.float64) == pytest.approx(_oracle(eng, PROMPT, "mean"), abs=1e-6)
    # start 0 resets
    eng.embed_prefill(1, PROMPT[:2], 0, 1, False)
    again = eng.embed_prefill(1, PROMPT, 0, 1, True)
    assert np.asarray(again, np.float64) == pytest.approx(_oracle(eng, PROMPT, "mean"), abs=1e-6)
    with pytest.raises(ValueError):
        eng.embed_prefill(0, PROMPT, 0, 2, True)              # cls pooling is not served
    # the slot decodes afterwards as after a prefill
    a = eng.decode([1], [50], [len(PROMPT)], [0.0], [0], 0)
    eng.prefill(0, PROMPT, 0, True)
    assert eng.decode([0], [50], [len(PROMPT)], [0.0], [0], 0) == a


# ---- scheduler, on a fake engine that records its calls ---------------------------------------------------
class FakeEngine:
    """prefill / embed_prefill / decode with a call log; tokens are a counter, embeddings a constant"""

    def __init__(self, vocab=512, embed=True):
        self.log, self.vocab, self._embed = [], vocab, embed

    def __getattr__(self, name):
        if name == "embed_prefill" and self._embed:
            return self._embed_prefill
        raise AttributeError(name)

    def prefill(self, slot, ids, start=0, want_logits=True):
        self.log.append(("prefill", slot, len(ids), start, bool(want_logits)))
        l = np.zeros(self.vocab, np.float32)
        l[7] = 1.0
        return l

    def _embed_prefill(self, slot, ids, start, pooling, final):
        self.log.append(("embed_prefill", slot, len(ids), start, pooling, bool(final)))
        return np.full(8, 0.5, np.float32) if final else np.zeros(0, np.float32)

    def decode(self, slots, toks, pos, temps, topk, seed, mask=b"", top_p=None, seeds=None):
        self.log.append(("decode", tuple(slots), tuple(pos)))
        return [7 + (p % 5) for p in pos]


def test_long_embedding_request_is_chunked_between_decode_steps(setup):
    _, tok = setup
    eng = FakeEngine()
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=4096)
    assert sched.can_embed and sched.prefill_chunk == 512
    ids = [1] + [3 + (i % 400) for i in range(1299)]
    # queued together, the chat request first: it is decoding when the embedding request is admitted
    chat, res = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=50, stop_ids=[]),
                             GenRequest(prompt_ids=ids, embed="mean", max_tokens=9, json_mode=True, logprobs=True,
                                        top_logprobs=3)])
    assert chat.finish_reason == "length" and chat.completion_tokens == 50
    assert res.finish_reason == "embedding" and res.prompt_tokens == 1300 and res.completion_tokens == 0
    assert res.embedding.shape == (8,) and res.logprobs is None and res.text == ""
    calls = [c for c in eng.log if c[0] == "embed_prefill"]
    assert [(c[2], c[3], c[5]) for c in calls] == [(512, 0, False), (512, 512, False), (276, 1024, True)]
    assert all(c[4] == 1 for c in calls) and len({c[1] for c in calls}) == 1
    slot = calls[0][1]
    at = [i for i, c in enumerate(eng.log) if c[0] == "embed_prefill"]
    for a, b in zip(at, at[1:]):  # decode steps of the other sequence run between the chunks
        assert any(c[0] == "decode" for c in eng.log[a + 1:b])
    assert slot in sched.free_slots and sched.slot_cache[slot] == ids
    assert sched.stats["embeddings"] == 1 and sched.stats["prefill_tokens"] >= 1300 + len(PROMPT)


def test_one_none_prompt_at_a_time(setup):
    """The engine stages "none" rows in one buffer for all slots.  A second "none" request that arrives while
    a first is mid-prefill (and the decoding sequence that made it chunk has ended, so the second would be
    prefilled whole at admission) waits until the first is through."""
    _, tok = setup
    box, evs = {}, {k: threading.Event() for k in "AB"}
    short = [1, 9, 10, 11]

    class Eng(FakeEngine):
        def _embed_prefill(self, slot, ids, start, pooling, final):
            if len(self.log) and not any(c[0] == "embed_prefill" for c in self.log):  # A's first chunk: B arrives
                sched.submit(GenRequest(prompt_ids=short, embed="none",
                                        on_done=lambda r: (box.__setitem__("B", r), evs["B"].set())))
            return super()._embed_prefill(slot, ids, start, pooling, final)

    eng = Eng()
    sched = Scheduler(eng, tok, max_batch=3, max_slots=3, max_ctx=4096)
    ids = [1] + [3 + (i % 400) for i in range(1299)]
    try:
        with sched.cv:  # the chat request decodes one step beside A's first chunk, then ends
            sched.submit(GenRequest(prompt_ids=list(PROMPT), max_tokens=2, stop_ids=[]))
            sched.submit(GenRequest(prompt_ids=ids, embed="none",
                                    on_done=lambda r: (box.__setitem__("A", r), evs["A"].set())))
        assert evs["A"].wait(60) and evs["B"].wait(60)
    finally:
        sched.close()
    assert box["A"].finish_reason == box["B"].finish_reason == "embedding"
    calls = [(c[2], c[3], c[5]) for c in eng.log if c[0] == "embed_prefill"]
    assert calls == [(512, 0, False), (788, 512, True), (len(short), 0, True)]


def test_chat_after_mean_request_reuses_the_prefix_and_last_reuses_a_cached_one(setup):
    path, tok = setup
    eng = _engine(path)
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=CTX)
    text = list(PROMPT) + [60, 61, 62]
    e1, = _run(sched, [GenRequest(prompt_ids=text, embed="mean")], close=False)
    assert e1.finish_reason == "embedding" and e1.cached_prompt_tokens == 0
    assert np.asarray(e1.embedding, np.float64) == pytest.approx(_oracle(eng, text, "mean"), abs=1e-6)
    chat, = _run(sched, [GenRequest(prompt_ids=text + [70, 71], max_tokens=2, stop_ids=[])], close=False)
    assert chat.cached_prompt_tokens == len(text) and chat.finish_reason in ("length", "stop")
    # "mean" again: from position 0 (cached positions have no hidden rows); "last": the cached prefix serves
    e2, = _run(sched, [GenRequest(prompt_ids=text, embed="mean")], close=False)
    assert e2.cached_prompt_tokens == 0
    assert np.asarray(e2.embedding, np.float64) == pytest.approx(np.asarray(e1.embedding, np.float64), abs=1e-6)
    e3, = _run(sched, [GenRequest(prompt_ids=text + [80], embed="last")], close=False)
    assert e3.cached_prompt_tokens == len(text)
    assert np.asarray(e3.embedding, np.float64) == pytest.approx(_oracle(eng, text + [80], "last"), abs=1e-5)
    # the whole window may be prompt: no token is generated
    full, over = _run(sched, [GenRequest(prompt_ids=[1] + [5] * (CTX - 1), embed="mean"),
                              GenRequest(prompt_ids=[1] + [5] * CTX, embed="mean")])
    assert full.finish_reason == "embedding" and over.finish_reason == "error" and "context window" in over.error


def test_chat_requests_make_the_engine_calls_they_made_before(setup):
    _, tok = setup

    def log_of(**kw):
        eng = FakeEngine()
        sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=CTX)
        r, = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=5, stop_ids=[], **kw)])
        assert r.finish_reason == "length" and r.embedding is None
        return eng.log

    base = log_of()
    assert base[0] == ("prefill", base[0][1], len(PROMPT), 0, True) and not any(c[0] == "embed_prefill" for c in base)
    assert log_of(embed=None) == base
    # ... and on an engine that cannot embed at all
    eng = FakeEngine(embed=False)
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=CTX)
    assert not sched.can_embed
    bad, ok = _run(sched, [GenRequest(prompt_ids=list(PROMPT), embed="mean"),
                           GenRequest(prompt_ids=list(PROMPT), max_tokens=5, stop_ids=[])])
    assert bad.finish_reason == "error" and "embeddings" in bad.error and bad.embedding is None
    assert ok.finish_reason == "length" and eng.log == base


def test_unknown_pooling_and_empty_input_are_request_errors(setup):
    _, tok = setup
    sched = Scheduler(FakeEngine(), tok, max_batch=2, max_slots=2, max_ctx=CTX)
    a, b = _run(sched, [GenRequest(prompt_ids=list(PROMPT), embed="cls"), GenRequest(prompt_ids=[], embed="mean")])
    assert a.finish_reason == b.finish_reason == "error" and not sched.failed
    assert sorted(sched.free_slots) == [0, 1]


def test_tensor_parallel_engine_hides_the_call(setup):
    from aios_amd.parallel.tp import TPEngine

    path, tok = setup
    shard = _engine(path)
    assert hasattr(shard, "embed_prefill")
    eng = TPEngine(shard, comm=type("Comm", (), {"error": staticmethod(lambda: False)})(), send=lambda msg: None)
    assert not hasattr(eng, "embed_prefill") and not hasattr(eng, "embed_tokens")
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=CTX)
    bad, = _run(sched, [GenRequest(prompt_ids=list(PROMPT), embed="mean")])
    assert bad.finish_reason == "error" and not sched.failed


def test_pooling_type_is_read_from_the_gguf():
    class Reader:
        architecture, tensors = "llama", {}

        def __init__(self, pooling):
            self.kv = {"embedding_length": 256, "attention.head_count": 4, "block_count": 2, "feed_forward_length": 512}
            if pooling is not None:
                self.kv["pooling_type"] = pooling

        def arch_get(self, k, default=None):
            return self.kv.get(k, default)

        def get(self, k, default=None):
            return default

    assert ModelConfig.from_gguf(Reader(None)).pooling == "mean" and ModelConfig("x").pooling == "mean"
    assert ModelConfig.from_gguf(Reader(3)).pooling == "last" and ModelConfig.from_gguf(Reader(1)).pooling == "mean"
    assert ModelConfig.from_gguf(Reader(2)).pooling == "mean"  # cls is not served: the default


# ---- HTTP -------------------------------------------------------------------------------------------------
def _serve(path, tok, port, calls, engine=None, pooling=None):
    import aiohttp

    from aios_amd.runtime import model_manager as mm
    from aios_amd.runtime.service import AIRuntimeService

    class Mgr(mm.ModelManager):
        def _load_blocking(self, m, context_length):
            m.engine = engine if engine is not None else _engine(path)
            m.tokenizer = tok
            m.template = chat_template.for_model("zephyr", tok)
            m.grammar = None
            m.context_length = CTX
            if pooling is not None:
                m.config = get_preset("test-tiny").scaled(pooling=pooling)
            m.scheduler = Scheduler(m.engine, tok, 2, 2, CTX, None, m.name)

    async def run():
        mgr = Mgr(base_port=18960)
        svc = AIRuntimeService(mgr, http=True)
        m = await mgr.load_model("tiny", "fake.gguf", port=port)
        await svc.start_http(m)
        try:
            async with aiohttp.ClientSession() as s:
                return await calls(s, f"http://127.0.0.1:{port}/v1/embeddings", m)
        finally:
            await svc.close()

    return asyncio.run(run())


async def _post(s, url, body):
    async with s.post(url, json=body) as r:
        return r.status, await r.json()


def test_http_input_forms_order_usage_and_base64(setup):
    path, tok = setup
    texts = ["the agent checked the memory", "status", "a third and rather longer input about the system"]

    async def calls(s, url, m):
        out = {"eng": m.engine}
        out["str"] = await _post(s, url, {"input": texts[0], "model": "whatever"})
        out["strs"] = await _post(s, url, {"input": texts})
        out["ids"] = await _post(s, url, {"input": PROMPT})
        out["idss"] = await _post(s, url, {"input": [PROMPT, PROMPT[:3]], "pooling": "last"})
        out["b64"] = await _post(s, url, {"input": texts, "encoding_format": "base64"})
        return out

    out = _serve(path, tok, 18961, calls)
    eng = out["eng"]
    for k in ("str", "strs", "ids", "idss", "b64"):
        status, js = out[k]
        assert status == 200 and js["object"] == "list" and js["model"] == "tiny"
        assert [d["index"] for d in js["data"]] == list(range(len(js["data"])))
        assert all(d["object"] == "embedding" for d in js["data"])
    ids = [tok.encode(t, add_bos=True, parse_special=False) for t in texts]
    assert all(i[0] == 1 for i in ids)
    js = out["strs"][1]
    assert js["usage"] == {"prompt_tokens": sum(map(len, ids)), "total_tokens": sum(map(len, ids))}
    for d, i in zip(js["data"], ids):  # in input order, each the oracle's vector of its own tokens
        v = np.asarray(d["embedding"], np.float64)
        assert v.shape == (256,) and abs(np.linalg.norm(v) - 1) < 1e-5
        assert v == pytest.approx(_oracle(eng, i, "mean"), abs=1e-6)
    assert out["str"][1]["data"][0]["embedding"] == js["data"][0]["embedding"] and len(out["str"][1]["data"]) == 1
    assert np.asarray(out["ids"][1]["data"][0]["embedding"]) == pytest.approx(_oracle(eng, PROMPT, "mean"), abs=1e-6)
    assert out["ids"][1]["usage"]["prompt_tokens"] == len(PROMPT)
    two = out["idss"][1]["data"]
    assert np.asarray(two[0]["embedding"]) == pytest.approx(_oracle(eng, PROMPT, "last"), abs=1e-5)
    assert np.asarray(two[1]["embedding"]) == pytest.approx(_oracle(eng, PROMPT[:3], "last"), abs=1e-5)
    for d, f in zip(out["b64"][1]["data"], js["data"]):
        raw = base64.b64decode(d["embedding"])
        assert np.frombuffer(raw, "<f4").tolist() == np.asarray(f["embedding"], np.float32).tolist()


def test_http_pooling_default_comes_from_the_model_config(setup):
    path, tok = setup

    async def calls(s, url, m):
        return m.engine, await _post(s, url, {"input": PROMPT}), await _post(s, url, {"input": PROMPT, "pooling": "mean"})

    eng, (s1, dflt), (s2, mean) = _serve(path, tok, 18962, calls, pooling="last")
    assert s1 == s2 == 200
    assert np.asarray(dflt["data"][0]["embedding"]) == pytest.approx(_oracle(eng, PROMPT, "last"), abs=1e-5)
    assert np.asarray(mean["data"][0]["embedding"]) == pytest.approx(_oracle(eng, PROMPT, "mean"), abs=1e-6)


def test_http_400s(setup):
    path, tok = setup

    async def calls(s, url, m):
        bodies = [{"input": "x", "dimensions": 64}, {"input": ""}, {"input": []}, {"input": ["ok", ""]}, {"input": [[]]},
                  {"input": ["x"] * 65}, {"input": [1] + [5] * CTX}, {"input": "x", "pooling": "none"},
                  {"input": "x", "pooling": "cls"}, {"input": "x", "encoding_format": "hex"}, {"input": 5}, {},
                  {"input": [1, "a"]}, {"input": [True, 2]}, {"input": [1, 99999]}, {"input": {"a": 1}}]
        out = [await _post(s, url, b) for b in bodies]
        ok = await _post(s, url, {"input": ["x"] * 64})
        full = await _post(s, url, {"input": [1] + [5] * (CTX - 1)})
        return out, ok, full

    out, ok, full = _serve(path, tok, 18963, calls)
    for status, js in out:
        assert status == 400 and js["error"]["type"] == "invalid_request_error" and js["error"]["message"]
    assert ok[0] == 200 and len(ok[1]["data"]) == 64
    assert full[0] == 200 and full[1]["usage"]["prompt_tokens"] == CTX


def test_http_400_on_a_tier_without_embed_prefill(setup):
    path, tok = setup

    class Bare:
        def __init__(self, eng):
            self._eng = eng

        def __getattr__(self, name):
            if name in ("embed_prefill", "embed_tokens"):
                raise AttributeError(name)
            return getattr(self._eng, name)

    async def calls(s, url, m):
        bad = await _post(s, url, {"input": "x"})
        async with s.post(url.replace("embeddings", "chat/completions"),
                          json={"messages": [{"role": "user", "content": "hi"}], "max_tokens": 2}) as r:
            return bad, r.status

    (status, js), chat = _serve(path, tok, 18964, calls, engine=Bare(_engine(path)))
    assert status == 400 and js["error"]["type"] == "invalid_request_error" and chat == 200
