"""Prompt scoring through the runtime on the CPU backend: CpuEngine.score_prefill against the float64 oracle
(tests/score_oracle.py), the scheduler's prompt_logprobs (chunked, cached prefixes, max_tokens 0, no call for
requests that do not ask) and the OpenAI /v1/completions endpoint: body fields, response shape, SSE and 400s."""
import asyncio
import json
import math
import threading

import numpy as np
import pytest

import score_oracle as O
from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab, write_synthetic_gguf
from aios_amd.runtime import chat_template
from aios_amd.runtime.cpu_engine import CpuEngine
from aios_amd.runtime.scheduler import GenRequest, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

PROMPT = [1, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49]
TOL = 1e-5  # the engine reports float32 values of a float64 rule over the same fp32 logits


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    p = tmp_path_factory.mktemp("cmpl") / "tiny.gguf"
    write_synthetic_gguf(str(p), get_preset("test-tiny"), "Q8_0", seed=5)
    t, s, ty = synthetic_vocab(512)
    return str(p), SpmTokenizer(t, s, ty, 1, 2)


def _engine(path, **kw):
    return CpuEngine.from_gguf(path, max_ctx=128, max_slots=2, max_batch=2, **kw)


class _Spy:
    """the engine with its prefill-side calls recorded"""

    def __init__(self, eng):
        self._eng = eng
        self.score_calls = []    # (slot, n tokens, start, next_token, top_n, want_logits)
        self.prefill_calls = []  # (slot, n tokens, start)

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def score_prefill(self, slot, ids, start=0, next_token=-1, top_n=0, want_logits=False):
        self.score_calls.append((slot, len(ids), start, next_token, top_n, want_logits))
        return self._eng.score_prefill(slot, ids, start, next_token, top_n, want_logits)

    def prefill(self, slot, ids, start=0, want_logits=True):
        self.prefill_calls.append((slot, len(ids), start))
        return self._eng.prefill(slot, ids, start, want_logits)


class _Bare:
    """a tensor-parallel tier's surface: the engine without score_prefill (and without the logprob calls)"""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        if name in ("score_prefill", "set_logprobs", "last_logprobs"):
            raise AttributeError(name)
        return getattr(self._eng, name)


def _run(sched, reqs, together=True):
    evs, box = [threading.Event() for _ in reqs], {}
    try:
        for i, r in enumerate(reqs):
            r.on_done = lambda res, i=i: (box.__setitem__(i, res), evs[i].set())
        if together:
            with sched.cv:  # queued together: admitted into one batch
                for r in reqs:
                    sched.submit(r)
            for e in evs:
                assert e.wait(60)
        else:
            for r, e in zip(reqs, evs):
                sched.submit(r)
                assert e.wait(60)
    finally:
        sched.close()
    return [box[i] for i in range(len(reqs))]


def _reference(path, ids):
    """the oracle's rows for the prompt from a fresh engine's full logits"""
    eng = _engine(path)
    logits = eng.model.forward(list(ids), eng.model.new_cache()).numpy()
    return logits, O.score_rows(logits, list(ids[1:]) + [-1])


def _check_prompt_entries(res, ids, ref, top_n):
    lp, rank, _best, _best_lp = ref
    plp = res.prompt_logprobs
    assert plp is not None and len(plp) == len(ids)
    assert plp[0] == (ids[0], None, None, [])
    for i in range(1, len(ids)):
        tid, x, r, top = plp[i]
        assert tid == ids[i] and r == rank[i - 1]
        assert x == pytest.approx(lp[i - 1], abs=TOL)
        assert len(top) == top_n
        if top_n:
            vals = [v for _, v in top]
            assert vals == sorted(vals, reverse=True)
            assert (r == 0) == (top[0][0] == tid)


# ---- CpuEngine ------------------------------------------------------------------------------------------
def test_cpu_engine_score_prefill_matches_the_oracle(setup):
    path, _ = setup
    logits, (lp, rank, best, best_lp) = _reference(path, PROMPT)
    eng = _engine(path)
    sc = eng.score_prefill(0, PROMPT, 0, -1, 4, True)
    T = len(PROMPT)
    assert sc["lp"].shape == sc["rank"].shape == (T,) and sc["ids"].shape == sc["lps"].shape == (T, 4)
    assert math.isnan(sc["lp"][-1]) and sc["rank"][-1] == -1
    assert sc["lp"][:-1] == pytest.approx(lp[:-1], abs=TOL) and sc["best_lp"] == pytest.approx(best_lp, abs=TOL)
    assert sc["rank"].tolist() == rank.tolist() and sc["best"].tolist() == best.tolist()
    assert sc["ids"][:, 0].tolist() == best.tolist()
    # want_logits: the last row is what sample_first reads, as after prefill
    assert np.array_equal(eng.last[0], logits[-1])
    assert eng.sample_first(T - 1, 0.0, 0, 1.0, 1) == int(np.argmax(logits[-1]))
    # in two calls, the seam row scored through next_token
    a = eng.score_prefill(1, PROMPT[:5], 0, PROMPT[5], 0, False)
    b = eng.score_prefill(1, PROMPT[5:], 5, 7, 0, False)
    both = np.concatenate([a["lp"], b["lp"]])
    assert both[:-1] == pytest.approx(lp[:-1], abs=TOL) and np.isfinite(both[-1]) and "ids" not in a
    assert O.score(logits[-1], 7)[0] == pytest.approx(float(both[-1]), abs=TOL)
    for bad in (dict(top_n=21), dict(top_n=-1), dict(next_token=512), dict(ids=[])):
        kw = dict(dict(ids=PROMPT, next_token=-1, top_n=0), **bad)
        with pytest.raises(ValueError):
            eng.score_prefill(0, kw["ids"], 0, kw["next_token"], kw["top_n"], False)


# ---- scheduler --------------------------------------------------------------------------------------------
def test_scheduler_entries_line_up_with_the_prompt(setup):
    path, tok = setup
    eng = _Spy(_engine(path))
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128)
    r, = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=3, prompt_logprobs=3, stop_ids=[])])
    _, ref = _reference(path, PROMPT)
    _check_prompt_entries(r, PROMPT, ref, 3)
    assert r.finish_reason in ("length", "stop") and r.logprobs is None
    assert eng.score_calls == [(eng.score_calls[0][0], len(PROMPT), 0, -1, 3, True)] and eng.prefill_calls == []
    assert sched.stats["prompt_scores"] == 1
    # the same generation as without scoring
    plain, = _run(Scheduler(_engine(path), tok, max_batch=2, max_slots=2, max_ctx=128),
                  [GenRequest(prompt_ids=list(PROMPT), max_tokens=3, stop_ids=[])])
    assert plain.token_ids == r.token_ids and plain.prompt_logprobs is None


def test_chunked_prompt_equals_the_unchunked_one(setup):
    path, tok = setup
    ids = [1] + [int(t) for t in np.random.default_rng(2).integers(3, 512, 36)]
    whole, = _run(Scheduler(_engine(path), tok, max_batch=2, max_slots=2, max_ctx=128),
                  [GenRequest(prompt_ids=list(ids), max_tokens=2, prompt_logprobs=2, stop_ids=[])])
    # chunks apply while another sequence decodes: a long-running mate first, then the scored prompt
    eng = _Spy(_engine(path))
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128)
    sched.prefill_chunk = 8
    mate = GenRequest(prompt_ids=[1, 9, 10], max_tokens=60, stop_ids=[])
    started = threading.Event()
    mate.on_delta = lambda d: started.set()
    evs, box = [threading.Event(), threading.Event()], {}
    try:
        mate.on_done = lambda res: (box.__setitem__(0, res), evs[0].set())
        sched.submit(mate)
        assert started.wait(60)
        req = GenRequest(prompt_ids=list(ids), max_tokens=2, prompt_logprobs=2, stop_ids=[])
        req.on_done = lambda res: (box.__setitem__(1, res), evs[1].set())
        sched.submit(req)
        assert evs[1].wait(60) and evs[0].wait(60)
    finally:
        sched.close()
    chunked = box[1]
    calls = [c for c in eng.score_calls]
    assert len(calls) >= 2 and sum(c[1] for c in calls) == len(ids), calls  # really went through in chunks
    assert all(c[3] == ids[c[2] + c[1]] for c in calls[:-1]) and calls[-1][3] == -1  # next chunk's first token
    assert [c[5] for c in calls] == [False] * (len(calls) - 1) + [True]
    assert len(chunked.prompt_logprobs) == len(whole.prompt_logprobs) == len(ids)
    for a, b in zip(chunked.prompt_logprobs[1:], whole.prompt_logprobs[1:]):
        assert a[0] == b[0] and a[2] == b[2] and a[1] == pytest.approx(b[1], abs=1e-5)
        assert [i for i, _ in a[3]] == [i for i, _ in b[3]]
    assert chunked.token_ids == whole.token_ids


def test_cached_prefix_is_still_scored_from_position_zero(setup):
    path, tok = setup
    eng = _Spy(_engine(path))
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128)
    first, second = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=2, stop_ids=[]),
                                 GenRequest(prompt_ids=list(PROMPT), max_tokens=2, prompt_logprobs=0, stop_ids=[])],
                         together=False)
    _, ref = _reference(path, PROMPT)
    _check_prompt_entries(second, PROMPT, ref, 0)
    assert second.cached_prompt_tokens == 0 and eng.score_calls[0][1:3] == (len(PROMPT), 0)
    assert first.prompt_logprobs is None and second.token_ids == first.token_ids


def test_max_tokens_zero_only_scores(setup):
    path, tok = setup
    eng = _Spy(_engine(path))
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128)
    r, plain = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=0, prompt_logprobs=1),
                            GenRequest(prompt_ids=list(PROMPT[:5]), max_tokens=0)])
    assert r.finish_reason == "length" and r.token_ids == [] and r.completion_tokens == 0 and r.text == ""
    assert len(r.prompt_logprobs) == len(PROMPT) and eng.score_calls[0][5] is False
    assert plain.completion_tokens >= 1  # without scoring, max_tokens 0 keeps meaning "at least one"
    assert sorted(sched.free_slots) == [0, 1]


def test_request_without_the_field_makes_no_score_call(setup):
    path, tok = setup
    eng = _Spy(_engine(path))
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128)
    r, = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=3, logprobs=True, top_logprobs=2)])
    assert eng.score_calls == [] and eng.prefill_calls and r.prompt_logprobs is None
    assert sched.stats["prompt_scores"] == 0


def test_combined_with_generated_logprobs_and_bad_values(setup):
    path, tok = setup
    sched = Scheduler(_engine(path), tok, max_batch=2, max_slots=2, max_ctx=128)
    both, bad = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=3, prompt_logprobs=2, logprobs=True,
                                        top_logprobs=1, stop_ids=[]),
                             GenRequest(prompt_ids=list(PROMPT), max_tokens=3, prompt_logprobs=21)])
    assert len(both.prompt_logprobs) == len(PROMPT) and len(both.logprobs) == both.completion_tokens >= 1
    assert bad.finish_reason == "error" and "prompt_logprobs" in bad.error


def test_tier_without_score_prefill_finishes_with_an_error(setup):
    path, tok = setup
    sched = Scheduler(_Bare(_engine(path)), tok, max_batch=2, max_slots=2, max_ctx=128)
    assert not sched.can_score
    bad, ok = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=3, prompt_logprobs=2),
                           GenRequest(prompt_ids=list(PROMPT), max_tokens=3)])
    assert bad.finish_reason == "error" and "score" in bad.error and bad.prompt_logprobs is None
    assert ok.finish_reason != "error" and ok.completion_tokens >= 1 and not sched.failed


def test_tensor_parallel_engine_hides_the_call(setup):
    from aios_amd.parallel.tp import TPEngine

    path, _ = setup
    shard = _engine(path)
    assert hasattr(shard, "score_prefill")
    eng = TPEngine(shard, comm=type("Comm", (), {"error": staticmethod(lambda: False)})(), send=lambda msg: None)
    assert not hasattr(eng, "score_prefill")


# ---- HTTP -------------------------------------------------------------------------------------------
def _manager(path, tok, bare=False):
    from aios_amd.runtime import model_manager as mm

    class Mgr(mm.ModelManager):
        def _load_blocking(self, m, context_length):
            m.engine = _Bare(_engine(path)) if bare else _engine(path)
            m.tokenizer = tok
            m.template = chat_template.for_model("zephyr", tok)
            m.grammar = None
            m.context_length = 128
            m.scheduler = Scheduler(m.engine, tok, 2, 2, 128, None, m.name)

    return Mgr(base_port=18960)


def _serve(path, tok, port, calls, bare=False):
    """start the endpoint of one model, run `calls(session, base url)`, tear down"""
    import aiohttp

    from aios_amd.runtime.service import AIRuntimeService

    async def run():
        mgr = _manager(path, tok, bare)
        svc = AIRuntimeService(mgr, http=True)
        m = await mgr.load_model("tiny", "fake.gguf", port=port)
        await svc.start_http(m)
        try:
            async with aiohttp.ClientSession() as s:
                return await calls(s, f"http://127.0.0.1:{port}")
        finally:
            await svc.close()

    return asyncio.run(run())


TEXT = "w10 w11 w12 w13"


def _prompt_text(tok):
    """a prompt string made of the synthetic vocabulary's own pieces"""
    ids = [i for i in range(20, 40) if tok.token_bytes(i).decode("utf-8", errors="replace").strip()][:5]
    return tok.decode(ids) or TEXT


def test_http_plain_completion_and_echo_logprobs(setup):
    path, tok = setup
    text = _prompt_text(tok)
    n_prompt = len(tok.encode(text, add_bos=True, parse_special=False))

    async def calls(s, base):
        url = base + "/v1/completions"
        async with s.post(url, json={"prompt": text, "max_tokens": 3, "temperature": 0}) as r:
            assert r.status == 200
            plain = await r.json()
        body = {"prompt": text, "max_tokens": 3, "temperature": 0, "echo": True, "logprobs": 2}
        async with s.post(url, json=body) as r:
            assert r.status == 200
            echo = await r.json()
        async with s.post(url, json=dict(body, max_tokens=0)) as r:
            assert r.status == 200
            score = await r.json()
        async with s.post(url, json={"prompt": text, "max_tokens": 3, "temperature": 0, "logprobs": 0}) as r:
            assert r.status == 200
            gen_only = await r.json()
        ids = tok.encode(text, add_bos=True, parse_special=False)
        async with s.post(url, json={"prompt": ids, "max_tokens": 3, "temperature": 0}) as r:
            assert r.status == 200
            from_ids = await r.json()
        return plain, echo, score, gen_only, from_ids

    plain, echo, score, gen_only, from_ids = _serve(path, tok, 18961, calls)
    c = plain["choices"][0]
    assert plain["object"] == "text_completion" and set(c) == {"text", "index", "logprobs", "finish_reason"}
    assert c["logprobs"] is None and c["index"] == 0 and c["finish_reason"] in ("length", "stop")
    n_gen = plain["usage"]["completion_tokens"]
    assert plain["usage"] == {"prompt_tokens": n_prompt, "completion_tokens": n_gen, "total_tokens": n_prompt + n_gen}
    assert 1 <= n_gen <= 3
    assert from_ids["choices"][0]["text"] == c["text"]  # the same tokens, given as ids

    e = echo["choices"][0]
    assert e["text"].startswith(text) and e["text"][len(text):] == c["text"]
    lp = e["logprobs"]
    n = n_prompt + echo["usage"]["completion_tokens"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == len(lp["text_offset"]) == n
    assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    assert all(isinstance(x, float) and x <= 0.0 for x in lp["token_logprobs"][1:])
    assert all(isinstance(d, dict) and 1 <= len(d) <= 2 for d in lp["top_logprobs"][1:])
    assert lp["text_offset"] == sorted(lp["text_offset"]) and lp["text_offset"][0] == 0
    for t, x, d in zip(lp["tokens"][1:], lp["token_logprobs"][1:], lp["top_logprobs"][1:]):
        if t in d:  # the token among its alternatives: the same number
            assert d[t] == pytest.approx(x, abs=1e-6)
        else:
            assert x <= min(d.values()) + 1e-6

    sc = score["choices"][0]
    assert sc["text"] == text and sc["finish_reason"] == "length" and score["usage"]["completion_tokens"] == 0
    assert len(sc["logprobs"]["tokens"]) == n_prompt and sc["logprobs"]["token_logprobs"][0] is None
    assert sc["logprobs"]["token_logprobs"][1:] == pytest.approx(lp["token_logprobs"][1:n_prompt], abs=1e-6)

    g = gen_only["choices"][0]
    assert g["text"] == c["text"] and len(g["logprobs"]["tokens"]) == gen_only["usage"]["completion_tokens"]
    assert all(d == {} for d in g["logprobs"]["top_logprobs"]) and None not in g["logprobs"]["token_logprobs"]


def test_http_streams_a_plain_completion(setup):
    path, tok = setup
    text = _prompt_text(tok)

    async def calls(s, base):
        url = base + "/v1/completions"
        async with s.post(url, json={"prompt": text, "max_tokens": 4, "temperature": 0}) as r:
            whole = (await r.json())["choices"][0]["text"]
        async with s.post(url, json={"prompt": text, "max_tokens": 4, "temperature": 0, "stream": True}) as r:
            assert r.status == 200 and r.headers["Content-Type"].startswith("text/event-stream")
            raw = (await r.read()).decode()
        return whole, raw

    whole, raw = _serve(path, tok, 18962, calls)
    events = [ln[6:] for ln in raw.split("\n") if ln.startswith("data: ")]
    assert events[-1] == "[DONE]"
    chunks = [json.loads(e) for e in events[:-1]]
    assert all(c["object"] == "text_completion" for c in chunks)
    assert "".join(c["choices"][0]["text"] for c in chunks) == whole
    assert chunks[-1]["choices"][0]["finish_reason"] in ("length", "stop")
    assert all(c["choices"][0]["finish_reason"] is None for c in chunks[:-1])


def test_http_rejects_what_it_cannot_serve(setup):
    path, tok = setup
    long_prompt = [1] + [5] * 200  # over the 128-token window

    async def calls(s, base):
        out = []
        for body in ({"prompt": ["a", "b"]}, {"prompt": [[1, 2], [3]]}, {"prompt": "w1", "n": 2},
                     {"prompt": "w1", "best_of": 2}, {"prompt": "w1", "suffix": "x"}, {"prompt": "w1", "logprobs": 21},
                     {"prompt": "w1", "logprobs": True}, {"prompt": "w1", "logprobs": 1, "stream": True},
                     {"prompt": ""}, {"prompt": []}, {}, {"prompt": long_prompt}, {"prompt": [1, 99999]},
                     {"prompt": "w1", "max_tokens": 0}, {"prompt": "w1", "max_tokens": -1}):
            async with s.post(base + "/v1/completions", json=body) as r:
                out.append((body, r.status, await r.json()))
        return out

    for body, status, js in _serve(path, tok, 18963, calls):
        assert status == 400 and js["error"]["type"] == "invalid_request_error", body


def test_http_tier_without_scoring(setup):
    path, tok = setup

    async def calls(s, base):
        url = base + "/v1/completions"
        out = []
        for body in ({"prompt": "w1 w2", "max_tokens": 2, "echo": True, "logprobs": 1},
                     {"prompt": "w1 w2", "max_tokens": 2, "logprobs": 1},
                     {"prompt": "w1 w2", "max_tokens": 2, "echo": True}):
            async with s.post(url, json=body) as r:
                out.append((r.status, await r.json()))
        return out

    echo_lp, gen_lp, plain = _serve(path, tok, 18964, calls, bare=True)
    assert echo_lp[0] == 400 and gen_lp[0] == 400
    assert plain[0] == 200 and plain[1]["choices"][0]["text"].startswith("w1 w2")  # works on every tier


def test_chat_endpoint_is_unchanged(setup):
    path, tok = setup

    async def calls(s, base):
        body = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 4, "temperature": 0}
        async with s.post(base + "/v1/chat/completions", json=body) as r:
            assert r.status == 200
            return await r.json()

    js = _serve(path, tok, 18965, calls)
    assert set(js) == {"id", "object", "created", "model", "choices", "usage", "timings"}
    assert js["object"] == "chat.completion" and set(js["choices"][0]) == {"index", "message", "finish_reason"}
    # the text a scheduler produces for the same templated prompt without the endpoint
    sched = Scheduler(_engine(path), tok, 2, 2, 128)
    ids = tok.encode(chat_template.for_model("zephyr", tok).render(body_messages(), add_generation_prompt=True))
    ref, = _run(sched, [GenRequest(prompt_ids=ids, max_tokens=4, temperature=0.0)])
    assert js["choices"][0]["message"]["content"] == ref.text
    assert js["usage"]["prompt_tokens"] == len(ids)


def body_messages():
    return [{"role": "user", "content": "hi"}]


def test_colliding_token_texts_keep_the_better_logprob(setup):
    from aios_amd.runtime import service

    _, tok = setup

    class Twins:
        def token_bytes(self, i):
            return b"same" if i in (5, 6) else tok.token_bytes(i)

    lp = service.completion_logprobs(Twins(), [(7, None, []), (5, -0.5, [(6, -0.25), (5, -0.5), (8, float("-inf"))])])
    assert lp["token_logprobs"] == [None, -0.5] and lp["top_logprobs"][0] is None
    assert lp["top_logprobs"][1]["same"] == -0.25 and -9999.0 in lp["top_logprobs"][1].values()
    assert lp["text_offset"] == [0, len(tok.token_bytes(7).decode("utf-8", errors="replace"))]
