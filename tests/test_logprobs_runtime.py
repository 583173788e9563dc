"""Per-token logprobs through the runtime on the CPU backend: CpuEngine's one-shot staging, the scheduler's
collection (GenResult.logprobs aligned with token_ids), and the OpenAI endpoint's body fields, response
shape and 400s.  The reference is the float64 oracle (tests/logprob_oracle.py) applied to the logits the
engine produced at each step."""
import asyncio
import threading

import numpy as np
import pytest

import logprob_oracle as O
from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab, write_synthetic_gguf
from aios_amd.runtime import chat_template
from aios_amd.runtime.cpu_engine import CpuEngine
from aios_amd.runtime.scheduler import GenRequest, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

PROMPT = [1, 40, 41, 42, 43, 44]
TOL = 1e-9  # both sides are float64 over the same fp32 logits; they differ in the order of one sum


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    p = tmp_path_factory.mktemp("lp") / "tiny.gguf"
    write_synthetic_gguf(str(p), get_preset("test-tiny"), "Q8_0", seed=5)
    t, s, ty = synthetic_vocab(512)
    return str(p), SpmTokenizer(t, s, ty, 1, 2)


def _engine(path, **kw):
    return CpuEngine.from_gguf(path, max_ctx=128, max_slots=2, max_batch=2, **kw)


class _Bare:
    """a tensor-parallel tier's surface: the engine without set_logprobs / last_logprobs"""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        if name in ("set_logprobs", "last_logprobs"):
            raise AttributeError(name)
        return getattr(self._eng, name)


class _Spy:
    """the engine with every sampler call's raw logits rows recorded, in order"""

    def __init__(self, eng):
        self._eng = eng
        self.rows = {}     # slot -> [logits row per sampled token]
        self.prompt = {}   # slot -> prompt length
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def set_logprobs(self, top_n):
        self.calls.append(list(top_n))
        return self._eng.set_logprobs(top_n)

    def prefill(self, slot, ids, start=0, want_logits=True):
        self._slot = slot
        self.prompt[slot] = start + len(ids)
        return self._eng.prefill(slot, ids, start, want_logits)

    def sample_first(self, *a):
        tok = self._eng.sample_first(*a)
        self.rows.setdefault(self._slot, []).append(np.array(self._eng.last[0]))
        return tok

    def decode(self, slots, *a):
        out = self._eng.decode(slots, *a)
        for b, s in enumerate(slots):
            self.rows.setdefault(s, []).append(np.array(self._eng.last[b]))
        return out


def _run(sched, reqs):
    evs, box = [threading.Event() for _ in reqs], {}
    try:
        with sched.cv:  # queued together: admitted into one batch
            for i, r in enumerate(reqs):
                r.on_done = lambda res, i=i: (box.__setitem__(i, res), evs[i].set())
                sched.submit(r)
        for e in evs:
            assert e.wait(60)
    finally:
        sched.close()
    return [box[i] for i in range(len(reqs))]


def _check_entries(res, rows, top_n):
    assert res.logprobs is not None and len(res.logprobs) == len(res.token_ids) == res.completion_tokens
    for k, (tid, lp, top) in enumerate(res.logprobs):
        assert tid == res.token_ids[k]
        x, ids, lps = O.logprobs(rows[k], tid, top_n)
        assert lp == pytest.approx(x, abs=TOL)
        assert [i for i, _ in top] == list(ids)
        assert [v for _, v in top] == pytest.approx(list(lps), abs=TOL)


def test_scheduler_collects_one_entry_per_token(setup):
    path, tok = setup
    eng = _Spy(_engine(path))
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128)
    a, b = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=6, logprobs=True, top_logprobs=5, stop_ids=[]),
                        GenRequest(prompt_ids=list(PROMPT[:4]), max_tokens=6)])
    assert a.finish_reason in ("length", "stop") and a.completion_tokens >= 1
    slot = next(s for s, n in eng.prompt.items() if n == len(PROMPT))
    _check_entries(a, eng.rows[slot], 5)
    assert b.logprobs is None
    # staged once per sampler launch the request took part in; its batch mate's row is off
    assert eng.calls and all(max(c) == 5 and set(c) <= {5, -1} for c in eng.calls)


def test_sampled_request_and_top_zero(setup):
    path, tok = setup
    eng = _Spy(_engine(path))
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128)
    r, = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=5, temperature=0.9, top_k=0, top_p=1.0, seed=3,
                                 logprobs=True, top_logprobs=0, repeat_penalty=1.3)])
    # the logprobs are those of the raw row, whatever the penalties did to the sampler's
    slot = next(iter(eng.rows))
    _check_entries(r, eng.rows[slot], 0)
    assert all(top == [] for _, _, top in r.logprobs)


def test_neutral_request_makes_no_call(setup):
    path, tok = setup
    eng = _Spy(_engine(path))
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128)
    r, = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=4)])
    assert r.logprobs is None and eng.calls == []


def test_cpu_engine_logprobs_are_one_shot(setup):
    path, _ = setup
    eng = _engine(path)
    eng.prefill(0, PROMPT, 0, True)
    eng.set_logprobs([3])
    t = eng.sample_first(len(PROMPT) - 1, 0.0, 0, 1.0, 1)
    lp, ids, lps = eng.last_logprobs()
    x, oid, olp = O.logprobs(eng.last[0], t, 3)
    assert lp[0] == pytest.approx(x, abs=TOL) and ids[0, :3].tolist() == list(oid) and ids[0, 3:].tolist() == [-1] * 17
    assert lps[0, :3] == pytest.approx(list(olp), abs=TOL) and np.all(np.isneginf(lps[0, 3:]))
    eng.decode([0], [t], [len(PROMPT)], [0.0], [0], 0)
    assert len(eng.last_logprobs()) == 0               # nothing staged: nothing reported
    eng.set_logprobs([1, 1])
    with pytest.raises(ValueError):                    # staged for another batch size
        eng.decode([0], [t], [len(PROMPT) + 1], [0.0], [0], 0)
    with pytest.raises(ValueError):
        eng.set_logprobs([21])


def test_fault_wrapper_passes_both_calls_through(setup):
    from aios_amd.runtime.faults import FaultSpec, FaultyEngine

    path, _ = setup
    eng = FaultyEngine(_engine(path), FaultSpec(""))
    eng.prefill(0, PROMPT, 0, True)
    eng.set_logprobs([0])
    eng.sample_first(len(PROMPT) - 1, 0.0, 0, 1.0, 1)
    assert len(eng.last_logprobs()) == 3


def test_engine_without_set_logprobs_finishes_with_an_error(setup):
    path, tok = setup
    sched = Scheduler(_Bare(_engine(path)), tok, max_batch=2, max_slots=2, max_ctx=128)
    assert not sched.can_logprobs
    bad, ok = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=3, logprobs=True, top_logprobs=2),
                           GenRequest(prompt_ids=list(PROMPT), max_tokens=3)])
    assert bad.finish_reason == "error" and "logprobs" in bad.error and bad.logprobs is None
    assert ok.finish_reason != "error" and ok.completion_tokens >= 1


def test_tensor_parallel_engine_has_neither_call(setup):
    """the runtime's tensor-parallel tier (parallel/tp.py TPEngine) forwards unknown names to its shard's
    Engine, which binds both calls (and throws from set_logprobs): the wrapper has to hide them, so that the
    scheduler refuses the one request instead of running into an engine failure that takes the tier down"""
    from aios_amd.parallel.tp import TPEngine

    path, tok = setup
    shard = _engine(path)
    assert hasattr(shard, "set_logprobs") and hasattr(shard, "last_logprobs")
    eng = TPEngine(shard, comm=type("Comm", (), {"error": staticmethod(lambda: False)})(), send=lambda msg: None)
    assert not hasattr(eng, "set_logprobs") and not hasattr(eng, "last_logprobs")
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128)
    assert not sched.can_logprobs
    bad, ok = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=3, logprobs=True, top_logprobs=2),
                           GenRequest(prompt_ids=list(PROMPT), max_tokens=3)])
    assert bad.finish_reason == "error" and "logprobs" in bad.error
    assert ok.finish_reason != "error" and ok.completion_tokens >= 1 and not sched.failed


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

    return Mgr(base_port=18940)


def _serve(path, tok, port, calls, bare=False):
    """start the endpoint of one model, run `calls(session, url)`, tear down"""
    import aiohttp

    from aios_amd.runtime.service import AIRuntimeService

    async def run():
        mgr = _manager(path, tok, bare)
        svc = AIRuntimeService(mgr, http=True)
        m = await mgr.load_model("tiny", "fake.gguf", port=port)
        await svc.start_http(m)
        try:
            async with aiohttp.ClientSession() as s:
                return await calls(s, f"http://127.0.0.1:{port}/v1/chat/completions")
        finally:
            await svc.close()

    return asyncio.run(run())


MSG = [{"role": "user", "content": "hi"}]


def test_http_response_has_the_openai_shape(setup):
    path, tok = setup

    async def calls(s, url):
        body = {"messages": MSG, "max_tokens": 6, "temperature": 0.8, "seed": 4, "logprobs": True, "top_logprobs": 4}
        async with s.post(url, json=body) as r:
            assert r.status == 200
            with_lp = await r.json()
        async with s.post(url, json={"messages": MSG, "max_tokens": 3}) as r:
            without = await r.json()
        async with s.post(url, json={"messages": MSG, "max_tokens": 3, "logprobs": True}) as r:
            top0 = await r.json()
        return with_lp, without, top0

    js, without, top0 = _serve(path, tok, 18941, calls)
    content = js["choices"][0]["logprobs"]["content"]
    assert len(content) == js["usage"]["completion_tokens"] >= 1
    text = b""
    for it in content:
        assert set(it) == {"token", "logprob", "bytes", "top_logprobs"}
        assert bytes(it["bytes"]).decode("utf-8", errors="replace") == it["token"]
        assert isinstance(it["logprob"], float) and it["logprob"] <= 0.0
        alts = it["top_logprobs"]
        assert len(alts) == 4 and all(set(a) == {"token", "logprob", "bytes"} for a in alts)
        lps = [a["logprob"] for a in alts]
        assert lps == sorted(lps, reverse=True)
        same = [a for a in alts if a["bytes"] == it["bytes"]]
        if same:  # the chosen token among its alternatives: the same number
            assert same[0]["logprob"] == it["logprob"]
        else:
            assert it["logprob"] <= lps[-1]
        text += bytes(it["bytes"])
    assert text.decode("utf-8", errors="replace").strip() == js["choices"][0]["message"]["content"].strip()
    assert "logprobs" not in without["choices"][0]   # a request that did not ask: the body it always had
    assert all(it["top_logprobs"] == [] for it in top0["choices"][0]["logprobs"]["content"])


def test_http_rejects_what_it_cannot_serve(setup):
    path, tok = setup

    async def calls(s, url):
        out = []
        for extra in ({"top_logprobs": 3}, {"logprobs": True, "top_logprobs": 21}, {"logprobs": True, "top_logprobs": -1},
                      {"logprobs": True, "stream": True}):
            async with s.post(url, json=dict({"messages": MSG, "max_tokens": 3}, **extra)) as r:
                out.append((r.status, await r.json()))
        return out

    for status, js in _serve(path, tok, 18942, calls):
        assert status == 400 and js["error"]["type"] == "invalid_request_error"


def test_http_rejects_logprobs_on_a_tier_without_them(setup):
    path, tok = setup

    async def calls(s, url):
        async with s.post(url, json={"messages": MSG, "max_tokens": 3, "logprobs": True}) as r:
            bad = (r.status, await r.json())
        async with s.post(url, json={"messages": MSG, "max_tokens": 3}) as r:
            return bad, r.status

    (status, js), ok = _serve(path, tok, 18943, calls, bare=True)
    assert status == 400 and js["error"]["type"] == "invalid_request_error" and ok == 200


def test_negative_infinity_is_reported_as_minus_9999(setup):
    from aios_amd.runtime import service

    _, tok = setup
    c = service.logprobs_content(tok, [(5, -0.5, [(5, -0.5), (6, float("-inf"))])])
    assert c[0]["logprob"] == -0.5 and c[0]["top_logprobs"][1]["logprob"] == -9999.0
    assert c[0]["bytes"] == list(tok.token_bytes(5))
