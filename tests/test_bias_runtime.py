"""logit_bias and ignore_eos through the runtime on the CPU backend: the scheduler (a ban moves the greedy token
to the argmax of logits + bias, ignore_eos runs past EOS, the grammar wins over bans for one step, tiers that
cannot apply a bias refuse it, requests without the fields make the engine calls they always made) and the two
HTTP endpoints (both body forms, every 400)."""
import asyncio
import json
import threading

import numpy as np
import pytest

from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab, write_synthetic_gguf
from aios_amd.runtime import chat_template, native, service
from aios_amd.runtime import sampler as host
from aios_amd.runtime.cpu_engine import CpuEngine
from aios_amd.runtime.scheduler import GenRequest, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

PROMPT = [1, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49]
V = 512
EOS = 2


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    p = tmp_path_factory.mktemp("bias") / "tiny.gguf"
    write_synthetic_gguf(str(p), get_preset("test-tiny"), "Q8_0", seed=5)
    t, s, ty = synthetic_vocab(V)
    return str(p), SpmTokenizer(t, s, ty, 1, EOS)


def _engine(path, **kw):
    return CpuEngine.from_gguf(path, max_ctx=128, max_slots=2, max_batch=2, **kw)


class _Spy:
    """the engine with the arguments of its set_sample_processors calls recorded"""

    def __init__(self, eng):
        self._eng = eng
        self.proc_calls = []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def set_sample_processors(self, *a, **kw):
        self.proc_calls.append((a, kw))
        return self._eng.set_sample_processors(*a, **kw)


class _Bare:
    """a tensor-parallel tier's surface: the engine without set_sample_processors"""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        if name == "set_sample_processors":
            raise AttributeError(name)
        return getattr(self._eng, name)


def _run(sched, reqs, together=True):
    evs, box = [threading.Event() for _ in reqs], {}
    try:
        for i, r in enumerate(reqs):
            r.on_done = lambda res, i=i: (box.__setitem__(i, res), evs[i].set())
        if together:
            with sched.cv:
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


def _sched(eng, tok, grammar=None):
    return Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128, grammar=grammar)


def _first_logits(path):
    eng = _engine(path)
    return eng.model.forward(list(PROMPT), eng.model.new_cache()).numpy()[-1].astype(np.float32)


# ---- scheduler --------------------------------------------------------------------------------------------
def test_banning_the_greedy_first_token_moves_it_to_the_biased_argmax(setup):
    path, tok = setup
    logits = _first_logits(path)
    order = np.argsort(-logits)
    best, third = int(order[0]), int(order[2])
    # the best token banned and the third lifted over the second: the answer is neither of the raw top two
    bias = {best: -np.inf, third: float(logits[order[1]] - logits[third]) + 1.0}
    want = int(np.argmax(host.apply_logit_bias(logits, list(bias), list(bias.values()))))
    assert want == third
    eng = _Spy(_engine(path))
    plain, biased = _run(_sched(eng, tok), [GenRequest(prompt_ids=list(PROMPT), max_tokens=4, stop_ids=[]),
                                            GenRequest(prompt_ids=list(PROMPT), max_tokens=4, stop_ids=[],
                                                       logit_bias=bias)], together=False)
    assert plain.token_ids[0] == best and biased.token_ids[0] == want
    assert best not in biased.token_ids  # the ban holds at every step, not only the first
    # the plain request staged nothing; the biased one staged its list before every sampler launch
    assert len(eng.proc_calls) == len(biased.token_ids)
    for a, _ in eng.proc_calls:
        assert len(a) == 7 and a[:5] == ([0.0], [1.0], [0.0], [0.0], [[]]) and a[5] == [list(bias)]
        assert a[6] == [list(bias.values())]


def test_bias_and_penalties_together_follow_the_chain_order(setup):
    """two rows in one batch, one with a bias and a penalty, one plain: the first token of the biased row is the
    argmax of penalties(bias(logits)) with the prompt tail as its window"""
    path, tok = setup
    logits = _first_logits(path)
    best = int(np.argmax(logits))
    bias = {best: -2.5, PROMPT[-1]: 30.0}
    want = host.apply_penalties(host.apply_logit_bias(logits, list(bias), list(bias.values())), PROMPT[-4:], 1.0, 40.0, 0.0)
    a, b = _run(_sched(_engine(path), tok), [
        GenRequest(prompt_ids=list(PROMPT), max_tokens=3, stop_ids=[], logit_bias=bias, presence_penalty=40.0,
                   repeat_last_n=4),
        GenRequest(prompt_ids=list(PROMPT), max_tokens=3, stop_ids=[])])
    assert a.token_ids[0] == int(np.argmax(want)) != PROMPT[-1]  # (+30 alone would have chosen the prompt's tail)
    assert b.token_ids[0] == best


def test_ignore_eos_runs_to_max_tokens(setup):
    path, tok = setup

    def engine():
        eng = _engine(path)
        fwd = eng.model.forward

        def forward(ids, cache):  # a model whose greedy choice is EOS at every step
            out = fwd(ids, cache)
            out[:, EOS] += 1e3
            return out

        eng.model.forward = forward
        return eng

    stops, runs, both = _run(_sched(engine(), tok), [
        GenRequest(prompt_ids=list(PROMPT), max_tokens=6),
        GenRequest(prompt_ids=list(PROMPT), max_tokens=6, ignore_eos=True),
        GenRequest(prompt_ids=list(PROMPT), max_tokens=6, ignore_eos=True, logit_bias={EOS: 5.0, 7: 0.25})],
        together=False)
    assert stops.finish_reason == "stop" and stops.token_ids == []
    for r in (runs, both):  # (a finite bias on EOS is overridden by the ban)
        assert r.finish_reason == "length" and len(r.token_ids) == 6 and EOS not in r.token_ids
    # a stop id other than EOS still ends such a request
    first = runs.token_ids[0]
    cut, = _run(_sched(engine(), tok), [GenRequest(prompt_ids=list(PROMPT), max_tokens=6, ignore_eos=True,
                                                   stop_ids=[first])])
    assert cut.finish_reason == "stop" and cut.token_ids == []


class _State:
    def __init__(self, toks=()):
        self.toks = list(toks)

    def copy(self):
        return _State(self.toks)


class _OpenFirst:
    """a grammar whose first token must be `open_`; everything is allowed behind it and it never completes"""

    def __init__(self, open_):
        self.open = open_

    def initial(self):
        return _State()

    def accept_token(self, st, tok):
        if not st.toks and tok != self.open:
            return False
        st.toks.append(tok)
        return True

    def complete(self, st):
        return False

    def mask(self, st):
        if st.toks:
            return host.all_allowed(V)
        bits = np.zeros(V, np.uint8)
        bits[self.open] = 1
        return np.packbits(bits, bitorder="little").tobytes()

    mask_open = mask


def test_the_grammar_wins_over_a_ban_for_that_step(setup):
    path, tok = setup
    brace = int(tok.encode("{", add_bos=False)[-1])
    eng = _Spy(_engine(path))
    sched = _sched(eng, tok, grammar=_OpenFirst(brace))
    r, = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=5, json_mode=True, stop_ids=[],
                                 logit_bias={brace: -np.inf, 9: 0.5})])
    assert r.finish_reason == "length" and r.token_ids[0] == brace  # the only token the grammar allows
    assert brace not in r.token_ids[1:]                                # ... and banned again where it allows others
    assert sched.stats["bias_overridden"] == 1
    # that one step was staged without the ban, with the finite entry kept
    lists = [(a[5][0], a[6][0]) for a, _ in eng.proc_calls]
    assert lists[0] == ([9], [0.5]) and all(l == ([brace, 9], [-np.inf, 0.5]) for l in lists[1:])


@pytest.mark.skipif(native.load() is None, reason="native extension not built")
def test_the_json_grammar_wins_when_all_it_allows_is_banned(setup):
    path, tok = setup
    g = native.load().JsonGrammar(tok.all_token_bytes(), tok.eos_id)
    openers = [int(t) for t in np.flatnonzero(host.mask_to_bool(g.mask(g.initial()), V))]
    assert openers and len(openers) < host.BIAS_MAX
    sched = _sched(_engine(path), tok, grammar=g)
    r, = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=3, json_mode=True,
                                 logit_bias={t: -np.inf for t in openers})])
    assert r.finish_reason != "error" and r.token_ids and r.token_ids[0] in openers
    assert sched.stats["bias_overridden"] >= 1


def test_requests_without_the_fields_make_the_calls_they_always_made(setup):
    path, tok = setup
    eng = _Spy(_engine(path))
    plain, = _run(_sched(eng, tok), [GenRequest(prompt_ids=list(PROMPT), max_tokens=4, stop_ids=[])])
    assert eng.proc_calls == [] and len(plain.token_ids) == 4  # neutral: no call at all
    eng = _Spy(_engine(path))
    sched = _sched(eng, tok)
    pen, = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=4, stop_ids=[], repeat_penalty=1.3)])
    # one call per sampler launch, with the five arguments of the call before logit_bias existed
    # (a launch that drew EOS ended the request without a token)
    assert len(eng.proc_calls) == len(pen.token_ids) + (pen.finish_reason == "stop") >= 1
    assert all(len(a) == 5 and not kw for a, kw in eng.proc_calls)
    assert sched.stats["bias_overridden"] == 0
    # an empty map and ignore_eos: false are "without the fields" too
    eng = _Spy(_engine(path))
    same, = _run(_sched(eng, tok), [GenRequest(prompt_ids=list(PROMPT), max_tokens=4, stop_ids=[], logit_bias={},
                                               ignore_eos=False)])
    assert eng.proc_calls == [] and same.token_ids == plain.token_ids


def test_bad_lists_and_tiers_without_the_call_finish_with_an_error(setup):
    path, tok = setup
    bad = [{V: 1.0}, {-1: 1.0}, {5: np.inf}, {5: float("nan")}, {"w5": 1.0}, {5.5: 1.0},
           {t: -np.inf for t in range(V)}]
    res = _run(_sched(_engine(path), tok), [GenRequest(prompt_ids=list(PROMPT), max_tokens=2, logit_bias=b) for b in bad]
               + [GenRequest(prompt_ids=list(PROMPT), max_tokens=2)], together=False)
    for b, r in zip(bad, res):
        assert r.finish_reason == "error" and "logit_bias" in r.error, b
    assert res[-1].finish_reason != "error" and res[-1].token_ids
    sched = _sched(_Bare(_engine(path)), tok)
    assert not sched.can_bias
    refused, eos, ok = _run(sched, [GenRequest(prompt_ids=list(PROMPT), max_tokens=2, logit_bias={5: 1.0}),
                                    GenRequest(prompt_ids=list(PROMPT), max_tokens=2, ignore_eos=True),
                                    GenRequest(prompt_ids=list(PROMPT), max_tokens=2, repeat_penalty=1.2)])
    for r in (refused, eos):
        assert r.finish_reason == "error" and "single-GPU engines only" in r.error
    assert ok.finish_reason != "error" and ok.token_ids and not sched.failed  # (penalties there: ignored, as before)
    assert sorted(sched.free_slots) == [0, 1]


def test_cpu_engine_validates_like_the_native_one(setup):
    path, _ = setup
    eng = _engine(path)
    args = ([0.0], [1.0], [0.0], [0.0], [[]])
    eng.set_sample_processors(*args, [[]], [[]])
    eng.set_sample_processors(*args)
    for ids, vals in (([[1]], [[0.0], [0.0]]), ([[1, 2]], [[0.0]]), ([[V]], [[0.0]]), ([[3, 3]], [[0.0, 0.0]]),
                      ([[3]], [[np.inf]]), ([[3]], [[np.nan]]), ([list(range(V))], [[-np.inf] * V])):
        with pytest.raises(ValueError):
            eng.set_sample_processors(*args, ids, vals)


def test_tensor_parallel_engine_hides_the_call(setup):
    from aios_amd.parallel.tp import TPEngine

    path, _ = setup
    eng = TPEngine(_engine(path), comm=type("Comm", (), {"error": staticmethod(lambda: False)})(), send=lambda msg: None)
    assert not hasattr(eng, "set_sample_processors")


# ---- HTTP -------------------------------------------------------------------------------------------
def test_body_parser_forms_and_limits():
    class S:
        vocab, can_bias = 1024, True

    f = service.bias_from_body
    assert f({}, S) == (None, False) and f({"logit_bias": {}, "ignore_eos": False}, S) == (None, False)
    assert f({"logit_bias": {"5": -100, "7": 2.5, " 9 ": 1e4}}, S) == ({5: -100.0, 7: 2.5, 9: 1e4}, False)
    got, ieos = f({"logit_bias": [[5, False], [7, 2.5], [8, float("-inf")]], "ignore_eos": True}, S)
    assert got == {5: -np.inf, 7: 2.5, 8: -np.inf} and ieos is True
    assert len(f({"logit_bias": {str(i): 1 for i in range(512)}}, S)[0]) == 512
    with pytest.raises(ValueError, match="logit_bias: more than 512"):
        f({"logit_bias": {str(i): 1 for i in range(513)}}, S)
    with pytest.raises(ValueError, match="logit_bias: more than 512"):
        f({"logit_bias": [[i, 1] for i in range(513)]}, S)


BAD_BODIES = [
    ({"logit_bias": {"w5": 1}}, "logit_bias"), ({"logit_bias": {"5.5": 1}}, "logit_bias"),
    ({"logit_bias": {str(V): 1}}, "logit_bias"), ({"logit_bias": {"-1": 1}}, "logit_bias"),
    ({"logit_bias": [[V, 1]]}, "logit_bias"), ({"logit_bias": [["5", 1]]}, "logit_bias"),
    ({"logit_bias": [[5.5, 1]]}, "logit_bias"), ({"logit_bias": [[True, 1]]}, "logit_bias"),
    ({"logit_bias": {"5": "x"}}, "logit_bias"), ({"logit_bias": {"5": None}}, "logit_bias"),
    ({"logit_bias": {"5": True}}, "logit_bias"), ({"logit_bias": [[5, [1]]]}, "logit_bias"),
    ({"logit_bias": {"5": float("nan")}}, "logit_bias"), ({"logit_bias": {"5": float("inf")}}, "logit_bias"),
    ({"logit_bias": [[5, float("inf")]]}, "logit_bias"),
    ({"logit_bias": [[i % V, 1] for i in range(513)]}, "logit_bias"),
    ({"logit_bias": [[5, 1], [6, 1], [5, 2]]}, "logit_bias: duplicate"),
    ({"logit_bias": [[5]]}, "logit_bias"), ({"logit_bias": [5, 1]}, "logit_bias"), ({"logit_bias": "5:1"}, "logit_bias"),
    ({"ignore_eos": 1}, "ignore_eos"), ({"ignore_eos": "yes"}, "ignore_eos"),
]


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

    return Mgr(base_port=19010)


def _serve(path, tok, port, calls, bare=False):
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


async def _post(s, url, body):
    # (json.dumps writes NaN / Infinity as the bare words Python's parser takes back)
    async with s.post(url, data=json.dumps(body), headers={"Content-Type": "application/json"}) as r:
        return r.status, await r.json()


CHAT = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 4, "temperature": -1}
CMPL = {"prompt": PROMPT, "max_tokens": 4, "temperature": 0}


def test_http_rejects_malformed_fields_on_both_endpoints(setup):
    path, tok = setup

    async def calls(s, base):
        out = []
        for extra, word in BAD_BODIES:
            for url, body in ((base + "/v1/chat/completions", CHAT), (base + "/v1/completions", CMPL)):
                out.append((url, extra, word, await _post(s, url, dict(body, **extra))))
        return out

    for url, extra, word, (status, js) in _serve(path, tok, 19011, calls):
        assert status == 400 and js["error"]["type"] == "invalid_request_error", (url, extra, js)
        assert word in js["error"]["message"], (url, extra, js)


def test_http_tensor_parallel_tier_refuses_both_fields(setup):
    path, tok = setup

    async def calls(s, base):
        out = []
        for url, body in ((base + "/v1/chat/completions", CHAT), (base + "/v1/completions", CMPL)):
            out.append(await _post(s, url, dict(body, logit_bias={"5": 1})))
            out.append(await _post(s, url, dict(body, ignore_eos=True)))
            out.append(await _post(s, url, dict(body, logit_bias={}, ignore_eos=False)))
        return out

    res = _serve(path, tok, 19012, calls, bare=True)
    for bias, eos, neither in (res[:3], res[3:]):
        assert bias[0] == 400 and "logit_bias: single-GPU engines only" in bias[1]["error"]["message"]
        assert eos[0] == 400 and "ignore_eos: single-GPU engines only" in eos[1]["error"]["message"]
        assert neither[0] == 200


def test_http_applies_both_forms(setup):
    path, tok = setup
    logits = _first_logits(path)
    best = int(np.argmax(logits))
    lifted = int(np.argsort(-logits)[5])

    async def calls(s, base):
        url = base + "/v1/completions"
        out = [await _post(s, url, CMPL),
               await _post(s, url, dict(CMPL, logit_bias={str(best): float("-inf"), str(lifted): 1000})),
               await _post(s, url, dict(CMPL, logit_bias=[[best, False], [lifted, 1000]])),
               await _post(s, url, dict(CMPL, max_tokens=1, logit_bias={str(EOS): 1000})),
               await _post(s, url, dict(CMPL, max_tokens=3, logit_bias={str(EOS): 1000}, ignore_eos=True))]
        chat = base + "/v1/chat/completions"
        out += [await _post(s, chat, CHAT), await _post(s, chat, dict(CHAT, logit_bias={str(lifted): 1000}))]
        return out

    plain, as_map, as_list, eos, past_eos, chat, chat_biased = _serve(path, tok, 19013, calls)
    assert all(r[0] == 200 for r in (plain, as_map, as_list, eos, past_eos, chat, chat_biased))
    text = lambda r: r[1]["choices"][0]["text"]  # noqa: E731
    # +1000 is outside OpenAI's range and taken as it is: every token is the lifted one
    assert text(as_map) == text(as_list) == tok.decode([lifted] * 4) != text(plain)
    assert eos[1]["usage"]["completion_tokens"] == 0 and eos[1]["choices"][0]["finish_reason"] == "stop"
    assert past_eos[1]["usage"]["completion_tokens"] == 3 and past_eos[1]["choices"][0]["finish_reason"] == "length"
    assert chat_biased[1]["choices"][0]["message"]["content"] == tok.decode([lifted] * 4)
    assert chat_biased[1]["choices"][0]["message"]["content"] != chat[1]["choices"][0]["message"]["content"]
