"""Logit processors off the GPU: the host sampler's rule (the reference of the device sampler's tests),
the scheduler's calls over the CPU engine, the tier defaults from the node config and the fields of the
OpenAI endpoint."""
import asyncio
import threading

import numpy as np
import pytest

from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab, write_synthetic_gguf
from aios_amd.runtime import sampler as host
from aios_amd.runtime.cpu_engine import CpuEngine
from aios_amd.runtime.scheduler import GenRequest, GenResult, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer


# ---- host sampler rule ---------------------------------------------------------------------------
def test_apply_penalties_rule():
    l = np.array([2.0, -2.0, 1.0, 0.5, -0.5, 3.0], np.float32)
    out = host.apply_penalties(l, [0, 1, 1, 3, 3, 3, -1, 99], repeat_penalty=2.0, presence_penalty=0.25,
                               frequency_penalty=0.5)
    assert out.dtype == np.float32
    want = [2.0 / 2 - (0.5 + 0.25),        # positive logit: divided; count 1
            -2.0 * 2 - (2 * 0.5 + 0.25),   # negative logit: multiplied; count 2
            1.0,                           # not in the window
            0.5 / 2 - (3 * 0.5 + 0.25),    # count 3
            -0.5, 3.0]
    assert np.allclose(out, want, rtol=0, atol=1e-7)
    assert l[0] == 2.0  # a copy
    # neutral values and an empty window change nothing
    assert np.array_equal(host.apply_penalties(l, [0, 1, 3]), l)
    assert np.array_equal(host.apply_penalties(l, [], 2.0, 1.0, 1.0), l)
    assert np.array_equal(host.apply_penalties(l, [-1, -1], 2.0, 1.0, 1.0), l)


def test_penalty_window_clamp():
    assert [host.penalty_window(n) for n in (0, 1, 64, 256, 257, -1)] == [0, 1, 64, 256, 256, 256]


def test_min_p_ratio_and_mask():
    T = 0.8
    l = np.full(50, -30.0)
    l[[3, 7, 11, 19, 23]] = [1.0, 0.5, 0.0, -0.5, -1.0]  # ratios 1, 0.54, 0.29, 0.15, 0.08
    p = host.probabilities(l, T, min_p=0.2)
    assert set(np.nonzero(p)[0]) == {3, 7, 11}
    w = np.exp(np.array([1.0, 0.5, 0.0]) / T)
    assert np.allclose(p[[3, 7, 11]], w / w.sum())
    # it intersects with the nucleus instead of renormalising before it: top-p 0.5 keeps two tokens
    # (0.44 < 0.5), and the second one passes min-p on its ratio to the best (0.54), whatever its mass
    p2 = host.probabilities(l, T, top_p=0.5, min_p=0.5)
    assert set(np.nonzero(p2)[0]) == {3, 7}
    # masked: the ratio is to the best ALLOWED token
    bits = np.ones(50, np.uint8)
    bits[3] = 0
    mask = np.packbits(bits, bitorder="little").tobytes()
    pm = host.probabilities(l, T, mask=mask, min_p=0.2)
    assert set(np.nonzero(pm)[0]) == {7, 11, 19}
    # min_p off: the five spikes carry (nearly) all the mass
    assert np.count_nonzero(host.probabilities(l, T) > 1e-9) == 5
    # draws stay inside the survivors; greedy ignores min-p
    rng = np.random.default_rng(0)
    assert {host.sample(l, T, 0, 1.0, None, rng, min_p=0.2) for _ in range(200)} == {3, 7, 11}
    assert host.sample(l, 0.0, min_p=0.99) == 3
    # existing positional calls are unaffected
    assert host.sample(l, 0.0, 0, 1.0, mask, None) == 7


# ---- scheduler over the CPU engine ---------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    p = tmp_path_factory.mktemp("proc") / "small.gguf"
    write_synthetic_gguf(str(p), get_preset("test-small"), "Q8_0", seed=11)
    t, s, ty = synthetic_vocab(1024)
    return str(p), SpmTokenizer(t, s, ty, 1, 2)


def _generate(eng, tok, req, **sched_kw):
    sched = Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128, **sched_kw)
    ev, box = threading.Event(), {}

    def done(r):
        box["r"] = r
        ev.set()

    req.on_done = done
    try:
        sched.submit(req)
        assert ev.wait(60)
    finally:
        sched.close()
    return box["r"]


def _spied(path):
    eng = CpuEngine.from_gguf(path, max_ctx=128, max_slots=2, max_batch=2)
    calls = {"decode": [], "proc": []}
    dec, setp = eng.decode, eng.set_sample_processors

    def decode(*a):
        calls["decode"].append(a)
        return dec(*a)

    def set_sample_processors(*a):
        calls["proc"].append(a)
        return setp(*a)

    eng.decode, eng.set_sample_processors = decode, set_sample_processors
    return eng, calls


# (the end-of-sequence id 2 is in the prompt: penalised like the rest of it, it cannot end the run early)
PROMPT = [1, 2, 40, 41, 42, 43]


def test_presence_penalty_stops_repeats(setup):
    path, tok = setup
    eng, calls = _spied(path)
    r = _generate(eng, tok, GenRequest(prompt_ids=list(PROMPT), max_tokens=12, presence_penalty=1e4, repeat_last_n=256))
    assert r.finish_reason == "length" and len(r.token_ids) == 12
    assert len(set(r.token_ids)) == 12 and not set(r.token_ids) & set(PROMPT)
    # one call per sampler launch (first token + 11 steps), each with the row's whole history so far
    assert len(calls["proc"]) == 12
    for i, (mp, rp, pp, fp, recent) in enumerate(calls["proc"]):
        assert (mp, rp, pp, fp) == ([0.0], [1.0], [1e4], [0.0])
        assert recent == [PROMPT + r.token_ids[:i]]
    assert all(len(c) == 9 for c in calls["decode"])


def test_negative_presence_penalty_keeps_to_the_window(setup):
    """the counterpart that no unpenalised run passes: a reward of 1e4 for the window's tokens"""
    path, tok = setup
    prompt = [1, 40, 41, 42, 43]
    eng = CpuEngine.from_gguf(path, max_ctx=128, max_slots=2, max_batch=2)
    plain = _generate(eng, tok, GenRequest(prompt_ids=list(prompt), max_tokens=8))
    assert not set(plain.token_ids) <= set(prompt)
    r = _generate(eng, tok, GenRequest(prompt_ids=list(prompt), max_tokens=8, presence_penalty=-1e4, repeat_last_n=-1))
    assert len(r.token_ids) == 8 and set(r.token_ids) <= set(prompt)


def test_window_is_the_last_n_tokens(setup):
    path, tok = setup
    eng, calls = _spied(path)
    r = _generate(eng, tok, GenRequest(prompt_ids=list(PROMPT), max_tokens=6, frequency_penalty=0.5, repeat_last_n=4))
    for i, (_, _, _, _, recent) in enumerate(calls["proc"]):
        assert recent == [(PROMPT + r.token_ids[:i])[-4:]]


def test_neutral_request_makes_no_call(setup):
    path, tok = setup
    eng, calls = _spied(path)
    r = _generate(eng, tok, GenRequest(prompt_ids=list(PROMPT), max_tokens=8, min_p=0.0, repeat_penalty=1.0,
                                       presence_penalty=0.0, frequency_penalty=0.0))
    assert r.finish_reason in ("length", "stop")
    assert calls["proc"] == []
    assert calls["decode"] and all(len(c) == 9 for c in calls["decode"])


def test_engine_without_the_method_still_serves(setup):
    path, tok = setup

    class Bare:
        """the CPU engine minus set_sample_processors"""

        def __init__(self, eng):
            self._eng = eng
            self.config = eng.config

        def prefill(self, *a):
            return self._eng.prefill(*a)

        def decode(self, *a):
            return self._eng.decode(*a)

    eng = Bare(CpuEngine.from_gguf(path, max_ctx=128, max_slots=2, max_batch=2))
    assert not hasattr(eng, "set_sample_processors")
    r = _generate(eng, tok, GenRequest(prompt_ids=list(PROMPT), max_tokens=6, min_p=0.1, temperature=0.7, seed=5))
    assert r.finish_reason in ("length", "stop") and r.error == ""


def test_cpu_engine_processors_are_one_shot(setup):
    path, _ = setup
    eng = CpuEngine.from_gguf(path, max_ctx=128, max_slots=2, max_batch=2)
    logits = np.asarray(eng.prefill(0, [1, 40, 41], 0, True))
    best = int(np.argmax(logits))
    eng.set_sample_processors([0.0], [1.0], [1e4], [0.0], [[best]])
    assert eng.sample_first(2, 0.0, 0, 1.0, 1) != best
    assert eng.sample_first(2, 0.0, 0, 1.0, 1) == best
    with pytest.raises(ValueError):
        eng.set_sample_processors([0.0], [1.0], [0.0], [0.0], [[1] * 257])
    with pytest.raises(ValueError):
        eng.set_sample_processors([0.0], [1.0], [0.0], [0.0], [[eng.config.vocab_size]])
    with pytest.raises(ValueError):
        eng.set_sample_processors([0.0, 0.0], [1.0], [0.0], [0.0], [[1]])


def test_fault_wrapper_passes_the_method_through(setup):
    from aios_amd.runtime.faults import FaultSpec, FaultyEngine

    path, _ = setup
    eng = FaultyEngine(CpuEngine.from_gguf(path, max_ctx=128, max_slots=2, max_batch=2), FaultSpec(""))
    assert hasattr(eng, "set_sample_processors")
    eng.set_sample_processors([0.1], [1.0], [0.0], [0.0], [[5]])


# ---- config ----------------------------------------------------------------------------------------
TOML = """
[models.a]
file = "synthetic:test-small"
min_p = 0.05
repeat_penalty = 1.1
[models.b]
file = "synthetic:test-small"
kv_dtype = "fp8_e4m3"
presence_penalty = 0.5
frequency_penalty = 0.25
[models.c]
file = "synthetic:test-small"
"""


def test_config_keys_reach_the_scheduler_defaults(tmp_path, setup):
    from aios_amd.parallel.tp import spec_kv_dtype, spec_sampling
    from aios_amd.utils import config as node_config

    t = node_config.ModelTier()
    assert (t.min_p, t.repeat_penalty, t.presence_penalty, t.frequency_penalty) == (0.0, 1.0, 0.0, 0.0)
    f = tmp_path / "c.toml"
    f.write_text(TOML)
    cfg = node_config.load(str(f), env={})
    assert not cfg.warnings
    specs = {n: s for n, s, _ in cfg.model_specs()}
    assert {p["name"]: p["spec"] for p in cfg.tier_plan()} == specs
    assert spec_sampling(specs["a"]) == {"min_p": 0.05, "repeat_penalty": 1.1}
    assert spec_sampling(specs["b"]) == {"presence_penalty": 0.5, "frequency_penalty": 0.25}
    assert spec_kv_dtype(specs["b"]) == "fp8_e4m3"
    assert specs["c"] == "synthetic:test-small" and spec_sampling(specs["c"]) == {}

    # the tier's values act as the defaults of requests that leave the fields unset
    path, tok = setup
    eng, calls = _spied(path)
    _generate(eng, tok, GenRequest(prompt_ids=list(PROMPT), max_tokens=3), sampling_defaults=spec_sampling(specs["a"]))
    assert calls["proc"] and all(c[:4] == ([0.05], [1.1], [0.0], [0.0]) for c in calls["proc"])
    eng, calls = _spied(path)
    _generate(eng, tok, GenRequest(prompt_ids=list(PROMPT), max_tokens=3, min_p=0.0, repeat_penalty=1.0),
              sampling_defaults=spec_sampling(specs["a"]))
    assert calls["proc"] == []  # a request may set them back to neutral
    with pytest.raises(ValueError):
        Scheduler(eng, tok, max_batch=2, max_slots=2, max_ctx=128, sampling_defaults={"top_q": 1.0}).close()


def test_model_manager_hands_the_defaults_to_the_scheduler():
    import inspect

    from aios_amd.runtime import model_manager

    src = inspect.getsource(model_manager.ModelManager._load_blocking)
    assert "sampling_defaults=spec_sampling(m.path)" in src


def test_default_config_documents_the_keys():
    import os

    from aios_amd.utils import config as node_config

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "config", "default-config.toml")
    cfg = node_config.load(path, env={})
    assert not cfg.warnings
    t = cfg.models.tiers["tactical"]
    assert (t.min_p, t.repeat_penalty, t.presence_penalty, t.frequency_penalty) == (0.0, 1.0, 0.0, 0.0)
    assert "0.05" in open(path).read()


# ---- HTTP ------------------------------------------------------------------------------------------
class _Sched:
    def __init__(self):
        self.reqs = []

    def submit(self, req):
        self.reqs.append(req)
        req.on_done(GenResult("ok", [5], len(req.prompt_ids), 1, "stop"))


class _Model:
    name = "m"

    def __init__(self, tok):
        self.tokenizer = tok
        self.scheduler = _Sched()
        self.template = type("T", (), {"render": staticmethod(lambda msgs, add_generation_prompt=True: "hello")})()


class _Request:
    def __init__(self, m, body):
        self.app = {"model": m}
        self._body = body

    async def json(self):
        return self._body


def test_http_body_fields_land_in_the_request(setup):
    from aios_amd.runtime import service

    _, tok = setup
    m = _Model(tok)
    svc = object.__new__(service.AIRuntimeService)
    body = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 7, "temperature": 0.7, "top_p": 0.8,
            "top_k": 20, "seed": 99, "min_p": 0.05, "repeat_penalty": 1.1, "presence_penalty": 0.5,
            "frequency_penalty": 0.25}
    resp = asyncio.run(svc._http_chat(_Request(m, body)))
    assert resp.status == 200
    r = m.scheduler.reqs[-1]
    assert (r.max_tokens, r.temperature, r.top_p, r.top_k, r.seed) == (7, 0.7, 0.8, 20, 99)
    assert (r.min_p, r.repeat_penalty, r.presence_penalty, r.frequency_penalty) == (0.05, 1.1, 0.5, 0.25)
    # absent (or null) fields stay the request's and the tier's defaults
    asyncio.run(svc._http_chat(_Request(m, {"messages": [], "top_p": None})))
    r = m.scheduler.reqs[-1]
    d = GenRequest(prompt_ids=[])
    assert (r.top_p, r.top_k, r.seed) == (d.top_p, d.top_k, d.seed)
    assert (r.min_p, r.repeat_penalty, r.presence_penalty, r.frequency_penalty) == (None, None, None, None)
    bad = asyncio.run(svc._http_chat(_Request(m, {"messages": [], "min_p": "lots"})))
    assert bad.status == 400
    # generate()'s keyword takes the same names and refuses others
    asyncio.run(service.generate(m, [], 4, 0.0, False, sampling={"min_p": 0.1}))
    assert m.scheduler.reqs[-1].min_p == 0.1
    with pytest.raises(ValueError):
        asyncio.run(service.generate(m, [], 4, 0.0, False, sampling={"max_tokens": 1}))
