"""The scheduler's context shift on a recording fake engine (no device, no model): the engine's next token is a
function of the number of tokens the slot holds, every call is logged, and shift_context does to the slot's token
list what the rule (tests/context_shift_oracle.py) does to its rows."""
import threading

import numpy as np
import pytest

from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.runtime.scheduler import GenRequest, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

V = 512
EOS = 2
MAX_CTX = 64
PROMPT = [1] + list(range(100, 119))          # 20 tokens


@pytest.fixture(scope="module")
def tok():
    t, s, ty = synthetic_vocab(V)
    return SpmTokenizer(t, s, ty, 1, EOS)


def nxt(ctx):
    return 40 + (len(ctx) * 7 + sum(ctx[-2:])) % 200


class Fake:
    """the engine surface the scheduler uses (plain steps: no pipelined calls); log: every call in order"""

    def __init__(self, shift=True):
        self.ctx = {}
        self.log = []
        if shift:
            self.shift_context = self._shift_context

    def prefill(self, slot, ids, start=0, want_logits=True):
        self.log.append(("prefill", slot, len(ids), start))
        self.ctx[slot] = self.ctx.get(slot, [])[:start] + list(ids)
        self._slot = slot
        return np.zeros(V, np.float32)

    def sample_first(self, pos, temperature, top_k, top_p, seed, mask):
        return nxt(self.ctx[self._slot])

    def _step(self, kind, slots, toks, pos):
        self.log.append((kind, list(slots), list(toks), list(pos)))
        for s, t, p in zip(slots, toks, pos):
            assert 0 <= p < MAX_CTX and p <= len(self.ctx[s]), (p, len(self.ctx[s]))
            self.ctx[s] = self.ctx[s][:p] + [t]

    def decode(self, slots, toks, pos, temps, topk, seed, mask, topp, seeds):
        self._step("decode", slots, toks, pos)
        return [nxt(self.ctx[s]) for s in slots]

    def _shift_context(self, slot, n_tokens, n_keep, n_discard):
        self.log.append(("shift", slot, n_tokens, n_keep, n_discard))
        if not (1 <= n_tokens <= MAX_CTX and n_keep >= 0 and n_discard >= 1 and n_keep + n_discard <= n_tokens):
            raise RuntimeError("shift_context: bad arguments")
        c = self.ctx[slot][:n_tokens]
        self.ctx[slot] = c[:n_keep] + c[n_keep + n_discard:]
        return n_tokens - n_discard


class PipedFake(Fake):
    """the same with the pipelined calls: a submit without tokens continues from the token the sampler left"""

    def __init__(self, shift=True):
        super().__init__(shift)
        self._dev, self._rows, self.in_flight = [], [], False

    def decode_submit(self, slots, toks, pos, temps, topk, seed, topp, seeds):
        self._step("submit" if toks else "submit_dev", slots, toks or self._dev, pos)
        self._rows = list(slots)

    def decode_sample(self, mask=b""):
        self._dev = [nxt(self.ctx[s]) for s in self._rows]
        self.in_flight = True

    def decode_collect(self):
        self.in_flight = False
        return list(self._dev)

    def _shift_context(self, *a):
        assert not self.in_flight, "shift_context while a pipelined step is in flight"
        return super()._shift_context(*a)


def run(tok, eng, reqs, **kw):
    sched = Scheduler(eng, tok, max_batch=4, max_slots=2, max_ctx=MAX_CTX, grammar=None, **kw)
    evs, box = [threading.Event() for _ in reqs], {}
    try:
        for i, r in enumerate(reqs):
            r.on_done = lambda res, i=i: (box.__setitem__(i, res), evs[i].set())
            sched.submit(r)
            assert evs[i].wait(30)
    finally:
        sched.close()
    return [box[i] for i in range(len(reqs))], sched


def req(**kw):
    kw.setdefault("prompt_ids", list(PROMPT))
    kw.setdefault("stop_ids", [])
    return GenRequest(**kw)


def expected(n_keep, max_tokens):
    """the tokens and the shifts of a run, from the rule alone: the slot's token list, llama.cpp's numbers"""
    ctx, out, shifts = list(PROMPT), [], []
    out.append(nxt(ctx))
    while len(out) < max_tokens:
        if len(ctx) + 1 >= MAX_CTX:               # the window: the step behind this one would not fit
            n_past = len(ctx)
            d = (n_past - n_keep) // 2
            if d < 1:
                break
            shifts.append((n_past, n_keep, d))
            ctx = ctx[:n_keep] + ctx[n_keep + d:]
        ctx.append(out[-1])
        out.append(nxt(ctx))
    return out, shifts


@pytest.mark.parametrize("engine_cls", [Fake, PipedFake])
@pytest.mark.parametrize("n_keep", [-1, 4, 0, 1000])
def test_shift_gives_every_token(tok, engine_cls, n_keep):
    eng = engine_cls()
    want_keep = len(PROMPT) if n_keep < 0 else min(n_keep, len(PROMPT))
    want, shifts = expected(want_keep, 150)
    (res,), sched = run(tok, eng, [req(max_tokens=150, context_shift=True, n_keep=n_keep)])
    assert res.finish_reason == "length" and res.completion_tokens == 150  # more than the window, not clamped
    assert res.token_ids == want
    calls = [c for c in eng.log if c[0] == "shift"]
    assert [c[2:] for c in calls] == shifts and len(shifts) >= 3
    assert all(c[3] == want_keep and c[4] == (c[2] - want_keep) // 2 for c in calls)   # llama.cpp's numbers
    assert res.context_shifts == len(shifts) == sched.stats["context_shifts"]
    assert sched.stats["shifted_tokens"] == sum(n - k - d for n, k, d in shifts)
    # the step behind every shift is host-fed, at the new position, with the last sampled token
    for i, c in enumerate(eng.log):
        if c[0] == "shift":
            nx = eng.log[i + 1]
            assert nx[0] in ("decode", "submit") and nx[3] == [c[2] - c[4]] and len(nx[2]) == 1
    # the slot's record of cached tokens: the first n_keep prompt tokens, and nothing behind them
    assert sched.slot_cache[0] == PROMPT[:want_keep]


@pytest.mark.parametrize("engine_cls", [Fake, PipedFake])
def test_next_request_reuses_at_most_n_keep(tok, engine_cls):
    eng = engine_cls()
    (a, b), sched = run(tok, eng, [req(max_tokens=100, context_shift=True, n_keep=6), req(max_tokens=3)])
    assert a.context_shifts >= 1 and b.cached_prompt_tokens == 6
    pre = [c for c in eng.log if c[0] == "prefill"]
    assert pre[-1] == ("prefill", 0, len(PROMPT) - 6, 6)


@pytest.mark.parametrize("engine_cls", [Fake, PipedFake])
def test_without_the_flag_nothing_changes(tok, engine_cls):
    eng = engine_cls()
    (res,), sched = run(tok, eng, [req(max_tokens=150)])
    # today's behaviour: max_tokens clamped to the window, "length" there, the slot keeps prompt + output
    assert res.finish_reason == "length" and res.completion_tokens == MAX_CTX - len(PROMPT) and res.context_shifts == 0
    assert not [c for c in eng.log if c[0] == "shift"] and sched.stats["context_shifts"] == 0
    want, _ = expected(len(PROMPT), MAX_CTX - len(PROMPT))
    assert res.token_ids == want
    bare = engine_cls(shift=False)
    (res2,), sched2 = run(tok, bare, [req(max_tokens=150)])
    assert res2.token_ids == res.token_ids and bare.log == eng.log      # the same call sequence
    assert sched2.slot_cache[0] == sched.slot_cache[0] == (PROMPT + res.token_ids)[:len(sched.slot_cache[0])]
    assert len(sched.slot_cache[0]) >= MAX_CTX - 2


def test_window_reached_with_nothing_to_drop_ends_length(tok):
    """n_keep covers everything the slot holds: n_discard < 1"""
    eng = Fake()
    long_prompt = [1] + list(range(100, 100 + MAX_CTX - 2))         # 63 tokens: the first sampled token fills the window
    (res,), _ = run(tok, eng, [req(prompt_ids=long_prompt, max_tokens=10, context_shift=True)])
    assert res.finish_reason == "length" and res.completion_tokens == 1 and res.context_shifts == 0


def test_engine_without_shift_context_gives_error(tok):
    eng = Fake(shift=False)
    (res,), sched = run(tok, eng, [req(max_tokens=150, context_shift=True)])
    assert res.finish_reason == "error" and "context_shift" in res.error and res.completion_tokens == 0
    assert not sched.can_shift


def test_pool_exhausted_falls_back_to_length(tok):
    class Full(Fake):
        def _shift_context(self, *a):
            self.log.append(("shift",) + a)
            raise RuntimeError("paged KV: pool exhausted")

    eng = Full()
    (res,), _ = run(tok, eng, [req(max_tokens=150, context_shift=True)])
    assert res.finish_reason == "length" and res.completion_tokens == MAX_CTX - len(PROMPT) and res.context_shifts == 0


def test_tier_default(tok):
    eng = Fake()
    (res,), sched = run(tok, eng, [req(max_tokens=100)], context_shift=True)
    assert res.completion_tokens == 100 and res.context_shifts >= 1
    bare = Fake(shift=False)                                          # a tier that cannot: the default is dropped
    (res,), sched = run(tok, bare, [req(max_tokens=100)], context_shift=True)
    assert res.finish_reason == "length" and res.completion_tokens == MAX_CTX - len(PROMPT)
