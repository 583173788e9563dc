"""The scheduler's speculative step on a stub engine (no device, no model): the engine's next token is a
scripted function of the tokens before it, spec_decode is the accept rule of tests/spec_oracle.py over that
function, and plain decode is the same function one token at a time -- so a run with speculation on must give
the tokens, text and finish reason of the run with it off, in fewer engine steps."""
import logging
import threading

import numpy as np
import pytest

import spec_oracle as O
from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.runtime.scheduler import GenRequest, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

V = 512
EOS = 2
PATTERN = [40, 41, 42, 43, 44, 45, 46]
PROMPT = [1] + PATTERN * 3 + PATTERN[:2]      # 24 tokens; the model goes on with the pattern
MASK_BYTES = (V + 7) // 8


@pytest.fixture(scope="module")
def tok():
    t, s, ty = synthetic_vocab(V)
    return SpmTokenizer(t, s, ty, 1, EOS)


def cycle(ctx):
    """the pattern forever: every draft is right"""
    return PATTERN[(len(ctx) - 1) % len(PATTERN)]


def bumpy(ctx):
    """the pattern, but every 5th position says something else: drafts are cut short there"""
    return 200 + len(ctx) % 50 if len(ctx) % 5 == 0 else cycle(ctx)


class Stub:
    """the engine surface the scheduler uses, without the pipelined calls (the scheduler then steps plainly)"""

    def __init__(self, nxt, spec=True):
        self.nxt = nxt
        self.ctx = {}
        self.spec_calls = []      # (tokens, pos0, masks, rows decoding at that moment)
        self.decode_rows = []     # rows of every plain step
        self.sched = None
        if spec:
            self.spec_decode = self._spec_decode

    def prefill(self, slot, ids, start=0, want_logits=True):
        self.ctx[slot] = self.ctx.get(slot, [])[:start] + list(ids)
        self._slot = slot
        return np.zeros(V, np.float32)

    def sample_first(self, pos, temperature, top_k, top_p, seed, mask):
        return self.nxt(self.ctx[self._slot])

    def decode(self, slots, toks, pos, temps, topk, seed, mask, topp, seeds):
        self.decode_rows.append(len(slots))
        out = []
        for s, t, p in zip(slots, toks, pos):
            self.ctx[s] = self.ctx[s][:p] + [t]
            out.append(self.nxt(self.ctx[s]))
        return out

    def _spec_decode(self, slot, tokens, pos0, temperature, top_k, top_p, seed, masks):
        base = self.ctx[slot][:pos0]
        outs = [self.nxt(base + list(tokens[:i + 1])) for i in range(len(tokens))]
        n, emitted = O.accept(tokens, outs)
        self.ctx[slot] = base + list(tokens[:n + 1])
        self.spec_calls.append((list(tokens), pos0, bytes(masks), len(self.sched.active) if self.sched else -1))
        return n, emitted


class PipedStub(Stub):
    """the same with the pipelined calls, as every device engine has them: the scheduler queues step t + 1's
    forward (from the token the sampler left on the device) before it has collected step t's token"""

    def __init__(self, nxt, spec=True):
        super().__init__(nxt, spec)
        self.host_fed = 0         # submits that carried host tokens (a batch's first step, or after a drain)
        self._dev, self._out, self._rows = [], [], []

    def decode_submit(self, slots, toks, pos, temps, topk, seed, topp, seeds):
        if not slots:
            raise RuntimeError("decode_submit: batch out of range")
        self.host_fed += bool(toks)
        for s, t, p in zip(slots, toks or self._dev, pos):
            self.ctx[s] = self.ctx[s][:p] + [t]
        self._rows = list(slots)

    def decode_sample(self, mask=b""):
        self.decode_rows.append(len(self._rows))
        self._dev = [self.nxt(self.ctx[s]) for s in self._rows]
        self._out = list(self._dev)

    def decode_collect(self):
        return list(self._out)

    def _spec_decode(self, slot, tokens, *a):
        n, emitted = super()._spec_decode(slot, tokens, *a)
        self._dev = [emitted[-1]]
        return n, emitted


def run(tok, nxt, reqs, spec_engine=True, grammar=None, max_ctx=128, engine_cls=None, **sched_kw):
    eng = (engine_cls or Stub)(nxt, spec_engine)
    sched = Scheduler(eng, tok, max_batch=8, max_slots=2, max_ctx=max_ctx, grammar=grammar, **sched_kw)
    eng.sched = sched
    evs, box = [threading.Event() for _ in reqs], {}
    try:
        with sched.cv:
            for i, r in enumerate(reqs):
                r.on_done = lambda res, i=i: (box.__setitem__(i, res), evs[i].set())
                sched.submit(r)
        for e in evs:
            assert e.wait(30)
    finally:
        sched.close()
    return [box[i] for i in range(len(reqs))], eng, sched


def req(**kw):
    kw.setdefault("prompt_ids", list(PROMPT))
    kw.setdefault("max_tokens", 30)
    kw.setdefault("stop_ids", [])
    return GenRequest(**kw)


def same(a, b):
    assert (a.token_ids, a.text, a.finish_reason) == (b.token_ids, b.text, b.finish_reason)


@pytest.mark.parametrize("nxt", [cycle, bumpy])
def test_same_output_fewer_steps_and_the_stats(tok, nxt):
    (off,), e0, s0 = run(tok, nxt, [req(speculative=False)])
    (on,), e1, s1 = run(tok, nxt, [req(speculative=True)])
    same(on, off)
    assert off.completion_tokens == 30 and e0.spec_calls == [] and s0.stats["spec_steps"] == 0
    assert (off.draft_tokens, off.accepted_draft_tokens) == (0, 0) and s0.metrics()["spec_accept_rate"] == 0.0
    calls = e1.spec_calls
    drafted = sum(len(t) - 1 for t, _, _, _ in calls)
    # accepted drafts: every emitted token but one per engine step (and the first, sampled by the prefill)
    accepted = on.completion_tokens - 1 - len(calls) - len(e1.decode_rows)
    st = s1.stats
    assert calls and (st["spec_steps"], st["spec_drafted"], st["spec_accepted"]) == (len(calls), drafted, accepted)
    assert (on.draft_tokens, on.accepted_draft_tokens) == (drafted, accepted)
    assert s1.metrics()["spec_accept_rate"] == pytest.approx(accepted / drafted)
    assert st["steps"] == len(calls) + len(e1.decode_rows) < s0.stats["steps"] and st["tokens"] == s0.stats["tokens"]
    if nxt is cycle:
        assert accepted == drafted
    else:
        assert 0 < accepted < drafted
    assert all(2 <= len(t) <= 8 for t, _, _, _ in calls)        # draft_max 7 by default
    # the tier's default serves a request that says nothing; the request's word wins over the tier's
    (dflt,), e2, _ = run(tok, nxt, [req()], speculative=dict(mode="lookup", draft_max=3))
    same(dflt, off)
    assert e2.spec_calls and max(len(t) for t, _, _, _ in e2.spec_calls) == 4
    (no,), e3, _ = run(tok, nxt, [req(speculative=False)], speculative=dict(mode="lookup"))
    same(no, off)
    assert e3.spec_calls == []


def test_prediction_is_a_draft_source(tok):
    """a prompt with nothing to look up: only the prediction's tokens can be drafted"""
    prompt = [1, 300, 301, 302, 40, 41]
    pred = PATTERN * 3
    (off,), _, _ = run(tok, cycle, [req(prompt_ids=prompt, speculative=False, max_tokens=12)])
    (on,), e, _ = run(tok, cycle, [req(prompt_ids=prompt, speculative=True, prediction_ids=pred, max_tokens=12)])
    same(on, off)
    first = e.spec_calls[0][0]      # the last token, then what follows it in the prediction
    assert first[1:] == pred[pred.index(first[0]) + 1:][:7] and len(first) == 8
    assert on.accepted_draft_tokens > 0
    (none,), e, _ = run(tok, cycle, [req(prompt_ids=prompt, speculative=True, max_tokens=3)])
    assert e.spec_calls == [] and none.token_ids == off.token_ids[:3]      # (without it: nothing to draft from yet)


def test_eos_ends_the_request_inside_a_run(tok):
    def nxt(ctx):
        return EOS if len(ctx) == len(PROMPT) + 9 else cycle(ctx)

    (off,), _, _ = run(tok, nxt, [req(speculative=False)])
    (on,), e, _ = run(tok, nxt, [req(speculative=True)])
    same(on, off)
    assert on.finish_reason == "stop" and on.completion_tokens == 9
    assert all(EOS not in t for t, _, _, _ in e.spec_calls)
    # a stop id among the drafted tokens cuts the draft in front of it
    (off,), _, _ = run(tok, cycle, [req(speculative=False, stop_ids=[44])])
    (on,), e, _ = run(tok, cycle, [req(speculative=True, stop_ids=[44])])
    same(on, off)
    assert on.finish_reason == "stop" and all(44 not in t[1:] for t, _, _, _ in e.spec_calls)


def test_max_tokens_and_context_clips(tok):
    for mt in (2, 3, 7):
        (off,), _, _ = run(tok, cycle, [req(speculative=False, max_tokens=mt)])
        (on,), e, _ = run(tok, cycle, [req(speculative=True, max_tokens=mt)])
        same(on, off)
        assert on.completion_tokens == mt and on.finish_reason == "length"
        for t, pos0, _, _ in e.spec_calls:     # rows never run past the request's last token
            assert (pos0 - len(PROMPT) + 1) + len(t) <= mt
    ctx = len(PROMPT) + 9
    (off,), _, _ = run(tok, cycle, [req(speculative=False, max_tokens=100)], max_ctx=ctx)
    (on,), e, _ = run(tok, cycle, [req(speculative=True, max_tokens=100)], max_ctx=ctx)
    same(on, off)
    assert on.finish_reason == "length" and e.spec_calls
    assert all(pos0 + len(t) <= ctx - 1 for t, pos0, _, _ in e.spec_calls)
    # above spec_max_context no draft is tried
    (_,), e, _ = run(tok, cycle, [req(speculative=True)], speculative=dict(max_context=len(PROMPT) + 3))
    assert e.spec_calls and all(pos0 + 1 <= len(PROMPT) + 3 for _, pos0, _, _ in e.spec_calls)


class _State:
    def __init__(self, toks=()):
        self.toks = list(toks)

    def copy(self):
        return _State(self.toks)


class FakeGrammar:
    """a grammar that rejects `banned`, is complete after `closer`, and whose masks name their state"""

    def __init__(self, banned=(), closer=None):
        self.banned, self.closer = set(banned), closer

    def initial(self):
        return _State()

    def accept_token(self, st, tok):
        if tok in self.banned:
            return False
        st.toks.append(tok)
        return True

    def complete(self, st):
        return bool(st.toks) and st.toks[-1] == self.closer

    def mask(self, st):
        return bytes([len(st.toks) % 256, 0]) + b"\xff" * (MASK_BYTES - 2)

    def mask_open(self, st):
        return bytes([len(st.toks) % 256, 1]) + b"\xff" * (MASK_BYTES - 2)


SEQ = [40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 250, 52, 53]
STOP_TOK = 250


def seq_cycle(ctx):
    return SEQ[(len(ctx) - 1) % len(SEQ)]


@pytest.mark.parametrize("kind", ["rejects", "completes"])
def test_grammar_cuts_the_draft_and_masks_are_per_row(tok, kind):
    """the model repeats its prompt, whose 13th token the grammar rejects (or is complete behind): the lookup
    proposes it, the scheduler cuts the draft in front of it, and the model's own sample of it ends the request"""
    g = dict(banned=[STOP_TOK]) if kind == "rejects" else dict(closer=STOP_TOK)
    prompt = [1] + SEQ + SEQ[:2]
    n0 = len(prompt)
    kw = dict(prompt_ids=prompt, json_mode=True, min_tokens=6, max_tokens=40)
    (off,), _, _ = run(tok, seq_cycle, [req(speculative=False, **kw)], grammar=FakeGrammar(**g))
    (on,), e, _ = run(tok, seq_cycle, [req(speculative=True, **kw)], grammar=FakeGrammar(**g),
                      speculative=dict(draft_max=7))
    same(on, off)
    assert on.finish_reason == ("stop" if kind == "rejects" else "grammar")
    assert on.token_ids == SEQ[2:12] + ([] if kind == "rejects" else [STOP_TOK])
    assert e.spec_calls and all(STOP_TOK not in t[1:] for t, _, _, _ in e.spec_calls)
    assert sum(len(t) - 1 for t, _, _, _ in e.spec_calls) == on.accepted_draft_tokens > 0   # what was left was right
    for t, pos0, masks, _ in e.spec_calls:
        R, done = len(t), pos0 - n0 + 1          # tokens generated (and accepted by the grammar) before this step
        assert len(masks) == R * MASK_BYTES
        for i in range(R):
            row = masks[i * MASK_BYTES:(i + 1) * MASK_BYTES]
            assert row[0] == done + i                                   # the state behind drafts 0..i-1
            assert row[1] == (1 if done + i + 1 < 6 else 0)             # min_tokens counted per row
    opens = [m[i * MASK_BYTES + 1] for _, _, m, _ in e.spec_calls for i in range(len(m) // MASK_BYTES)]
    assert 0 in opens and 1 in opens
    assert max(len(t) for t, _, _, _ in e.spec_calls) > 2


def test_two_decoding_rows_take_plain_steps(tok):
    a, b = req(speculative=True, max_tokens=12), req(speculative=True, max_tokens=12, prompt_ids=PROMPT[:-1])
    (ra, rb), e, s = run(tok, cycle, [a, b])
    assert ra.completion_tokens == rb.completion_tokens == 12
    assert e.spec_calls == [] and s.stats["spec_steps"] == 0 and set(e.decode_rows) == {2}
    # one of them longer: it speculates once it is alone, never before
    a, b = req(speculative=True, max_tokens=30), req(speculative=True, max_tokens=6, prompt_ids=PROMPT[:-1])
    (ra, rb), e, s = run(tok, cycle, [a, b])
    (alone,), _, _ = run(tok, cycle, [req(speculative=False, max_tokens=30)])
    same(ra, alone)
    assert e.spec_calls and all(n_active == 1 for _, _, _, n_active in e.spec_calls)
    assert all(pos0 >= len(PROMPT) + 5 for _, pos0, _, _ in e.spec_calls)


def test_engine_without_spec_decode_decodes_plainly_and_says_so_once(tok, caplog):
    with caplog.at_level(logging.WARNING, logger="aios.runtime.scheduler"):
        (r1, r2), e, s = run(tok, cycle, [req(speculative=True, max_tokens=8),
                                          req(speculative=True, prediction_ids=list(PATTERN), max_tokens=8)],
                             spec_engine=False)
    assert r1.completion_tokens == r2.completion_tokens == 8
    assert (r1.draft_tokens, r1.accepted_draft_tokens, s.stats["spec_steps"]) == (0, 0, 0)
    assert len([m for m in caplog.messages if "spec_decode" in m]) == 1


def test_bad_tier_settings_are_refused(tok):
    for bad in (dict(mode="tree"), dict(draft_max=8), dict(draft_max=0), dict(ngram_min=3, ngram_max=2), dict(rows=4),
                dict(max_context=0), dict(ngram_max=9)):
        with pytest.raises(ValueError):
            Scheduler(Stub(cycle), tok, max_batch=8, max_slots=2, max_ctx=64, speculative=bad).close()


def fresh(ctx):
    """text that never repeats: nothing is ever drafted"""
    return 100 + len(ctx)


def healthy(sched):
    assert sched.failed == "" and sched.stats["errors"] == 0


@pytest.mark.parametrize("nxt", [fresh, cycle, bumpy])
def test_pipelined_engine_every_request_length(tok, nxt):
    """a pipelined engine: whichever step the request's last token comes from -- a speculative one, a plain
    one, or the in-flight one collected while looking for a draft -- the scheduler makes no further engine call
    for it and the tier stays healthy"""
    for mt in range(1, 13):
        (off,), e0, s0 = run(tok, nxt, [req(speculative=False, max_tokens=mt)], engine_cls=PipedStub)
        (on,), e1, s1 = run(tok, nxt, [req(speculative=True, max_tokens=mt)], engine_cls=PipedStub)
        assert s0.pipeline and s1.pipeline
        same(on, off)
        assert on.completion_tokens == mt and on.finish_reason == "length"
        healthy(s0)
        healthy(s1)
        if nxt is fresh:
            assert e1.spec_calls == []
        elif mt > 4:
            assert e1.spec_calls


@pytest.mark.parametrize("base", [fresh, cycle, bumpy])
def test_pipelined_engine_eos_on_every_token(tok, base):
    for k in range(1, 12):
        def nxt(ctx, k=k):
            return EOS if len(ctx) == len(PROMPT) + k - 1 else base(ctx)

        (off,), _, s0 = run(tok, nxt, [req(speculative=False)], engine_cls=PipedStub)
        (on,), _, s1 = run(tok, nxt, [req(speculative=True)], engine_cls=PipedStub)
        same(on, off)
        assert on.finish_reason == "stop" and on.completion_tokens == k - 1
        healthy(s0)
        healthy(s1)


def test_text_that_does_not_repeat_stays_pipelined(tok):
    """no in-flight step is collected early while nothing can be drafted: the speculating request makes the
    plain request's engine calls, host-fed submits included"""
    (off,), e0, _ = run(tok, fresh, [req(speculative=False, max_tokens=20)], engine_cls=PipedStub)
    (on,), e1, s1 = run(tok, fresh, [req(speculative=True, max_tokens=20)], engine_cls=PipedStub)
    same(on, off)
    assert e1.host_fed == e0.host_fed == 1 and e1.decode_rows == e0.decode_rows and e1.spec_calls == []
    healthy(s1)
    # text that does repeat: steps are collected early, drafts run, and the output is the same
    (off,), e0, _ = run(tok, cycle, [req(speculative=False, max_tokens=20)], engine_cls=PipedStub)
    (on,), e1, s1 = run(tok, cycle, [req(speculative=True, max_tokens=20)], engine_cls=PipedStub)
    same(on, off)
    assert e1.spec_calls and len(e1.spec_calls) + len(e1.decode_rows) < len(e0.decode_rows)
    healthy(s1)


def test_tensor_parallel_proxy_is_a_tier_without_spec_decode(tok, caplog):
    from aios_amd.parallel.tp import TPEngine

    shard = Stub(cycle)
    assert hasattr(shard, "spec_decode")
    eng = TPEngine(shard, comm=type("Comm", (), {"error": staticmethod(lambda: False)})(), send=lambda msg: None)
    assert not hasattr(eng, "spec_decode")
    sched = Scheduler(eng, tok, max_batch=8, max_slots=2, max_ctx=128, speculative=dict(mode="lookup"))
    assert not sched.can_spec
    import threading as th
    ev, box = th.Event(), {}
    r = req(max_tokens=8, prediction_ids=list(PATTERN))
    r.on_done = lambda res: (box.__setitem__(0, res), ev.set())
    with caplog.at_level(logging.WARNING, logger="aios.runtime.scheduler"):
        try:
            sched.submit(r)
            assert ev.wait(30)
        finally:
            sched.close()
    assert box[0].completion_tokens == 8 and (box[0].draft_tokens, box[0].accepted_draft_tokens) == (0, 0)
    assert shard.spec_calls == [] and len([m for m in caplog.messages if "spec_decode" in m]) == 1
    healthy(sched)
