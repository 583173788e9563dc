"""The scheduler's multi-sequence speculative step on a stub engine (no device, no model), in the style of
tests/test_spec_scheduler.py, whose stubs it extends: the engine's next token is a scripted function of the
tokens before it, spec_decode_multi is the segmented accept rule of tests/spec_multi_oracle.py over that function,
and plain decode is the same function one token at a time -- so concurrent requests with speculation on must
return the tokens, text and finish reason they return with it off."""
import threading

import pytest

import spec_multi_oracle as M
import spec_oracle as O
from aios_amd.runtime.scheduler import Scheduler
from test_spec_scheduler import EOS, PATTERN, PROMPT, PipedStub, Stub, bumpy, cycle, healthy, req, same
from test_spec_scheduler import tok  # noqa: F401  (the module's tokenizer fixture)

# three prompts of different lengths that tell themselves apart by their second token; each goes on with the
# pattern, as test_spec_scheduler's PROMPT does
PROMPTS = [[1, 300 + i] + PATTERN[1:] + PATTERN * 2 + PATTERN[:k] for i, k in enumerate((2, 1, 5))]
assert all(cycle(p) == PATTERN[k] for p, k in zip(PROMPTS, (2, 1, 5))) and len(PROMPTS[0]) == len(PROMPT)


class MultiMixin:
    def _init_multi(self):
        self.multi_calls = []    # dict(slots, tokens, pos0, masks, emitted) per spec_decode_multi
        self.calls = []          # the order of the engine's decoding calls, by name

    def spec_decode_multi(self, slots, tokens, pos0, temperature, top_k, top_p, seeds, masks):
        assert len(set(slots)) == len(slots) == len(tokens) == len(pos0) == len(temperature) == len(top_k) == len(seeds)
        assert 1 <= len(slots) <= 8 and all(1 <= len(t) <= 8 for t in tokens) and sum(map(len, tokens)) <= 32
        flat_in, flat_out = [], []
        for slot, t, p in zip(slots, tokens, pos0):
            assert p == len(self.ctx[slot])            # the segment starts where the slot's context ends
            flat_in += list(t)
            flat_out += [self.nxt(self.ctx[slot] + list(t[:i + 1])) for i in range(len(t))]
        res = M.accept(flat_in, flat_out, M.segments([len(t) for t in tokens]))
        for slot, t, (n, _) in zip(slots, tokens, res):
            self.ctx[slot] = self.ctx[slot] + list(t[:n + 1])
        self.multi_calls.append(dict(slots=list(slots), tokens=[list(t) for t in tokens], pos0=list(pos0),
                                     ctx=[list(self.ctx[slot][:p]) for slot, p in zip(slots, pos0)],
                                     masks=bytes(masks), emitted=[list(o) for _, o in res]))
        self.calls.append("multi")
        return res


class MultiStub(MultiMixin, Stub):
    def __init__(self, nxt, spec=True):
        Stub.__init__(self, nxt, spec)
        self._init_multi()

    def decode(self, slots, *a):
        self.calls.append("decode%d" % len(slots))
        return Stub.decode(self, slots, *a)

    def _spec_decode(self, slot, tokens, *a):
        self.calls.append("spec")
        return Stub._spec_decode(self, slot, tokens, *a)


class NoMultiStub(MultiStub):
    """the engine of the parent commit: no spec_decode_multi"""
    spec_decode_multi = property()   # hasattr() is False


class PipedMultiStub(MultiMixin, PipedStub):
    def __init__(self, nxt, spec=True):
        PipedStub.__init__(self, nxt, spec)
        self._init_multi()

    def spec_decode_multi(self, slots, tokens, *a):
        res = MultiMixin.spec_decode_multi(self, slots, tokens, *a)
        self._dev = [o[-1] for _, o in res]      # rows 0..S-1 of the step state: the sequences' last tokens
        self._rows = list(slots)
        return res


def run(tok, nxt, reqs, engine_cls=MultiStub, max_batch=16, max_slots=4, max_ctx=128, **sched_kw):
    eng = engine_cls(nxt, True)
    sched = Scheduler(eng, tok, max_batch=max_batch, max_slots=max_slots, max_ctx=max_ctx, **sched_kw)
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


def expected(c, nxt, max_tokens, cap=16, rows_max=8):
    """the segments of call c by the rule: per sequence its last token and the lookup's draft behind it, clipped
    to the request's end, then the longest draft (the first among equals) gives up its last token until the
    rows fit the cap"""
    drafts = []
    for ctx in c["ctx"]:
        i = ctx[1] - 300
        made = len(ctx) + 1 - len(PROMPTS[i])       # tokens generated so far, the segment's first included
        lim = max(0, min(max_tokens[i] - made - 1, rows_max - 1))
        drafts.append(O.lookup_draft(ctx + [nxt(ctx)], draft_max=7)[:lim])
    while len(drafts) + sum(map(len, drafts)) > cap:
        max(drafts, key=len).pop()
    return [[nxt(ctx)] + d for ctx, d in zip(c["ctx"], drafts)]


def alone(tok, nxt, **kw):
    (r,), _, _ = run(tok, nxt, [req(speculative=False, **kw)], engine_cls=Stub)
    return r


@pytest.mark.parametrize("nxt", [cycle, bumpy])
@pytest.mark.parametrize("n", [2, 3])
def test_concurrent_requests_take_multi_steps_with_the_expected_segments(tok, nxt, n):
    reqs = [req(speculative=True, prompt_ids=PROMPTS[i], max_tokens=30 - 12 * i) for i in range(n)]
    res, e, s = run(tok, nxt, reqs)
    for i, r in enumerate(res):
        same(r, alone(tok, nxt, prompt_ids=PROMPTS[i], max_tokens=30 - 12 * i))
    calls = e.multi_calls
    assert calls and len(calls[0]["slots"]) == n
    for c in calls:
        assert c["tokens"] == expected(c, nxt, [30 - 12 * i for i in range(3)])
        assert sum(len(t) for t in c["tokens"]) <= 16 and c["masks"] == b""
        assert any(len(t) > 1 for t in c["tokens"])               # never a step without a draft
    # once one request is left it speculates alone, through spec_decode
    if n == 2:
        assert e.spec_calls and e.calls.index("spec") > max(i for i, c in enumerate(e.calls) if c == "multi")
    st = s.stats
    drafted = sum(len(t) - 1 for c in calls for t in c["tokens"]) + sum(len(t) - 1 for t, _, _, _ in e.spec_calls)
    accepted = sum(len(o) - 1 for c in calls for o in c["emitted"])
    assert st["spec_multi_steps"] == len(calls) and st["spec_steps"] == len(calls) + len(e.spec_calls)
    assert st["spec_drafted"] == drafted == sum(r.draft_tokens for r in res)
    assert st["spec_accepted"] == sum(r.accepted_draft_tokens for r in res) >= accepted > 0
    assert st["steps"] == len(calls) + len(e.spec_calls) + len(e.decode_rows)
    assert st["batch_sum"] == sum(len(c["slots"]) for c in calls) + len(e.spec_calls) + sum(e.decode_rows)   # S, not Rt
    if nxt is cycle:
        assert st["spec_accepted"] == st["spec_drafted"]
    healthy(s)


def test_a_request_without_speculation_rides_along_as_one_row(tok):
    reqs = [req(speculative=False, prompt_ids=PROMPTS[0], max_tokens=20),
            req(speculative=True, prompt_ids=PROMPTS[1], max_tokens=20)]
    (plain, spec), e, s = run(tok, cycle, reqs)
    same(plain, alone(tok, cycle, prompt_ids=PROMPTS[0], max_tokens=20))
    same(spec, alone(tok, cycle, prompt_ids=PROMPTS[1], max_tokens=20))
    assert e.multi_calls and all(len(c["tokens"][0]) == 1 and len(c["tokens"][1]) > 1 for c in e.multi_calls)
    assert (plain.draft_tokens, plain.accepted_draft_tokens) == (0, 0) and spec.accepted_draft_tokens > 0
    # a context past spec_max_context rides along the same way
    reqs = [req(speculative=True, prompt_ids=PROMPTS[0], max_tokens=12), req(speculative=True, prompt_ids=PROMPTS[2], max_tokens=12)]
    _, e, _ = run(tok, cycle, reqs, speculative=dict(max_context=len(PROMPTS[2]) + 4))
    assert e.multi_calls
    for c in e.multi_calls:
        for t, p0 in zip(c["tokens"], c["pos0"]):
            assert len(t) == 1 or p0 + 1 <= len(PROMPTS[2]) + 4


def test_drafts_are_trimmed_longest_first_to_the_row_cap(tok):
    # max_batch 8, three sequences with 7 drafts each: 5 draft rows are left, taken off the longest in turn
    reqs = [req(speculative=True, prompt_ids=PROMPTS[i], max_tokens=30) for i in range(3)]
    res, e, s = run(tok, cycle, reqs, max_batch=8)
    for i, r in enumerate(res):
        same(r, alone(tok, cycle, prompt_ids=PROMPTS[i], max_tokens=30))
    assert [len(t) for t in e.multi_calls[0]["tokens"]] == [2, 3, 3]
    for c in e.multi_calls:
        assert c["tokens"] == expected(c, cycle, [30] * 3, cap=8, rows_max=8) and sum(len(t) for t in c["tokens"]) <= 8
    # a short draft keeps its tokens: only the long ones give theirs up (one draft is left to the first request)
    reqs = [req(speculative=True, prompt_ids=PROMPTS[0], max_tokens=4)] + \
           [req(speculative=True, prompt_ids=PROMPTS[i], max_tokens=30) for i in (1, 2)]
    res, e, s = run(tok, cycle, reqs, max_batch=8)
    three = [c for c in e.multi_calls if len(c["slots"]) == 3]
    assert three and all(c["tokens"] == expected(c, cycle, [4, 30, 30], cap=8) for c in e.multi_calls)
    assert [len(t) for t in three[-1]["tokens"]] == [2, 3, 3]
    # the engine's cap of 32 rows: 8 sequences, max_batch 64 -- 24 draft rows, 3 each
    reqs = [req(speculative=True, prompt_ids=PROMPTS[i % 3][:8] + PATTERN * (i // 3) + PROMPTS[i % 3][8:], max_tokens=60) for i in range(8)]
    res, e, s = run(tok, cycle, reqs, max_batch=64, max_slots=8)
    eight = [c for c in e.multi_calls if len(c["slots"]) == 8]
    assert eight and [len(t) for t in eight[0]["tokens"]] == [4] * 8
    assert all(sum(len(t) for t in c["tokens"]) <= 32 for c in e.multi_calls)
    # as many sequences as rows: nothing to draft with
    reqs = [req(speculative=True, prompt_ids=PROMPTS[i], max_tokens=10) for i in range(2)]
    res, e, s = run(tok, cycle, reqs, max_batch=2)
    assert e.multi_calls == [] and set(e.decode_rows) == {2}


def test_a_request_that_finishes_inside_its_segment_leaves_the_others_alone(tok):
    a = req(speculative=True, prompt_ids=PROMPTS[0], max_tokens=30)
    b = req(speculative=True, prompt_ids=PROMPTS[1], max_tokens=30)
    seen = []

    def on_delta(text):        # the client goes away behind the third token: the next token finds it cancelled
        seen.append(text)
        if len(seen) == 3:
            a.cancelled = True

    a.on_delta = on_delta
    (ra, rb), e, s = run(tok, cycle, [a, b])
    same(rb, alone(tok, cycle, prompt_ids=PROMPTS[1], max_tokens=30))
    full = alone(tok, cycle, prompt_ids=PROMPTS[0], max_tokens=30)
    assert ra.finish_reason == "cancelled" and 0 < len(ra.token_ids) < 8
    assert ra.token_ids == full.token_ids[:len(ra.token_ids)]
    first = e.multi_calls[0]
    assert len(first["emitted"][0]) == 8 > len(ra.token_ids) - 1     # the step emitted more than the request took
    assert all(len(c["slots"]) == 1 or c is first for c in e.multi_calls)   # b went on without it
    healthy(s)
    # an EOS the model samples ends one request; the other's tokens are what they are alone
    def nxt(ctx):
        return EOS if len(ctx) == len(PROMPTS[0]) + 9 else cycle(ctx)

    reqs = [req(speculative=True, prompt_ids=PROMPTS[i], max_tokens=30) for i in range(2)]
    res, e, s = run(tok, nxt, reqs)
    for i, r in enumerate(res):
        same(r, alone(tok, nxt, prompt_ids=PROMPTS[i], max_tokens=30))
    assert e.multi_calls and res[0].finish_reason == "stop"


@pytest.mark.parametrize("how", ["spec_multi_false", "speculation_off"])
def test_switched_off_the_engine_sees_the_parents_calls(tok, how):
    def reqs():
        on = None if how == "spec_multi_false" else False
        return [req(speculative=on, prompt_ids=PROMPTS[i], max_tokens=14 + 5 * i) for i in range(3)]

    kw = dict(speculative=dict(mode="lookup", multi=0)) if how == "spec_multi_false" else dict(speculative=dict(mode="lookup"))
    got, e, s = run(tok, cycle, reqs(), **kw)
    want, p, _ = run(tok, cycle, reqs(), engine_cls=NoMultiStub, speculative=dict(mode="lookup"))
    assert not hasattr(p, "spec_decode_multi")
    for a, b in zip(got, want):
        same(a, b)
    assert e.multi_calls == [] and e.calls == p.calls and s.stats["spec_multi_steps"] == 0
    assert e.spec_calls == p.spec_calls and e.decode_rows == p.decode_rows
    if how == "spec_multi_false":
        assert "spec" in e.calls and "decode3" in e.calls     # (the lone last request still speculates)
    else:
        assert "spec" not in e.calls


def test_one_active_request_takes_the_single_sequence_path(tok):
    (r,), e, s = run(tok, cycle, [req(speculative=True)])
    (p,), q, _ = run(tok, cycle, [req(speculative=True)], engine_cls=NoMultiStub)
    same(r, p)
    assert e.multi_calls == [] and e.spec_calls == q.spec_calls and e.calls == q.calls and "spec" in e.calls
    assert s.stats["spec_multi_steps"] == 0 and s.stats["spec_steps"] == len(e.spec_calls)


@pytest.mark.parametrize("nxt", [cycle, bumpy])
def test_pipelined_engine(tok, nxt):
    """with the pipelined calls the in-flight step is collected before a multi step, and whichever step a
    request's last token comes from, the others go on and the tier stays healthy"""
    for mts in ((1, 9), (5, 5), (12, 4, 7), (2, 3, 30)):
        reqs = [req(speculative=True, prompt_ids=PROMPTS[i], max_tokens=mt) for i, mt in enumerate(mts)]
        res, e, s = run(tok, nxt, reqs, engine_cls=PipedMultiStub)
        assert s.pipeline
        for i, (r, mt) in enumerate(zip(res, mts)):
            same(r, alone(tok, nxt, prompt_ids=PROMPTS[i], max_tokens=mt))
        healthy(s)
        if min(mts) > 4:
            assert e.multi_calls and s.stats["spec_multi_steps"] == len(e.multi_calls)


class ProcStub(MultiStub):
    """the engine with the staging calls: what is staged at a spec_decode_multi call is kept with the call, and
    every sampler launch reports logprobs that name the token of their row (lp = -token / 1000)"""

    def __init__(self, nxt, spec=True):
        MultiStub.__init__(self, nxt, spec)
        self._proc = self._topn = self._last = None

    def set_sample_processors(self, min_p, rep, pres, freq, windows, bias_ids=None, bias_vals=None):
        self._proc = dict(min_p=list(min_p), rep=list(rep), pres=list(pres), freq=list(freq),
                          windows=[list(w) for w in windows], bias_ids=bias_ids, bias_vals=bias_vals)

    def set_logprobs(self, top_n):
        self._topn = list(top_n)

    def _launched(self, toks):
        """a sampler launch over rows that sampled `toks`: one shot for everything staged"""
        assert self._topn is None or len(self._topn) == len(toks)
        assert self._proc is None or len(self._proc["windows"]) == len(toks)
        self._last = list(toks) if self._topn is not None else None
        self._proc = self._topn = None

    def last_logprobs(self):
        if self._last is None:
            return ()
        n = len(self._last)
        return ([-t / 1000.0 for t in self._last], [[t, t + 1, t + 2] + [-1] * 17 for t in self._last],
                [[-1.0, -2.0, -3.0] + [float("-inf")] * 17 for _ in range(n)])

    def sample_first(self, *a):
        t = MultiStub.sample_first(self, *a)
        self._launched([t])
        return t

    def decode(self, slots, *a):
        out = MultiStub.decode(self, slots, *a)
        self._launched(out)
        return out

    def _spec_decode(self, slot, tokens, pos0, *a):
        outs = [self.nxt(self.ctx[slot][:pos0] + list(tokens[:i + 1])) for i in range(len(tokens))]
        res = MultiStub._spec_decode(self, slot, tokens, pos0, *a)
        self._launched(outs)
        return res

    def spec_decode_multi(self, slots, tokens, pos0, *a):
        staged = dict(proc=self._proc, topn=self._topn)
        outs = [self.nxt(self.ctx[s][:p] + list(t[:i + 1])) for s, t, p in zip(slots, tokens, pos0) for i in range(len(t))]
        res = MultiStub.spec_decode_multi(self, slots, tokens, pos0, *a)
        self.multi_calls[-1].update(staged)
        self._launched(outs)
        return res


def test_masks_windows_bias_and_logprobs_per_row_in_segment_order(tok):
    """a JSON-mode request, a penalised and biased request and a logprobs request in the same multi steps: every
    row gets its own mask (the grammar behind the drafts before it), penalty window (the drafts before it behind
    the sequence's tokens), bias list and logprob entry, concatenated in segment order"""
    from test_spec_scheduler import MASK_BYTES, FakeGrammar

    def reqs(spec):
        return [req(speculative=spec, prompt_ids=PROMPTS[0], max_tokens=24, json_mode=True, min_tokens=6),
                req(speculative=spec, prompt_ids=PROMPTS[1], max_tokens=24, repeat_penalty=1.3, logit_bias={5: -1.0}),
                req(speculative=spec, prompt_ids=PROMPTS[2], max_tokens=24, logprobs=True, top_logprobs=2)]

    off, _, _ = run(tok, cycle, reqs(False), engine_cls=ProcStub, grammar=FakeGrammar())
    on, e, s = run(tok, cycle, reqs(True), engine_cls=ProcStub, grammar=FakeGrammar())
    for a, b in zip(on, off):
        same(a, b)
    healthy(s)
    assert on[2].logprobs == off[2].logprobs and len(on[2].logprobs) == 24
    for t, lp, top in on[2].logprobs:       # each emitted token with the entry of ITS row
        assert lp == -t / 1000.0 and top == [(t, -1.0), (t + 1, -2.0)]
    three = [c for c in e.multi_calls if len(c["slots"]) == 3]
    assert three and any(min(len(t) for t in c["tokens"]) > 1 for c in three)    # all three with drafts at once
    full = b"\xff" * MASK_BYTES
    for c in e.multi_calls:
        who = [ctx[1] - 300 for ctx in c["ctx"]]
        Rt = sum(len(t) for t in c["tokens"])
        masks, proc, topn = c["masks"], c["proc"], c["topn"]
        if 0 in who:
            assert len(masks) == Rt * MASK_BYTES
        if 1 in who:
            assert proc is not None and all(len(proc[k]) == Rt for k in ("min_p", "rep", "pres", "freq", "windows"))
            assert len(proc["bias_ids"]) == len(proc["bias_vals"]) == Rt
        if 2 in who:
            assert topn is not None and len(topn) == Rt
        r = 0
        for i, ctx, t in zip(who, c["ctx"], c["tokens"]):
            done = len(ctx) + 1 - len(PROMPTS[i])      # tokens generated (and seen by the grammar) before this step
            for j in range(len(t)):
                if masks:
                    row = masks[(r + j) * MASK_BYTES:(r + j + 1) * MASK_BYTES]
                    if i == 0:
                        assert row[0] == done + j and row[1] == (1 if done + j + 1 < 6 else 0)
                        assert row[2:] == full[2:]
                    else:
                        assert row == full
                if proc is not None:
                    if i == 1:
                        assert proc["rep"][r + j] == 1.3 and proc["windows"][r + j] == (ctx + t[:j + 1])[-64:]
                        assert (proc["bias_ids"][r + j], proc["bias_vals"][r + j]) == ([5], [-1.0])
                    else:
                        assert proc["rep"][r + j] == 1.0 and proc["windows"][r + j] == []
                        assert (proc["bias_ids"][r + j], proc["bias_vals"][r + j]) == ([], [])
                if topn is not None:
                    assert topn[r + j] == (2 if i == 2 else -1)
            r += len(t)
