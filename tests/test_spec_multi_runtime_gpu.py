"""Multi-sequence speculative steps end to end on the device: a real Scheduler (pipelined decode, the engine's
spec_decode_multi) on test-tiny, two concurrent greedy requests on a tier with speculative = "lookup", their
prompts a token pattern repeated and their own plain output as the prediction, so the lookup drafts.

What the tokens are compared with.  (1) The engine-level reference of tests/test_spec_multi_engine_gpu.py, taken
inside the live run: a proxy around the engine copies every sequence's slot to a twin before each
spec_decode_multi call, lets the call run, then runs decode() of the same flat rows on the twins and holds the
call's results to the accept rule (tests/spec_multi_oracle.py) over decode()'s tokens -- the same Rt-row kernels on
both sides, Q4_K_M weights, equality exact.  (2) The run with spec_multi = false and the plain run, token for token.
Equality there needs the compared runs to take batched steps of the same kernels, and on THIS model they do:
measured on the device over the 31 tokens each request generates (test-tiny, Q4_K_M, model seed 10, both prompts),
the logits of a position are bit for bit the same whether it runs in the two requests' 2-row step, as a row of a
4-, 8- or 16-row step of both, or as one of 4 or 8 rows of one request alone (max |difference| 0.0 in each case:
test-tiny's shapes take one set of batched kernels from 2 rows up).  Only the one-row step differs, by at most
0.00158, against a smallest top-2 logit gap of 0.1316 over those tokens: a ratio of 83, above the 10 that
tests/test_spec_runtime_gpu.py asks of the same seed (seeds 4 and 9 gave 52 and 35).  So whichever of the three
schedules a position falls into -- one-row steps while a request is alone, 2-row steps, multi steps -- its greedy
token is the same, and the test asserts it.  That the scheduler hands each sequence's results to the right request
is checked by that equality on the device and, with a scripted engine, by tests/test_spec_multi_scheduler.py.
"""
import threading

import pytest

import spec_multi_oracle as M
from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.runtime.scheduler import GenRequest, Scheduler
from aios_amd.runtime.service import prediction_usage
from aios_amd.runtime.tokenizer import SpmTokenizer

pytestmark = pytest.mark.gpu

PATTERNS = [[60, 61, 62, 63, 64, 65, 66, 67, 68], [90, 91, 92, 93, 94, 95, 96]]
PROMPTS = [[1] + PATTERNS[0] * 4, [1] + PATTERNS[1] * 3]
MAX_TOKENS = 32
MODEL_SEED = 10


class Checked:
    """the engine, with every spec_decode_multi call held to decode() of its rows on twins (slots 2 and 3)"""

    def __init__(self, eng):
        self._eng = eng
        self.calls = []     # (slots, tokens, results)

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def spec_decode_multi(self, slots, tokens, pos0, temperature, top_k, top_p, seeds, masks=b""):
        e = self._eng
        free = [s for s in range(4) if s not in slots][:len(slots)]
        assert len(free) == len(slots)
        for s, t, p in zip(slots, free, pos0):
            e.copy_slot(s, t, p)
        res = e.spec_decode_multi(slots, tokens, pos0, temperature, top_k, top_p, seeds, masks)
        rows = [(t, x, p + i, T, k, pp, sd) for t, toks, p, T, k, pp, sd in
                zip(free, tokens, pos0, temperature, top_k, top_p, seeds) for i, x in enumerate(toks)]
        sl, flat, pos, T, K, P, sd = [list(c) for c in zip(*rows)]
        dec = [int(t) for t in e.decode(sl, flat, pos, T, K, 0, masks, P, sd)]
        want = M.accept(flat, dec, M.segments([len(t) for t in tokens]))
        got = [(int(a), [int(t) for t in o]) for a, o in res]
        assert got == want, (tokens, got, want)
        self.calls.append((list(slots), [list(t) for t in tokens], got))
        return res


@pytest.fixture(scope="module")
def env():
    from aios_amd.runtime.loader import random_engine

    t, s, ty = synthetic_vocab(512)
    eng = random_engine(get_preset("test-tiny"), "Q4_K_M", seed=MODEL_SEED, max_ctx=256, max_slots=4, max_batch=16)
    return eng, SpmTokenizer(t, s, ty, 1, 2)


def run(env, tier, predictions=(None, None), check=False):
    eng, tok = env
    engine = Checked(eng) if check else eng
    # (two of the four slots are the scheduler's: the proxy's twins live in the other two)
    sched = Scheduler(engine, tok, max_batch=16, max_slots=2, max_ctx=256, speculative=tier)
    evs, box = [threading.Event(), threading.Event()], {}
    try:
        with sched.cv:
            for i, (p, pred) in enumerate(zip(PROMPTS, predictions)):
                r = GenRequest(prompt_ids=list(p), max_tokens=MAX_TOKENS, temperature=0.0, stop_ids=[],
                               prediction_ids=pred)
                r.on_done = lambda res, i=i: (box.__setitem__(i, res), evs[i].set())
                sched.submit(r)
        for e in evs:
            assert e.wait(60)
    finally:
        sched.close()
    for i in (0, 1):
        assert box[i].finish_reason != "error", box[i].error
    assert sched.failed == "" and sched.stats["errors"] == 0
    return [box[0], box[1]], sched, engine


def test_two_concurrent_requests_take_multi_steps(env):
    plain, s0, _ = run(env, dict(mode="off"))
    assert s0.stats["spec_steps"] == 0 and all(r.completion_tokens == MAX_TOKENS for r in plain)
    preds = [list(r.token_ids) for r in plain]
    on, s1, eng = run(env, dict(mode="lookup"), preds, check=True)       # every call checked as it runs
    off, s2, _ = run(env, dict(mode="lookup", multi=0), preds)
    st = s1.stats
    assert s1.pipeline and s1.can_spec_multi and st["spec_multi_steps"] > 0 and st["spec_multi_steps"] == len(eng.calls)
    assert s2.stats["spec_multi_steps"] == 0
    for i in (0, 1):
        assert on[i].token_ids == off[i].token_ids == plain[i].token_ids and on[i].text == plain[i].text
        assert on[i].finish_reason == off[i].finish_reason == plain[i].finish_reason
    assert st["spec_accepted"] > 0 and st["steps"] < s0.stats["steps"]
    # usage: accepted and rejected drafts per request; together at least what the multi calls had (a request's
    # lone steps at the end go through spec_decode and are counted as well)
    drafted = sum(len(t) - 1 for _, toks, _ in eng.calls for t in toks)
    accepted = sum(a for _, _, res in eng.calls for a, _ in res)
    assert st["spec_drafted"] >= drafted > 0 and st["spec_accepted"] >= accepted > 0
    for i in (0, 1):
        u = prediction_usage(on[i])
        assert u["accepted_prediction_tokens"] == on[i].accepted_draft_tokens > 0
        assert u["accepted_prediction_tokens"] + u["rejected_prediction_tokens"] == on[i].draft_tokens
    assert sum(r.draft_tokens for r in on) == st["spec_drafted"]
    assert sum(r.accepted_draft_tokens for r in on) == st["spec_accepted"]
    again, _, _ = run(env, dict(mode="off"))       # (and the engine is left as plain decode expects it)
    assert [r.token_ids for r in again] == [r.token_ids for r in plain]
