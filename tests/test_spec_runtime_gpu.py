"""Speculative decoding end to end on the device: a real Scheduler (pipelined decode, the engine's spec_decode)
on test-tiny, greedy, a prompt that is a token pattern repeated.

The speculative run must emit the tokens of the run with speculation off.  The rows of a speculative step go
through the batched kernels (B = R) and the plain run through the B = 1 kernels, which differ in the low bits, so a
near-tie between the two best logits could legitimately flip a greedy token.  The model seed below was picked on
the device so that this cannot happen here: over the tokens the plain run generates,
    the smallest top-2 logit gap is                                      0.1317
    the largest |logit(B = 1) - logit(B = 4 or 8)| on the same rows is   0.00158
a ratio of 83, above the 10 the margin asks for (seeds 0..11 gave ratios from 1.06 to 83; seed 10 is the best; the
decode kernels are the parent commit's: nothing in them changed).

Acceptance (`spec_accepted > 0`) is asserted with the plain run's own output as the prediction: the model is
random-init, it does not continue the prompt's pattern, so the prompt's text as the prediction has no reason to be
accepted.  That run is made too and must give the same tokens; what it drafts is not asserted.  After every run the
tier must be healthy: no engine error, whichever step the request's last token came from.
"""
import threading

import pytest

from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.runtime.scheduler import GenRequest, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

pytestmark = pytest.mark.gpu

PATTERN = [60, 61, 62, 63, 64, 65, 66, 67, 68]
PROMPT = [1] + PATTERN * 4
MAX_TOKENS = 40
MODEL_SEED = 10


@pytest.fixture(scope="module")
def env():
    from aios_amd.runtime.loader import random_engine

    t, s, ty = synthetic_vocab(512)
    eng = random_engine(get_preset("test-tiny"), "Q4_K_M", seed=MODEL_SEED, max_ctx=256, max_slots=4, max_batch=8)
    return eng, SpmTokenizer(t, s, ty, 1, 2)


def run(env, tier=None, max_tokens=MAX_TOKENS, **kw):
    eng, tok = env
    sched = Scheduler(eng, tok, max_batch=8, max_slots=4, max_ctx=256, speculative=tier)
    ev, box = threading.Event(), {}
    r = GenRequest(prompt_ids=list(PROMPT), max_tokens=max_tokens, temperature=0.0, stop_ids=[], **kw)
    r.on_done = lambda res: (box.__setitem__(0, res), ev.set())
    try:
        sched.submit(r)
        assert ev.wait(60)
    finally:
        sched.close()
    assert box[0].finish_reason != "error", box[0].error
    assert sched.failed == "" and sched.stats["errors"] == 0
    return box[0], sched


def test_speculative_run_emits_the_plain_run(env):
    off, s0 = run(env, speculative=False)
    assert s0.pipeline and s0.can_spec and s0.stats["spec_steps"] == 0 and off.completion_tokens > 8
    # the caller predicts the output exactly: (nearly) every draft is accepted
    on, s1 = run(env, speculative=True, prediction_ids=list(off.token_ids))
    assert on.token_ids == off.token_ids and on.text == off.text and on.finish_reason == off.finish_reason
    st = s1.stats
    assert st["spec_accepted"] > 0 and st["spec_steps"] > 0 and st["steps"] < s0.stats["steps"]
    assert (on.draft_tokens, on.accepted_draft_tokens) == (st["spec_drafted"], st["spec_accepted"])
    assert s1.metrics()["spec_accept_rate"] > 0.5
    # the prompt's own text as the prediction, and the tier's default instead of the request's field: whatever
    # is drafted, right or wrong, the tokens stay the plain run's
    onp, s2 = run(env, tier=dict(mode="lookup", draft_max=7), prediction_ids=list(PROMPT[1:]))
    assert onp.token_ids == off.token_ids and s2.spec["draft_max"] == 7
    again, _ = run(env, speculative=False)       # (and the engine is left as plain decode expects it)
    assert again.token_ids == off.token_ids


@pytest.mark.parametrize("max_tokens", [5, 6, 7, 8])
def test_every_request_length_leaves_the_tier_healthy(env, max_tokens):
    """the request's last token may be the one collected from the in-flight step while looking for a draft"""
    off, _ = run(env, speculative=False, max_tokens=max_tokens)
    on, _ = run(env, speculative=True, max_tokens=max_tokens)
    onp, _ = run(env, speculative=True, max_tokens=max_tokens, prediction_ids=list(off.token_ids))
    assert on.token_ids == onp.token_ids == off.token_ids and off.completion_tokens == max_tokens
