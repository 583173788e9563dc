"""JSON-schema requests through the scheduler on the native engine (test-tiny, random weights): the device computes
the masks (Engine.set_grammar_rows, no mask bytes uploaded), every request finishes "grammar" or "stop" with a text
that validates over 16 seeds at temperature 1, a request cut short leaves a live prefix, a schema beside a ban
goes back to host masks, and requests without a schema make no grammar call."""
import numpy as np
import pytest

import schema_oracle as SO
from aios_amd.runtime import json_schema as JS
from aios_amd.runtime.scheduler import GenRequest, Scheduler

pytestmark = pytest.mark.gpu

PROMPT = [1, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49]
V, EOS, CTX = 512, 2, 256


@pytest.fixture(scope="module")
def setup():
    from aios_amd.models.config import get_preset
    from aios_amd.models.synthetic import synthetic_vocab
    from aios_amd.runtime.loader import random_engine
    from aios_amd.runtime.tokenizer import SpmTokenizer

    cfg = get_preset("test-tiny")
    assert cfg.vocab_size == V
    eng = random_engine(cfg, "Q4_K_M", seed=5, max_ctx=CTX, max_slots=4, max_batch=4)
    t, s, ty = synthetic_vocab(V)
    return eng, SpmTokenizer(t, s, ty, 1, EOS)


def _sched(eng, tok):
    return Scheduler(eng, tok, max_batch=4, max_slots=4, max_ctx=CTX)


def check_finished(name, schema, res, tok):
    assert res.finish_reason in ("grammar", "stop"), (name, res.finish_reason, res.error, res.text)
    assert SO.parse_and_validate(res.text, schema), (name, res.text)
    assert res.text == tok.decode(res.token_ids)


@pytest.mark.parametrize("name", list(SO.BOUNDED))
def test_every_request_finishes_with_a_valid_text(setup, name):
    eng, tok = setup
    spy = SO.spy_on(eng)
    schema = SO.BOUNDED[name]
    longest = JS.compile_schema(schema).longest_path()
    assert longest is not None and longest + len(PROMPT) < CTX
    sched = _sched(spy, tok)
    assert sched.can_device_grammar
    reqs = [GenRequest(prompt_ids=list(PROMPT), max_tokens=longest, temperature=1.0, top_k=0, top_p=1.0, seed=seed,
                       json_schema=schema) for seed in range(1, 17)]
    res = SO.run_requests(sched, reqs)
    for r in res:
        check_finished(name, schema, r, tok)
    assert len({r.text for r in res}) > 1
    assert sched.stats["schema_requests"] == 16 and sched.stats["schema_compiles"] == 1 and not sched.failed
    # every sampler launch of these rows was staged on the device and uploaded no mask bytes
    assert len(spy.grammar_rows) >= sum(len(r.token_ids) for r in res) // 4 and set(spy.masks) <= {0}
    assert all(g >= 0 and s >= 1 for gids, states in spy.grammar_rows for g, s in zip(gids, states))
    assert sorted(sched.free_slots) == [0, 1, 2, 3]


def test_cut_short_banned_and_plain_rows(setup):
    eng, tok = setup
    schema = SO.BOUNDED["tool_call"]
    dfa = JS.compile_schema(schema)
    spy = SO.spy_on(eng)
    cut, = SO.run_requests(_sched(spy, tok), [GenRequest(prompt_ids=list(PROMPT), max_tokens=4, json_schema=schema)])
    assert cut.finish_reason == "length" and len(cut.token_ids) == 4 and spy.grammar_rows
    raw = b"".join(tok.token_bytes(t) for t in cut.token_ids)
    assert dfa.rejects_at(raw) == len(raw)                      # a prefix of the language, not yet a member
    # the same request through host masks (a ban on a token the answer never uses)
    unused = next(t for t in range(300, V) if t not in cut.token_ids)
    spy = SO.spy_on(eng)
    sched = _sched(spy, tok)
    host, moved = SO.run_requests(sched, [
        GenRequest(prompt_ids=list(PROMPT), max_tokens=4, json_schema=schema, logit_bias={unused: -np.inf}),
        GenRequest(prompt_ids=list(PROMPT), max_tokens=JS.compile_schema(SO.BOUNDED["flags"]).longest_path(),
                   json_schema=SO.BOUNDED["flags"], logit_bias={cut.token_ids[0]: -np.inf, 7: 0.5})], together=False)
    assert spy.grammar_rows == [] and host.finish_reason == "length"     # bans: the host path, no device rows
    raw = b"".join(tok.token_bytes(t) for t in host.token_ids)
    assert dfa.rejects_at(raw) == len(raw) and unused not in host.token_ids
    check_finished("flags", SO.BOUNDED["flags"], moved, tok)
    # rows without a schema make no grammar call and upload no mask
    spy = SO.spy_on(eng)
    plain, = SO.run_requests(_sched(spy, tok), [GenRequest(prompt_ids=list(PROMPT), max_tokens=6, stop_ids=[])])
    assert len(plain.token_ids) == 6 and spy.grammar_rows == [] and set(spy.masks) <= {0}
    # a schema row and a plain row in one batch: the plain row is not constrained by the neighbour's mask
    spy = SO.spy_on(eng)
    both = SO.run_requests(_sched(spy, tok), [GenRequest(prompt_ids=list(PROMPT), max_tokens=6, stop_ids=[]),
                                              GenRequest(prompt_ids=list(PROMPT), max_tokens=4, json_schema=schema)])
    raw = b"".join(tok.token_bytes(t) for t in both[1].token_ids)
    assert len(both[0].token_ids) == 6 and dfa.rejects_at(raw) == len(raw)
    free = b"".join(tok.token_bytes(t) for t in both[0].token_ids)
    assert dfa.rejects_at(free) not in (None, len(free))             # (random weights do not write a tool call)
    assert any(-1 in gids for gids, _ in spy.grammar_rows)
