"""logit_bias and ignore_eos through a real test-tiny tier on the GPU: the HTTP path (a ban on the greedy first
token, ignore_eos past an EOS the bias itself forces) and the scheduler's pipelined decode with a biased and an
unbiased request in one batch -- the unbiased one's tokens are those of a run of it alone."""
import asyncio
import threading

import numpy as np
import pytest

from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.runtime import chat_template
from aios_amd.runtime.scheduler import GenRequest, Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

pytestmark = pytest.mark.gpu


def _submit(sched, reqs):
    """queue the requests together (one batch) and wait for all of them"""
    evs, box = [threading.Event() for _ in reqs], {}
    for i, r in enumerate(reqs):
        r.on_done = lambda res, i=i: (box.__setitem__(i, res), evs[i].set())
    with sched.cv:
        for r in reqs:
            sched.submit(r)
    for e in evs:
        assert e.wait(60)
    return [box[i] for i in range(len(reqs))]


def test_http_and_pipelined_batch():
    import aiohttp

    from aios_amd.runtime import model_manager as mm
    from aios_amd.runtime.loader import random_engine
    from aios_amd.runtime.service import AIRuntimeService

    cfg = get_preset("test-tiny")
    t, s, ty = synthetic_vocab(cfg.vocab_size)
    tok = SpmTokenizer(t, s, ty, cfg.bos_id, cfg.eos_id)
    ids = [cfg.bos_id] + [int(x) for x in np.random.default_rng(8).integers(20, cfg.vocab_size, 11)]
    other = [cfg.bos_id] + [int(x) for x in np.random.default_rng(9).integers(20, cfg.vocab_size, 7)]
    N = 8

    class Mgr(mm.ModelManager):
        def _load_blocking(self, m, context_length):
            m.engine = random_engine(cfg, "Q4_K_M", seed=2, max_ctx=128, max_slots=2, max_batch=2)
            m.config, m.tokenizer, m.grammar, m.context_length = cfg, tok, None, 128
            m.template = chat_template.for_model("zephyr", tok)
            m.scheduler = Scheduler(m.engine, tok, 2, 2, 128, None, m.name)

    def req(prompt, **kw):
        return GenRequest(prompt_ids=list(prompt), max_tokens=N, temperature=0.0, stop_ids=[], **kw)

    async def run():
        mgr = Mgr(base_port=19020)
        svc = AIRuntimeService(mgr, http=True)
        m = await mgr.load_model("tiny", "fake.gguf", port=19021)
        await svc.start_http(m)
        sched = m.scheduler
        loop = asyncio.get_running_loop()
        out = {}
        try:
            assert sched.pipeline and sched.can_bias
            out["alone"], = await loop.run_in_executor(None, _submit, sched, [req(ids)])
            out["other_alone"], = await loop.run_in_executor(None, _submit, sched, [req(other, ignore_eos=True)])
            first = out["alone"].token_ids[0]
            bias = {first: -np.inf, 33: 1.5, 34: -2.0}
            out["biased_alone"], = await loop.run_in_executor(None, _submit, sched, [req(ids, logit_bias=bias)])
            # the pipelined path, the two kinds of row in one batch (in both row orders)
            out["pair"] = await loop.run_in_executor(None, _submit, sched, [req(ids, logit_bias=bias),
                                                                            req(other, ignore_eos=True)])
            out["pair2"] = await loop.run_in_executor(None, _submit, sched, [req(ids), req(ids, logit_bias=bias)])
            async with aiohttp.ClientSession() as ses:
                url = "http://127.0.0.1:19021/v1/completions"
                base = {"prompt": ids, "max_tokens": N, "temperature": 0}
                bodies = dict(plain=base,
                              banned=dict(base, logit_bias=[[first, False], [33, 1.5], [34, -2.0]]),
                              eos=dict(base, logit_bias={str(cfg.eos_id): 1000}),
                              past_eos=dict(base, logit_bias={str(cfg.eos_id): 1000}, ignore_eos=True),
                              bad=dict(base, logit_bias={str(cfg.vocab_size): 1}))
                for k, body in bodies.items():
                    async with ses.post(url, json=body) as r:
                        out[k] = (r.status, await r.json())
            out["stats"] = dict(sched.stats)
        finally:
            await svc.close()
        return out

    o = asyncio.run(run())
    alone, biased = o["alone"], o["biased_alone"]
    first = alone.token_ids[0]
    assert len(alone.token_ids) >= 1 and biased.token_ids[0] != first and first not in biased.token_ids
    # one batch, pipelined: each request's tokens are those of its run alone
    assert [r.token_ids for r in o["pair"]] == [biased.token_ids, o["other_alone"].token_ids]
    assert [r.token_ids for r in o["pair2"]] == [alone.token_ids, biased.token_ids]
    assert cfg.eos_id not in o["other_alone"].token_ids and len(o["other_alone"].token_ids) == N
    # HTTP
    text = lambda k: o[k][1]["choices"][0]["text"]  # noqa: E731
    assert o["plain"][0] == o["banned"][0] == o["eos"][0] == o["past_eos"][0] == 200
    assert text("plain") == alone.text and text("banned") == biased.text != alone.text
    assert o["eos"][1]["usage"]["completion_tokens"] == 0 and o["eos"][1]["choices"][0]["finish_reason"] == "stop"
    assert o["past_eos"][1]["usage"]["completion_tokens"] == N
    assert o["past_eos"][1]["choices"][0]["finish_reason"] == "length"
    assert o["bad"][0] == 400 and "logit_bias" in o["bad"][1]["error"]["message"]
    assert o["stats"]["bias_overridden"] == 0
