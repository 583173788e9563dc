"""context_shift and n_keep through a real test-tiny tier on the GPU (max_ctx 256, one slot): a body that asks for
more tokens than the window gets them all, the same body without the field stops at the window as before, a
malformed n_keep is a 400, and a following request with the same prompt reuses at most n_keep cached tokens."""
import asyncio

import numpy as np
import pytest

from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.runtime import chat_template
from aios_amd.runtime.scheduler import Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

pytestmark = pytest.mark.gpu

MAX_CTX = 256


def test_http_context_shift():
    import aiohttp

    from aios_amd.runtime import model_manager as mm
    from aios_amd.runtime.loader import random_engine
    from aios_amd.runtime.service import AIRuntimeService

    cfg = get_preset("test-tiny")
    t, s, ty = synthetic_vocab(cfg.vocab_size)
    tok = SpmTokenizer(t, s, ty, cfg.bos_id, cfg.eos_id)
    ids = [cfg.bos_id] + [int(x) for x in np.random.default_rng(8).integers(20, cfg.vocab_size, 29)]
    KEEP = 8

    class Mgr(mm.ModelManager):
        def _load_blocking(self, m, context_length):
            m.engine = random_engine(cfg, "Q4_K_M", seed=2, max_ctx=MAX_CTX, max_slots=1, max_batch=1)
            m.config, m.tokenizer, m.grammar, m.context_length = cfg, tok, None, MAX_CTX
            m.template = chat_template.for_model("zephyr", tok)
            m.scheduler = Scheduler(m.engine, tok, 1, 1, MAX_CTX, None, m.name)

    async def run():
        mgr = Mgr(base_port=19030)
        svc = AIRuntimeService(mgr, http=True)
        m = await mgr.load_model("tiny", "fake.gguf", port=19031)
        await svc.start_http(m)
        sched = m.scheduler
        out = {}
        try:
            assert sched.can_shift and not sched.context_shift
            async with aiohttp.ClientSession() as ses:
                url = "http://127.0.0.1:19031/v1/completions"
                base = {"prompt": ids, "max_tokens": 400, "temperature": 0, "ignore_eos": True}
                bodies = [("shift", dict(base, context_shift=True, n_keep=KEEP)),
                          ("plain", base),
                          ("bad_str", dict(base, context_shift=True, n_keep="8")),
                          ("bad_neg", dict(base, n_keep=-2)),
                          ("bad_bool", dict(base, n_keep=True)),
                          ("bad_flag", dict(base, context_shift="yes")),
                          ("chat", None)]
                for k, body in bodies:
                    if k == "chat":  # the chat endpoint takes the fields too, and reports the cached prefix
                        body = {"messages": [{"role": "user", "content": "hello"}], "max_tokens": 300, "temperature": 0,
                                "ignore_eos": True, "context_shift": True, "n_keep": 4}
                        async with ses.post("http://127.0.0.1:19031/v1/chat/completions", json=body) as r:
                            out[k] = (r.status, await r.json())
                        continue
                    async with ses.post(url, json=body) as r:
                        out[k] = (r.status, await r.json())
                    if k == "shift":
                        out["cache_after_shift"] = list(sched.slot_cache[0])
                    if k == "plain":
                        out["plain_cached"] = sched.stats["cached_tokens"]
            out["stats"] = dict(sched.stats)
        finally:
            await svc.close()
        return out

    o = asyncio.run(run())
    st, shift = o["shift"]
    assert st == 200 and shift["usage"]["completion_tokens"] == 400
    assert shift["choices"][0]["finish_reason"] == "length" and shift["usage"]["context_shifts"] >= 1
    # the slot's record of cached tokens was cut to n_keep, and the next request with this prompt reused no more
    assert o["cache_after_shift"] == ids[:KEEP] and o["plain_cached"] <= KEEP
    st, plain = o["plain"]
    assert st == 200 and plain["usage"]["completion_tokens"] == MAX_CTX - len(ids)
    assert plain["choices"][0]["finish_reason"] == "length" and "context_shifts" not in plain["usage"]
    for k in ("bad_str", "bad_neg", "bad_bool"):
        assert o[k][0] == 400 and "n_keep" in o[k][1]["error"]["message"], o[k]
    assert o["bad_flag"][0] == 400 and "context_shift" in o["bad_flag"][1]["error"]["message"]
    st, chat = o["chat"]
    assert st == 200 and chat["usage"]["completion_tokens"] == 300 and chat["usage"]["context_shifts"] >= 1
    assert o["stats"]["context_shifts"] >= 2 and o["stats"]["shifted_tokens"] > 0
