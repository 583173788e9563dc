"""/v1/completions through a real test-tiny tier on the GPU: one echo + logprobs request.  The prompt's
token_logprobs equal the values of a direct Engine.score_prefill call on the same engine within the scoring
kernel's tolerance (a 12-token prompt: its forward goes through the fixed-order ring GEMM, so the two forwards
are the same), and the generated text equals that of the same request without echo."""
import asyncio

import numpy as np
import pytest

import logprob_oracle
from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.runtime import chat_template
from aios_amd.runtime.scheduler import Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

pytestmark = pytest.mark.gpu


def test_echo_logprobs_round_trip():
    import aiohttp

    from aios_amd.runtime import model_manager as mm
    from aios_amd.runtime.loader import random_engine
    from aios_amd.runtime.service import AIRuntimeService

    cfg = get_preset("test-tiny")
    t, s, ty = synthetic_vocab(cfg.vocab_size)
    tok = SpmTokenizer(t, s, ty, cfg.bos_id, cfg.eos_id)
    ids = [cfg.bos_id] + [int(x) for x in np.random.default_rng(8).integers(20, cfg.vocab_size, 11)]

    class Mgr(mm.ModelManager):
        def _load_blocking(self, m, context_length):
            m.engine = random_engine(cfg, "Q4_K_M", seed=2, max_ctx=128, max_slots=2, max_batch=2)
            m.config, m.tokenizer, m.grammar, m.context_length = cfg, tok, None, 128
            m.template = chat_template.for_model("zephyr", tok)
            m.scheduler = Scheduler(m.engine, tok, 2, 2, 128, None, m.name)

    async def run():
        mgr = Mgr(base_port=18980)
        svc = AIRuntimeService(mgr, http=True)
        m = await mgr.load_model("tiny", "fake.gguf", port=18981)
        await svc.start_http(m)
        out = []
        try:
            async with aiohttp.ClientSession() as ses:
                base = {"prompt": ids, "max_tokens": 4, "temperature": 0}
                for body in (dict(base, echo=True, logprobs=3), base):
                    async with ses.post("http://127.0.0.1:18981/v1/completions", json=body) as r:
                        out.append((r.status, await r.json()))
            # (the scheduler is idle: its requests are answered) the same prompt, straight through the engine
            direct = m.engine.score_prefill(1, ids, 0, -1, 3, False)
            stats = dict(m.scheduler.stats)
        finally:
            await svc.close()
        return out, direct, stats

    ((s1, echo), (s2, plain)), direct, stats = asyncio.run(run())
    assert s1 == s2 == 200 and stats["prompt_scores"] == 1
    lp = echo["choices"][0]["logprobs"]
    n_gen = echo["usage"]["completion_tokens"]
    assert echo["usage"]["prompt_tokens"] == len(ids) and 1 <= n_gen <= 4
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(ids) + n_gen
    assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    got = np.asarray(lp["token_logprobs"][1:len(ids)], np.float64)
    want = direct["lp"][:-1].astype(np.float64)
    err = float(np.max(np.abs(got - want)))
    print(f"completions gpu: max |http - direct score_prefill| = {err:.3e}")
    assert err <= logprob_oracle.GPU_TOL
    assert all(1 <= len(d) <= 3 for d in lp["top_logprobs"][1:])
    prompt_text = tok.decode(ids)
    assert echo["choices"][0]["text"].startswith(prompt_text)
    assert echo["choices"][0]["text"][len(prompt_text):] == plain["choices"][0]["text"]
    assert plain["choices"][0]["logprobs"] is None
