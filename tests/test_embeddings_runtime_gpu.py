"""/v1/embeddings through a real test-small tier on the GPU: two inputs of different length return two unit
vectors, and the same input twice gives identical bytes (inputs below 33 tokens: their forward has no
float-atomic split-K, and the pooling kernel is bit-reproducible)."""
import asyncio

import numpy as np
import pytest

from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.runtime import chat_template
from aios_amd.runtime.scheduler import Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

pytestmark = pytest.mark.gpu


def test_round_trip():
    import aiohttp

    from aios_amd.runtime import model_manager as mm
    from aios_amd.runtime.loader import random_engine
    from aios_amd.runtime.service import AIRuntimeService

    cfg = get_preset("test-small")
    t, s, ty = synthetic_vocab(cfg.vocab_size)
    tok = SpmTokenizer(t, s, ty, cfg.bos_id, cfg.eos_id)

    class Mgr(mm.ModelManager):
        def _load_blocking(self, m, context_length):
            m.engine = random_engine(cfg, "Q4_K_M", seed=2, max_ctx=128, max_slots=2, max_batch=2)
            m.config, m.tokenizer, m.grammar, m.context_length = cfg, tok, None, 128
            m.template = chat_template.for_model("zephyr", tok)
            m.scheduler = Scheduler(m.engine, tok, 2, 2, 128, None, m.name)

    async def run():
        mgr = Mgr(base_port=18970)
        svc = AIRuntimeService(mgr, http=True)
        m = await mgr.load_model("small", "fake.gguf", port=18971)
        await svc.start_http(m)
        out = []
        try:
            async with aiohttp.ClientSession() as ses:
                for body in ({"input": ["status", "the agent checked the memory service"]},
                             {"input": ["status", "status"], "encoding_format": "base64"}):
                    async with ses.post("http://127.0.0.1:18971/v1/embeddings", json=body) as r:
                        out.append((r.status, await r.json()))
        finally:
            await svc.close()
        return out

    (s1, two), (s2, same) = asyncio.run(run())
    assert s1 == s2 == 200
    a, b = (np.asarray(d["embedding"], np.float64) for d in two["data"])
    assert a.shape == b.shape == (cfg.d_model,)
    assert abs(np.linalg.norm(a) - 1) < 1e-5 and abs(np.linalg.norm(b) - 1) < 1e-5
    assert not np.array_equal(a, b)  # (random-init weights: the two differ by ~1e-5 only, but they differ)
    assert two["usage"]["prompt_tokens"] == two["usage"]["total_tokens"] > 2
    assert same["data"][0]["embedding"] == same["data"][1]["embedding"]
