"""Speculative decoding's public surface on the CPU backend, whose engine has no spec_decode: the body fields
are parsed (`prediction`, `speculative`), malformed ones answer 400, the request is served by plain decode, and
usage.completion_tokens_details is present and 0 / 0.  Plus the node config's tier fields and their way to the
scheduler through the model spec."""
import asyncio

import pytest

from aios_amd.models.config import get_preset
from aios_amd.models.synthetic import synthetic_vocab, write_synthetic_gguf
from aios_amd.runtime import chat_template
from aios_amd.runtime.cpu_engine import CpuEngine
from aios_amd.runtime.scheduler import SPEC_DEFAULTS, Scheduler
from aios_amd.runtime.service import prediction_from_body, prediction_usage
from aios_amd.runtime.tokenizer import SpmTokenizer

ZERO = {"accepted_prediction_tokens": 0, "rejected_prediction_tokens": 0}


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    p = tmp_path_factory.mktemp("spec") / "tiny.gguf"
    write_synthetic_gguf(str(p), get_preset("test-tiny"), "Q8_0", seed=5)
    t, s, ty = synthetic_vocab(512)
    return str(p), SpmTokenizer(t, s, ty, 1, 2)


def test_prediction_is_parsed(setup):
    _, tok = setup
    text = "w10 w11 w12"
    ids = tok.encode(text, add_bos=False, parse_special=False)
    assert ids and tok.bos_id not in ids
    assert prediction_from_body({}, tok) == (None, None)
    assert prediction_from_body({"speculative": True}, tok) == (True, None)
    assert prediction_from_body({"speculative": False}, tok) == (False, None)
    assert prediction_from_body({"prediction": {"type": "content", "content": text}}, tok) == (True, ids)
    parts = [{"type": "text", "text": "w10 w11"}, {"type": "text", "text": " w12"}]
    assert prediction_from_body({"prediction": {"type": "content", "content": parts}}, tok) == (True, ids)
    # the request's own word about speculation stands; the prediction is still kept
    assert prediction_from_body({"prediction": {"type": "content", "content": text}, "speculative": False}, tok) == (False, ids)
    for bad in ({"prediction": "w10"}, {"prediction": {"type": "text", "content": text}}, {"prediction": {"type": "content"}},
                {"prediction": {"type": "content", "content": ""}}, {"prediction": {"type": "content", "content": []}},
                {"prediction": {"type": "content", "content": [{"type": "image", "text": "x"}]}},
                {"prediction": {"type": "content", "content": [{"type": "text", "text": 5}]}},
                {"prediction": {"type": "content", "content": 7}}, {"speculative": "yes"}, {"speculative": 1}):
        with pytest.raises(ValueError):
            prediction_from_body(bad, tok)


def test_usage_details():
    class R:
        draft_tokens, accepted_draft_tokens = 9, 4

    assert prediction_usage(R()) == {"accepted_prediction_tokens": 4, "rejected_prediction_tokens": 5}
    assert prediction_usage(object()) == ZERO


def _serve(path, tok, port, calls):
    import aiohttp

    from aios_amd.runtime import model_manager as mm
    from aios_amd.runtime.service import AIRuntimeService

    class Mgr(mm.ModelManager):
        def _load_blocking(self, m, context_length):
            m.engine = CpuEngine.from_gguf(path, max_ctx=128, max_slots=2, max_batch=2)
            m.tokenizer = tok
            m.template = chat_template.for_model("zephyr", tok)
            m.grammar = None
            m.context_length = 128
            m.scheduler = Scheduler(m.engine, tok, 2, 2, 128, None, m.name)

    async def run():
        mgr = Mgr(base_port=port)
        svc = AIRuntimeService(mgr, http=True)
        m = await mgr.load_model("tiny", "fake.gguf", port=port)
        await svc.start_http(m)
        try:
            async with aiohttp.ClientSession() as s:
                return await calls(s, f"http://127.0.0.1:{port}"), m.scheduler
        finally:
            await svc.close()

    return asyncio.run(run())


def test_http_fields_400s_and_usage(setup):
    pytest.importorskip("aiohttp")
    path, tok = setup
    text = "w10 w11 w12 w13"
    pred = {"type": "content", "content": text + " " + text}
    msgs = [{"role": "user", "content": text}]

    async def calls(s, base):
        out = {}
        chat, cmpl = base + "/v1/chat/completions", base + "/v1/completions"
        for name, url, body in (
                ("chat_plain", chat, {"messages": msgs, "max_tokens": 4, "temperature": 0}),
                ("chat_pred", chat, {"messages": msgs, "max_tokens": 4, "temperature": 0, "prediction": pred}),
                ("chat_spec", chat, {"messages": msgs, "max_tokens": 4, "temperature": 0, "speculative": True}),
                ("cmpl_plain", cmpl, {"prompt": text, "max_tokens": 4, "temperature": 0}),
                ("cmpl_pred", cmpl, {"prompt": text, "max_tokens": 4, "temperature": 0, "prediction": pred}),
                ("cmpl_off", cmpl, {"prompt": text, "max_tokens": 4, "temperature": 0, "speculative": False})):
            async with s.post(url, json=body) as r:
                assert r.status == 200, name
                out[name] = await r.json()
        bad = []
        for url, body in ((chat, {"messages": msgs, "prediction": {"type": "content"}}),
                          (chat, {"messages": msgs, "prediction": "w10"}),
                          (chat, {"messages": msgs, "speculative": "on"}),
                          (cmpl, {"prompt": text, "prediction": {"type": "audio", "content": text}}),
                          (cmpl, {"prompt": text, "prediction": {"type": "content", "content": [{"type": "text"}]}}),
                          (cmpl, {"prompt": text, "speculative": 3})):
            async with s.post(url, json=body) as r:
                bad.append((r.status, (await r.json())["error"]["type"]))
        return out, bad

    (out, bad), sched = _serve(path, tok, 18991, calls)
    assert bad == [(400, "invalid_request_error")] * 6
    # the engine cannot speculate: the fields are accepted, the text is the plain run's, nothing was drafted
    assert not sched.can_spec and sched.stats["spec_steps"] == 0
    for k in ("chat_plain", "chat_pred", "chat_spec"):
        assert out[k]["usage"]["completion_tokens_details"] == ZERO, k
        assert out[k]["choices"][0]["message"]["content"] == out["chat_plain"]["choices"][0]["message"]["content"]
    for k in ("cmpl_pred", "cmpl_off"):
        assert out[k]["usage"]["completion_tokens_details"] == ZERO, k
        assert out[k]["choices"][0]["text"] == out["cmpl_plain"]["choices"][0]["text"]
    u = out["cmpl_pred"]["usage"]
    assert u["total_tokens"] == u["prompt_tokens"] + u["completion_tokens"]


def test_tier_config_reaches_the_scheduler():
    from aios_amd.parallel.tp import spec_speculative
    from aios_amd.utils.config import ModelTier

    t = ModelTier()
    assert (t.speculative, t.spec_draft_max, t.spec_ngram_min, t.spec_ngram_max, t.spec_max_context) == (
        SPEC_DEFAULTS["mode"], SPEC_DEFAULTS["draft_max"], SPEC_DEFAULTS["ngram_min"], SPEC_DEFAULTS["ngram_max"],
        SPEC_DEFAULTS["max_context"])
    assert t.speculative == "off" and 1 <= t.spec_draft_max <= 7 and t.speculative_frag() == []
    t = ModelTier(speculative="lookup", spec_draft_max=6, spec_ngram_min=1, spec_ngram_max=4, spec_max_context=512)
    spec = "model.gguf#" + "&".join(["kv=fp8_e4m3"] + t.speculative_frag())
    assert spec_speculative(spec) == dict(mode="lookup", draft_max=6, ngram_min=1, ngram_max=4, max_context=512)
    assert spec_speculative("model.gguf") == {} and spec_speculative("model.gguf#tp=2") == {}
    # a malformed or out-of-range fragment keeps the default instead of failing the tier's load
    assert spec_speculative("m.gguf#spec=tree&specdraft=x&specctx=0&specnmin=3&specnmax=2") == {}
    assert spec_speculative("m.gguf#spec=lookup&specdraft=9&specnmax=9") == dict(mode="lookup")


def test_node_config_keeps_defaults_for_bad_values(tmp_path):
    from aios_amd.utils import config as C

    p = tmp_path / "node.toml"
    p.write_text('[models.operational]\nspeculative = "lookup"\nspec_max_context = 0\nspec_ngram_max = 12\n'
                 'spec_draft_max = 9\n[models.tactical]\nspeculative = "tree"\nspec_max_context = 512\n')
    cfg = C.load(str(p))
    op, ta = cfg.models.tiers["operational"], cfg.models.tiers["tactical"]
    assert (op.speculative, op.spec_max_context, op.spec_ngram_min, op.spec_ngram_max, op.spec_draft_max) == ("lookup", 4096, 2, 3, 7)
    assert (ta.speculative, ta.spec_max_context) == ("off", 512)
    assert op.speculative_frag() == ["spec=lookup"] and ta.speculative_frag() == ["specctx=512"]
