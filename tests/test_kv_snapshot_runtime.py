"""GET /slots and POST /slots/{id}?action=save|restore|erase on a model's port, over a fake engine
(test_kv_snapshot_scheduler.Fake): status codes, file-name hygiene, response shapes; and the configuration keys."""
import asyncio
import os

import pytest

import test_kv_snapshot_scheduler as T

from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.runtime import chat_template
from aios_amd.runtime.scheduler import Scheduler
from aios_amd.runtime.tokenizer import SpmTokenizer

BAD_NAMES = ["", "a/b", "../up.kv", "..", "x..y", "sub\\f", "nul\0byte", "/abs.kv", None, 5, ["a"]]


def serve(tmp_path, port, save_path, snapshots=True, work=None):
    """run `work(session, base_url, model)` against a one-model service on `port`"""
    import aiohttp

    from aios_amd.runtime import model_manager as mm
    from aios_amd.runtime.service import AIRuntimeService

    t, s, ty = synthetic_vocab(T.V)
    tok = SpmTokenizer(t, s, ty, 1, T.EOS)

    class Mgr(mm.ModelManager):
        def _load_blocking(self, m, context_length):
            m.engine = T.Fake(snapshots=snapshots)
            m.tokenizer, m.grammar, m.context_length = tok, None, T.MAX_CTX
            m.template = chat_template.for_model("zephyr", tok)
            m.scheduler = Scheduler(m.engine, tok, 4, 2, T.MAX_CTX, None, m.name)
            m.slot_save_path = save_path

    async def run():
        mgr = Mgr(base_port=port)
        svc = AIRuntimeService(mgr, http=True)
        m = await mgr.load_model("fake", "fake.gguf", port=port + 1)
        await svc.start_http(m)
        try:
            async with aiohttp.ClientSession() as ses:
                return await work(ses, f"http://127.0.0.1:{port + 1}", m)
        finally:
            await svc.close()

    return asyncio.run(run())


async def post(ses, url, body=None, raw=None):
    async with ses.post(url, json=body, data=raw) as r:
        return r.status, await r.json()


def test_actions_answer_501_without_a_save_path(tmp_path):
    async def work(ses, base, m):
        out = [await post(ses, f"{base}/slots/0?action={a}", {"filename": "a.kv"}) for a in ("save", "restore", "erase")]
        async with ses.get(f"{base}/slots") as r:  # the listing needs no directory
            out.append((r.status, await r.json()))
        out.append(await post(ses, f"{base}/slots/0?action=explode", {"filename": "a.kv"}))
        return out

    out = serve(tmp_path, 19040, "", work=work)
    for st, body in out[:3]:
        assert st == 501 and "slot_save_path" in body["error"]["message"]
    assert out[3] == (200, [{"id": 0, "is_processing": False, "n_cached": 0}, {"id": 1, "is_processing": False, "n_cached": 0}])
    assert out[4][0] == 400 and "action" in out[4][1]["error"]["message"]
    assert os.listdir(tmp_path) == []


def test_save_restore_erase_and_their_refusals(tmp_path):
    save_dir = tmp_path / "snaps"
    save_dir.mkdir()

    async def work(ses, base, m):
        o = {}
        async with ses.post(f"{base}/v1/completions", json={"prompt": list(T.PROMPT), "max_tokens": 4, "temperature": 0}) as r:
            assert r.status == 200
        async with ses.get(f"{base}/slots") as r:
            o["slots"] = await r.json()
        sid = max(o["slots"], key=lambda s: s["n_cached"])["id"]
        o["sid"] = sid
        o["bad"] = [await post(ses, f"{base}/slots/{sid}?action={a}", {"filename": n}) for n in BAD_NAMES
                    for a in ("save", "restore")]
        o["nobody"] = await post(ses, f"{base}/slots/{sid}?action=save", raw=b"not json")
        o["save"] = await post(ses, f"{base}/slots/{sid}?action=save", {"filename": "a.kv"})
        o["missing"] = await post(ses, f"{base}/slots/{sid}?action=restore", {"filename": "none.kv"})
        o["slot"] = [await post(ses, f"{base}/slots/{s}?action=save", {"filename": "b.kv"}) for s in ("7", "-1", "x")]
        o["action"] = await post(ses, f"{base}/slots/{sid}", {"filename": "a.kv"})
        o["empty"] = await post(ses, f"{base}/slots/{1 - sid}?action=save", {"filename": "e.kv"})
        o["erase"] = await post(ses, f"{base}/slots/{sid}?action=erase")
        o["restore"] = await post(ses, f"{base}/slots/{1 - sid}?action=restore", {"filename": "a.kv"})
        async with ses.get(f"{base}/slots") as r:
            o["slots_after"] = await r.json()
        # a header that does not fit: the engine's shape changes under the same file
        m.engine.config.head_dim = 16
        o["mismatch"] = await post(ses, f"{base}/slots/{sid}?action=restore", {"filename": "a.kv"})
        m.engine.config.head_dim = 8
        raw = (save_dir / "a.kv").read_bytes()
        (save_dir / "a.kv").write_bytes(raw[:-1] + bytes([raw[-1] ^ 1]))
        o["crc"] = await post(ses, f"{base}/slots/{sid}?action=restore", {"filename": "a.kv"})
        # a busy slot: the request's first decode step is held
        m.engine.entered.clear()
        m.engine.gate.clear()
        task = asyncio.ensure_future(post(ses, f"{base}/v1/completions",
                                          {"prompt": [1, 400, 401], "max_tokens": 3, "temperature": 0}))
        assert await asyncio.to_thread(m.engine.entered.wait, 30)
        busy = [s for s in m.scheduler.slot_cache if s not in m.scheduler.free_slots][0]
        pending = asyncio.ensure_future(post(ses, f"{base}/slots/{busy}?action=erase"))
        while not m.scheduler._ops:
            await asyncio.sleep(0.001)
        m.engine.gate.set()
        o["busy"] = await pending
        assert (await task)[0] == 200
        o["stats"] = dict(m.scheduler.stats)
        return o

    o = serve(tmp_path, 19044, str(save_dir), work=work)
    n = len(T.PROMPT) + 3
    assert sorted(s["n_cached"] for s in o["slots"]) == [0, n] and not any(s["is_processing"] for s in o["slots"])
    for st, body in o["bad"]:
        assert st == 400 and "filename" in body["error"]["message"], (st, body)
    assert o["nobody"][0] == 400
    st, save = o["save"]
    assert st == 200 and save["id_slot"] == o["sid"] and save["filename"] == "a.kv" and save["n_saved"] == n
    assert save["n_written"] > 0 and save["timings"]["save_ms"] >= 0
    assert o["missing"][0] == 404
    for st, body in o["slot"]:
        assert st == 400 and "slot" in body["error"]["message"]
    assert o["action"][0] == 400 and o["empty"][0] == 400
    assert o["erase"] == (200, {"id_slot": o["sid"], "n_erased": n})
    st, rest = o["restore"]
    assert st == 200 and rest["id_slot"] == 1 - o["sid"] and rest["n_restored"] == n and rest["n_read"] == save["n_written"]
    assert rest["timings"]["restore_ms"] >= 0
    assert {s["id"]: s["n_cached"] for s in o["slots_after"]} == {o["sid"]: 0, 1 - o["sid"]: n}
    assert o["mismatch"][0] == 409 and "head_dim" in o["mismatch"][1]["error"]["message"]
    assert o["crc"][0] == 409 and "crc32" in o["crc"][1]["error"]["message"]
    assert o["busy"][0] == 409 and "slot busy" in o["busy"][1]["error"]["message"]
    assert (o["stats"]["slot_saves"], o["stats"]["slot_restores"], o["stats"]["slot_erases"]) == (1, 1, 1)
    # nothing was opened or created outside the directory, and only the one file inside it
    assert sorted(os.listdir(tmp_path)) == ["snaps"] and os.listdir(save_dir) == ["a.kv"]


def test_a_tier_without_engine_snapshots_answers_400(tmp_path):
    """what a tensor-parallel or CPU tier presents: an engine without kv_save / kv_restore"""
    from aios_amd.parallel.tp import TPEngine

    class Shard:
        kv_save = kv_restore = copy_slot = staticmethod(lambda *a: None)

    tp = TPEngine(Shard(), comm=None, send=lambda msg: None)
    assert not hasattr(tp, "kv_save") and not hasattr(tp, "kv_restore") and hasattr(tp, "copy_slot")

    async def work(ses, base, m):
        return [await post(ses, f"{base}/slots/0?action={a}", {"filename": "a.kv"}) for a in ("save", "restore", "erase")]

    for st, body in serve(tmp_path, 19048, str(tmp_path), snapshots=False, work=work):
        assert st == 400 and body["error"]["message"] == "slots: single-GPU engines only"
    assert os.listdir(tmp_path) == []


def test_config_keys(tmp_path):
    from aios_amd.parallel.tp import spec_slot_snapshots
    from aios_amd.utils import config

    assert config.ModelsConfig().slot_save_path == "" and config.ModelTier().kv_restore == []
    assert config.ModelTier().snapshot_frag("") == [] and spec_slot_snapshots("synthetic:test-tiny#kv=fp8_e4m3") == ("", [])
    p = tmp_path / "c.toml"
    p.write_text('[models]\nslot_save_path = "/var/lib/aios/kv snaps&#"\n'
                 '[models.a]\nfile = "synthetic:test-tiny"\nkv_restore = ["pre amble.kv", "b,c.kv"]\n'
                 '[models.b]\nfile = "synthetic:test-tiny"\nslot_save_path = "/srv/b"\n'
                 '[models.c]\nfile = "synthetic:test-tiny"\nkv_restore = "notalist"\n')
    cfg = config.load(str(p), env={})
    specs = {name: spec for name, spec, _ in cfg.model_specs()}
    assert spec_slot_snapshots(specs["a"]) == ("/var/lib/aios/kv snaps&#", ["pre amble.kv", "b,c.kv"])
    assert spec_slot_snapshots(specs["b"]) == ("/srv/b", [])
    assert spec_slot_snapshots(specs["c"]) == ("/var/lib/aios/kv snaps&#", [])
    assert any("models.c.kv_restore" in w for w in cfg.warnings)
    assert {t["name"]: t["spec"] for t in cfg.tier_plan()} == specs
    # the default file leaves both off
    default = config.load(os.path.join(os.path.dirname(__file__), "..", "config", "default-config.toml"), env={})
    assert default.models.slot_save_path == "" and all(not t.kv_restore for t in default.models.tiers.values())
