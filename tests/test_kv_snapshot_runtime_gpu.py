"""KV snapshots through a real test-tiny tier on the GPU, loaded by ModelManager from a model spec: a completion at
temperature 0, save of the slot it used, erase, restore, and the same request again -- identical text, the prompt
served from the restored cache and not prefilled again.  Then the warm start: the tier loaded again with kv_restore
lists the slot as cached, skips a missing and a mismatching file, and serves the prompt from the restored slot."""
import asyncio
from urllib.parse import quote

import numpy as np
import pytest

from aios_amd.models.config import get_preset

pytestmark = pytest.mark.gpu

MAX_CTX = 256


def test_http_save_erase_restore_and_warm_start(tmp_path):
    import aiohttp

    from aios_amd.runtime import kv_snapshot
    from aios_amd.runtime import model_manager as mm
    from aios_amd.runtime.service import AIRuntimeService

    cfg = get_preset("test-tiny")
    ids = [cfg.bos_id] + [int(x) for x in np.random.default_rng(5).integers(20, cfg.vocab_size, 149)]
    body = {"prompt": ids, "max_tokens": 12, "temperature": 0, "ignore_eos": True}
    save_dir = tmp_path / "kv snaps"
    save_dir.mkdir()
    spec = "synthetic:test-tiny#slotsave=" + quote(str(save_dir), safe="/")
    PORT = 19061

    async def post(ses, path, js=None):
        async with ses.post(f"http://127.0.0.1:{PORT}{path}", json=js) as r:
            return r.status, await r.json()

    async def slots(ses):
        async with ses.get(f"http://127.0.0.1:{PORT}/slots") as r:
            assert r.status == 200
            return await r.json()

    async def run():
        mgr = mm.ModelManager(max_batch=2, max_slots=2, base_port=19060)
        svc = AIRuntimeService(mgr, http=True)
        o = {}
        try:
            m = await mgr.load_model("tiny", spec, MAX_CTX, port=PORT)
            assert m.status == "ready", m.error
            assert m.slot_save_path == str(save_dir) and m.scheduler.can_snapshot
            await svc.start_http(m)
            st = m.scheduler.stats
            async with aiohttp.ClientSession() as ses:
                o["first"] = await post(ses, "/v1/completions", body)
                listing = await slots(ses)
                sid = max(listing, key=lambda s: s["n_cached"])["id"]
                o["n_cached"] = listing[sid]["n_cached"]
                o["save"] = await post(ses, f"/slots/{sid}?action=save", {"filename": "a.kv"})
                o["erase"] = await post(ses, f"/slots/{sid}?action=erase")
                o["free_after_erase"] = (m.engine.kv_blocks_free, m.engine.kv_blocks_total)
                o["restore"] = await post(ses, f"/slots/{sid}?action=restore", {"filename": "a.kv"})
                c0, p0 = st["cached_tokens"], st["prefill_tokens"]
                o["second"] = await post(ses, "/v1/completions", body)
                o["reuse"] = (st["cached_tokens"] - c0, st["prefill_tokens"] - p0)
                # the control: after an erase alone the prompt is prefilled whole
                for s in (0, 1):
                    await post(ses, f"/slots/{s}?action=erase")
                c0, p0 = st["cached_tokens"], st["prefill_tokens"]
                o["third"] = await post(ses, "/v1/completions", body)
                o["no_reuse"] = (st["cached_tokens"] - c0, st["prefill_tokens"] - p0)

            # warm start: one good file between a missing one and one saved under another model name
            header, payload, _ = kv_snapshot.read(str(save_dir / "a.kv"))
            kv_snapshot.write(str(save_dir / "other.kv"), dict(header, model="other"), payload)
            assert await mgr.unload_model("tiny")
            warm = spec + "&kvrestore=" + ",".join(["none.kv", "other.kv", "a.kv"])
            m = await mgr.load_model("tiny", warm, MAX_CTX, port=PORT)
            o["warm_status"] = (m.status, m.error)
            await svc.start_http(m)
            st = m.scheduler.stats
            async with aiohttp.ClientSession() as ses:
                o["warm_slots"] = await slots(ses)
                o["warm"] = await post(ses, "/v1/completions", body)
                o["warm_reuse"] = (st["cached_tokens"], st["prefill_tokens"], st["slot_restores"])
        finally:
            await svc.close()
        return o

    o = asyncio.run(run())
    n_rec = len(ids) + body["max_tokens"] - 1   # the record: the prompt and every sampled token that was fed back
    st, first = o["first"]
    assert st == 200 and first["usage"]["completion_tokens"] == 12
    assert o["n_cached"] == n_rec
    st, save = o["save"]
    assert st == 200 and save["n_saved"] == n_rec and save["n_written"] == (save_dir / "a.kv").stat().st_size
    assert o["erase"][0] == 200 and o["erase"][1]["n_erased"] == n_rec
    assert o["free_after_erase"][0] == o["free_after_erase"][1]
    st, rest = o["restore"]
    assert st == 200 and rest["n_restored"] == n_rec and rest["n_read"] == save["n_written"]
    st, second = o["second"]
    assert st == 200 and second["choices"][0]["text"] == first["choices"][0]["text"]
    # all of the prompt but its last token (whose logits the request needs) came from the restored cache
    assert o["reuse"] == (len(ids) - 1, 1), o["reuse"]
    assert o["third"][0] == 200 and o["third"][1]["choices"][0]["text"] == first["choices"][0]["text"]
    assert o["no_reuse"] == (0, len(ids)), o["no_reuse"]

    assert o["warm_status"] == ("ready", ""), o["warm_status"]
    assert sorted(s["n_cached"] for s in o["warm_slots"]) == [0, n_rec]
    st, warm = o["warm"]
    assert st == 200 and warm["choices"][0]["text"] == first["choices"][0]["text"]
    assert o["warm_reuse"] == (len(ids) - 1, 1, 1), o["warm_reuse"]
