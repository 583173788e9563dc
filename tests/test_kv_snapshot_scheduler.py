"""Scheduler.save_slot / restore_slot / erase_slot / slots on a recording fake engine (no device, no model): the
engine's next token is a function of the tokens the slot holds, its "cache" is that token list, and kv_save /
kv_restore move it as bytes."""
import threading
import time
import types

import numpy as np
import pytest

from aios_amd.models.synthetic import synthetic_vocab
from aios_amd.runtime import kv_snapshot
from aios_amd.runtime.scheduler import GenRequest, Scheduler, SlotBusy, SlotsUnsupported
from aios_amd.runtime.tokenizer import SpmTokenizer

V = 512
EOS = 2
MAX_CTX = 64
PROMPT = [1] + list(range(100, 119))          # 20 tokens
ROW = 4 * 2 * 8 * 2                           # payload bytes per position: 2 layers, K and V, 2 heads, head_dim 8, bf16


@pytest.fixture(scope="module")
def tok():
    t, s, ty = synthetic_vocab(V)
    return SpmTokenizer(t, s, ty, 1, EOS)


def nxt(ctx):
    return 40 + (len(ctx) * 7 + sum(ctx[-2:])) % 200


class Fake:
    """the engine surface the scheduler uses (plain steps); log: every call in order"""

    def __init__(self, snapshots=True):
        self.config = types.SimpleNamespace(n_layers=2, n_kv_heads=2, head_dim=8, rope_theta=10000.0, rope_neox=0,
                                            max_ctx=MAX_CTX)
        self.kv_fp8, self.kv_scales, self.weight_bytes = False, [1.0] * 4, 77
        self.ctx, self.log = {}, []
        self.entered, self.gate = threading.Event(), threading.Event()
        self.gate.set()
        if snapshots:
            self.kv_save, self.kv_restore = self._kv_save, self._kv_restore

    def weight_type_summary(self):
        return "Q4_K:4"

    def prefill(self, slot, ids, start=0, want_logits=True):
        self.log.append(("prefill", slot, len(ids), start))
        assert start <= len(self.ctx.get(slot, []))
        self.ctx[slot] = self.ctx.get(slot, [])[:start] + list(ids)
        self._slot = slot
        return np.zeros(V, np.float32)

    def sample_first(self, pos, temperature, top_k, top_p, seed, mask):
        return nxt(self.ctx[self._slot])

    def decode(self, slots, toks, pos, temps, topk, seed, mask, topp, seeds):
        self.entered.set()
        assert self.gate.wait(30)
        self.log.append(("decode", list(slots), list(toks), list(pos)))
        for s, t, p in zip(slots, toks, pos):
            self.ctx[s] = self.ctx[s][:p] + [t]
        return [nxt(self.ctx[s]) for s in slots]

    def shift_context(self, slot, n_tokens, n_keep, n_discard):
        c = self.ctx[slot][:n_tokens]
        self.ctx[slot] = c[:n_keep] + c[n_keep + n_discard:]
        return n_tokens - n_discard

    def release_slot(self, slot):
        self.log.append(("release", slot))
        self.ctx.pop(slot, None)

    def _kv_save(self, slot, n):
        self.log.append(("kv_save", slot, n))
        assert 1 <= n <= len(self.ctx[slot])
        return b"".join(int(t).to_bytes(2, "little") * (ROW // 2) for t in self.ctx[slot][:n])

    def _kv_restore(self, slot, data, n):
        self.log.append(("kv_restore", slot, n))
        assert len(data) == n * ROW
        self.ctx[slot] = [int.from_bytes(data[i * ROW:i * ROW + 2], "little") for i in range(n)]


def generate(sched, **kw):
    kw.setdefault("prompt_ids", list(PROMPT))
    kw.setdefault("stop_ids", [])
    ev, box = threading.Event(), {}
    sched.submit(GenRequest(on_done=lambda res: (box.__setitem__(0, res), ev.set()), **kw))
    return ev, box


def finish(sched, **kw):
    ev, box = generate(sched, **kw)
    assert ev.wait(30)
    assert box[0].finish_reason in ("length", "stop"), box[0].error
    return box[0]


@pytest.fixture
def sched(tok):
    s = Scheduler(Fake(), tok, max_batch=4, max_slots=2, max_ctx=MAX_CTX, grammar=None)
    yield s
    s.engine.gate.set()
    s.close()


def used_slot(sched):
    return max(sched.slot_cache, key=lambda s: len(sched.slot_cache[s]))


def test_save_writes_exactly_the_record(sched, tmp_path):
    eng = sched.engine
    finish(sched, max_tokens=5)
    slot = used_slot(sched)
    record = list(sched.slot_cache[slot])
    assert record == PROMPT + eng.ctx[slot][len(PROMPT):] and len(record) == len(PROMPT) + 4 == len(eng.ctx[slot])
    path = str(tmp_path / "a.kv")
    got = sched.save_slot(slot, path)
    assert got["n_saved"] == len(record) and got["n_written"] == (tmp_path / "a.kv").stat().st_size
    assert eng.log[-1] == ("kv_save", slot, len(record))
    assert sched.slot_cache[slot] == record and sched.stats["slot_saves"] == 1
    header, payload, _ = kv_snapshot.read(path)
    assert header["tokens"] == record and header["model"] == sched.name and len(payload) == len(record) * ROW
    assert sched.slots() == [{"id": s, "is_processing": False, "n_cached": len(sched.slot_cache[s])} for s in (0, 1)]


def test_save_after_a_context_shift_stops_at_n_keep(sched, tmp_path):
    eng = sched.engine
    res = finish(sched, max_tokens=60, context_shift=True, n_keep=8)
    assert res.context_shifts >= 1
    slot = used_slot(sched)
    assert sched.slot_cache[slot] == PROMPT[:8]  # what _pick_slot trusts; the engine holds more
    assert len(eng.ctx[slot]) > 8
    assert sched.save_slot(slot, str(tmp_path / "s.kv"))["n_saved"] == 8
    assert eng.log[-1] == ("kv_save", slot, 8)
    empty = 1 - slot
    with pytest.raises(kv_snapshot.SnapshotError, match="tokens"):
        sched.save_slot(empty, str(tmp_path / "e.kv"))
    assert not (tmp_path / "e.kv").exists()


def test_restore_sets_the_record_and_the_next_request_reuses_it(sched, tmp_path):
    eng = sched.engine
    finish(sched, max_tokens=5)
    src = used_slot(sched)
    saved = list(sched.slot_cache[src])
    path = str(tmp_path / "a.kv")
    sched.save_slot(src, path)
    assert sched.erase_slot(src) == {"n_erased": len(saved)}
    assert sched.slot_cache[src] == [] and src not in eng.ctx and eng.log[-1] == ("release", src)
    dst = 1 - src
    got = sched.restore_slot(dst, path)
    assert got["n_restored"] == len(saved) and got["n_read"] == (tmp_path / "a.kv").stat().st_size
    assert sched.slot_cache[dst] == saved == eng.ctx[dst]
    assert sched.stats["slot_saves"] == sched.stats["slot_restores"] == sched.stats["slot_erases"] == 1
    # a request with that prefix: admitted into the restored slot, only the remainder prefilled
    eng.log.clear()
    cached, prefilled = sched.stats["cached_tokens"], sched.stats["prefill_tokens"]
    prompt = saved + [300, 301, 302]
    res = finish(sched, prompt_ids=prompt, max_tokens=2)
    assert eng.log[0] == ("prefill", dst, 3, len(saved))
    assert res.cached_prompt_tokens == len(saved)
    assert sched.stats["cached_tokens"] - cached == len(saved) and sched.stats["prefill_tokens"] - prefilled == 3
    # the restored run continues as the original would: the fake's next token depends on the whole context
    assert res.token_ids[0] == nxt(prompt)


def test_refusals_leave_the_record(sched, tmp_path):
    finish(sched, max_tokens=3)
    slot = used_slot(sched)
    record = list(sched.slot_cache[slot])
    path = str(tmp_path / "a.kv")
    sched.save_slot(slot, path)
    for bad in (-1, 2, "0", True, None):
        for call in (lambda: sched.save_slot(bad, path), lambda: sched.restore_slot(bad, path), lambda: sched.erase_slot(bad)):
            with pytest.raises(ValueError, match="unknown slot"):
                call()
    with pytest.raises(FileNotFoundError):
        sched.restore_slot(slot, str(tmp_path / "none.kv"))
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:-3] + bytes([raw[-3] ^ 4]) + raw[-2:])
    with pytest.raises(kv_snapshot.SnapshotError, match="crc32"):
        sched.restore_slot(slot, path)
    assert sched.slot_cache[slot] == record and sched.stats["slot_restores"] == 0
    assert not any(c[0] == "kv_restore" for c in sched.engine.log)


def test_a_busy_slot_is_refused(sched, tmp_path):
    eng = sched.engine
    eng.gate.clear()
    ev, box = generate(sched, max_tokens=6)
    assert eng.entered.wait(30)                  # the worker is inside a decode step of the request
    busy = [s for s in sched.slot_cache if s not in sched.free_slots]
    assert len(busy) == 1
    errs = []

    def act(fn, *a):
        try:
            fn(*a)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=act, args=(sched.save_slot, busy[0], str(tmp_path / "b.kv"))),
               threading.Thread(target=act, args=(sched.restore_slot, busy[0], str(tmp_path / "b.kv"))),
               threading.Thread(target=act, args=(sched.erase_slot, busy[0]))]
    for t in threads:
        t.start()
    limit = time.time() + 30
    while len(sched._ops) < 3 and time.time() < limit:  # the three actions wait for the worker
        time.sleep(0.001)
    assert len(sched._ops) == 3
    eng.gate.set()                               # the step ends; the actions run before the next one
    for t in threads:
        t.join(30)
    assert len(errs) == 3 and all(isinstance(e, SlotBusy) and "slot busy" in str(e) for e in errs), errs
    assert ev.wait(30) and box[0].finish_reason == "length" and len(box[0].token_ids) == 6
    assert not any(c[0] in ("kv_save", "kv_restore", "release") for c in eng.log)
    assert not (tmp_path / "b.kv").exists()
    assert sched.stats["slot_saves"] == sched.stats["slot_restores"] == sched.stats["slot_erases"] == 0
    assert [s["is_processing"] for s in sched.slots()] == [False, False]


def test_an_engine_without_snapshots_refuses(tok, tmp_path):
    s = Scheduler(Fake(snapshots=False), tok, max_batch=4, max_slots=2, max_ctx=MAX_CTX, grammar=None)
    try:
        assert not s.can_snapshot
        for call in (lambda: s.save_slot(0, str(tmp_path / "a")), lambda: s.restore_slot(0, str(tmp_path / "a")),
                     lambda: s.erase_slot(0)):
            with pytest.raises(SlotsUnsupported, match="single-GPU engines only"):
                call()
        assert [x["id"] for x in s.slots()] == [0, 1]
    finally:
        s.close()
    with pytest.raises(RuntimeError, match="closed"):
        s.slots()
