"""Engine.kv_save / kv_restore (csrc/engine.hip, csrc/kernels/kv_snapshot.hip) on Q4_K_M engines of test-tiny and
test-mistral-shape with bf16 and fp8 KV, and the file layer (runtime/kv_snapshot.py) on a real engine.

  * kv_save equals kv_read byte for byte;
  * a restore into another slot of the same engine and into a second engine built from the same seed gives an equal
    kv_read, the same 16 greedy tokens and logits that agree as closely as two plain runs of the untouched decode
    agree with each other (the control is measured here; the decode is deterministic, so both are 0) -- through the
    graph the first run captured, and again after capture_graphs, a B = 2 step included;
  * a restore into a slot that shares blocks through copy_slot leaves the other slot's bytes alone, and after
    releasing everything the pool is whole;
  * every refusal leaves block_table, kv_blocks_free and kv_read as they were.

Not covered: the "pool exhausted" refusal of kv_restore.  A pool holds max_slots x (max_ctx / 128) blocks and a slot
maps at most max_ctx / 128 of them, so with need = the unmapped or shared entries of the slot's row below
ceil(n / 128) and p = the slot's private blocks, need <= max_ctx / 128 - p <= kv_blocks_free always holds: no
sequence of engine calls sizes the pool so that a restore does not fit.  The check precedes every change
(Engine::kv_restore) and stays as the guard it is in shift_context.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_CTX, SLOTS, BATCH = 256, 4, 2
N, STEPS = 200, 16
PRESETS = ["test-tiny", "test-mistral-shape"]
KVS = ["bf16", "fp8_e4m3"]


def fp8_scales(n_layers):
    return [0.05 if i % 2 == 0 else 0.02 for i in range(2 * n_layers)]


def make_engine(preset, kv):
    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset(preset)
    eng = random_engine(cfg, "Q4_K_M", seed=3, max_ctx=MAX_CTX, max_slots=SLOTS, max_batch=BATCH, kv_dtype=kv)
    if kv != "bf16":
        eng.set_kv_scales(fp8_scales(cfg.n_layers))
    return eng, cfg


_ENGINES = {}


def engines(preset, kv):
    """(engine, its twin from the same seed, cfg), all slots released"""
    if (preset, kv) not in _ENGINES:
        a, cfg = make_engine(preset, kv)
        b, _ = make_engine(preset, kv)
        _ENGINES[(preset, kv)] = (a, b, cfg)
    a, b, cfg = _ENGINES[(preset, kv)]
    for e in (a, b):
        for s in range(SLOTS):
            e.release_slot(s)
        assert e.kv_blocks_free == e.kv_blocks_total == SLOTS * MAX_CTX // 128
    return a, b, cfg


CASES = pytest.mark.parametrize("preset,kv", [(p, k) for p in PRESETS for k in KVS])


def tokens(cfg, seed, n):
    return [cfg.bos_id] + [int(t) for t in np.random.default_rng(seed).integers(3, cfg.vocab_size, n - 1)]


def greedy(eng, slot, first, pos, steps=STEPS):
    """steps greedy decode steps from `slot`: (tokens, logits [steps][V])"""
    toks, logits, t = [], [], first
    for i in range(steps):
        t = int(eng.decode([slot], [t], [pos + i])[0])
        toks.append(t)
        logits.append(np.asarray(eng.last_logits(1), np.float32).reshape(-1).copy())
    return toks, np.stack(logits)


def state(eng):
    return ([eng.block_table(s) for s in range(SLOTS)], eng.kv_blocks_free,
            [eng.kv_read(s, MAX_CTX) for s in range(SLOTS)])


@CASES
def test_round_trip_and_decode_from_a_restored_slot(preset, kv):
    eng, twin, cfg = engines(preset, kv)
    toks = tokens(cfg, 11, N)
    first = int(np.asarray(eng.prefill(0, toks, 0, True)).argmax())
    want, want_100 = eng.kv_read(0, N), eng.kv_read(0, 100)
    data = eng.kv_save(0, N)
    assert isinstance(data, bytes) and len(data) == eng.kv_snapshot_bytes(N) == len(want)
    assert data == want, "kv_save differs from kv_read"
    assert eng.kv_save(0, 1) == eng.kv_read(0, 1) and eng.kv_save(0, 129) == eng.kv_read(0, 129)

    # two plain runs of the untouched decode (the second rewrites the same positions): the control
    ref_toks, ref = greedy(eng, 0, first, N)
    again_toks, again = greedy(eng, 0, first, N)
    control = float(np.abs(again - ref).max())
    assert again_toks == ref_toks
    print(f"[{preset}, {kv}] control: two plain runs differ by {control:.3g}")

    def check(label, e, slot):
        assert e.kv_read(slot, N) == want, f"{label}: kv_read differs after the restore"
        got_toks, got = greedy(e, slot, first, N)
        err = float(np.abs(got - ref).max())
        print(f"[{preset}, {kv}] {label}: logits differ by {err:.3g} (control {control:.3g})")
        assert got_toks == ref_toks, f"{label}: tokens differ"
        assert err <= control, f"{label}: logits differ by {err}, two plain runs by {control}"

    # another slot of the same engine, through the B = 1 graph the runs above captured and replayed
    free = eng.kv_blocks_free
    eng.kv_restore(2, data, N)
    assert eng.kv_blocks_free == free - 2 and eng.block_table(2)[2:] == [-1] * (MAX_CTX // 128 - 2)
    check("same engine, slot 2", eng, 2)
    # a second engine from the same seed, which has never seen the prompt
    twin.kv_restore(1, data, N)
    check("second engine, slot 1", twin, 1)

    # after capture_graphs, into a slot that held something longer (its upper block goes back to the pool)
    eng.capture_graphs(BATCH)
    eng.prefill(3, tokens(cfg, 12, 250), 0, False)
    free = eng.kv_blocks_free
    eng.kv_restore(3, eng.kv_save(2, 100), 100)
    assert eng.kv_blocks_free == free + 1 and eng.block_table(3)[1] == -1
    assert eng.kv_read(3, 100) == want_100
    eng.kv_restore(3, data, N)
    check("after capture_graphs, slot 3", eng, 3)
    # B = 2: the restored slot and the original swap rows; each row sees the same step either way
    eng.kv_restore(2, data, N)
    out_a = eng.decode([0, 2], [first, first], [N, N])
    lg_a = np.asarray(eng.last_logits(2), np.float32).reshape(2, -1).copy()
    out_b = eng.decode([2, 0], [first, first], [N, N])
    lg_b = np.asarray(eng.last_logits(2), np.float32).reshape(2, -1)
    assert [int(t) for t in out_a] == [int(t) for t in out_b] == [ref_toks[0]] * 2
    assert float(np.abs(lg_b - lg_a).max()) <= control


@CASES
def test_restore_into_a_sharing_slot_never_writes_through(preset, kv):
    eng, _, cfg = engines(preset, kv)
    eng.prefill(0, tokens(cfg, 21, N), 0, False)
    eng.prefill(2, tokens(cfg, 22, 150), 0, False)
    data = eng.kv_save(2, 150)
    eng.copy_slot(0, 1, N)                      # block 0 shared, the partial block copied
    assert eng.block_table(1)[0] == eng.block_table(0)[0]
    before, free = eng.kv_read(0, MAX_CTX), eng.kv_blocks_free
    eng.kv_restore(1, data, 150)
    assert eng.block_table(1)[0] != eng.block_table(0)[0] and eng.kv_blocks_free == free - 1
    assert eng.kv_read(0, MAX_CTX) == before, "the restore wrote through a shared block"
    assert eng.kv_read(1, 150) == data == eng.kv_read(2, 150)
    dev = eng.kv_device_tables(0)
    assert dev == [eng.kv_blocks_total if b < 0 else b for s in range(SLOTS) for b in eng.block_table(s)]
    for s in range(SLOTS):
        eng.release_slot(s)
    assert eng.kv_blocks_free == eng.kv_blocks_total
    assert not np.frombuffer(eng.kv_read_block(eng.kv_blocks_total), np.uint8).any(), "the null block was written"


@CASES
def test_refusals_change_nothing(preset, kv):
    eng, _, cfg = engines(preset, kv)
    eng.prefill(0, tokens(cfg, 31, N), 0, False)
    eng.prefill(1, tokens(cfg, 32, 140), 0, False)
    eng.copy_slot(0, 2, N)
    data = eng.kv_save(0, N)
    was = state(eng)
    for call, msg in [
        (lambda: eng.kv_restore(1, data[:-1], N), "payload"),
        (lambda: eng.kv_restore(1, data + b"\0", N), "payload"),
        (lambda: eng.kv_restore(1, data, N - 1), "payload"),
        (lambda: eng.kv_restore(1, b"", 0), "n_tokens out of range"),
        (lambda: eng.kv_restore(1, data, MAX_CTX + 1), "n_tokens out of range"),
        (lambda: eng.kv_restore(-1, data, N), "bad slot"),
        (lambda: eng.kv_restore(SLOTS, data, N), "bad slot"),
        (lambda: eng.kv_save(SLOTS, N), "bad slot"),
        (lambda: eng.kv_save(0, 0), "n_tokens out of range"),
        (lambda: eng.kv_save(0, MAX_CTX + 1), "n_tokens out of range"),
    ]:
        with pytest.raises(RuntimeError, match=msg):
            call()
        assert state(eng) == was, f"a refusal ({msg}) changed the engine"


@pytest.mark.parametrize("kv", KVS)
def test_file_layer_on_an_engine(kv, tmp_path):
    from aios_amd.runtime import kv_snapshot as S

    eng, twin, cfg = engines("test-tiny", kv)
    other, _, _ = engines("test-mistral-shape", kv)
    other_kv, _, _ = engines("test-tiny", KVS[1 - KVS.index(kv)])
    toks = tokens(cfg, 41, N)
    eng.prefill(0, toks, 0, False)
    path = str(tmp_path / "s.kv")
    n, written = S.save_slot(eng, 0, toks, path, "m")
    assert n == N and written > eng.kv_snapshot_bytes(N)
    got, nread = S.restore_slot(twin, 2, path, "m", MAX_CTX)
    assert got == toks and nread == written and twin.kv_read(2, N) == eng.kv_read(0, N)

    def refused(field, e, p):
        was = state(e)
        with pytest.raises(S.SnapshotError) as err:
            S.restore_slot(e, 1, p, "m", MAX_CTX)
        assert err.value.field == field, str(err.value)
        assert state(e) == was

    refused("head_dim", other, path)            # a header from another shape
    refused("kv_dtype", other_kv, path)         # another KV dtype
    raw = open(path, "rb").read()
    flipped, cut = str(tmp_path / "f.kv"), str(tmp_path / "c.kv")
    open(flipped, "wb").write(raw[:-100] + bytes([raw[-100] ^ 1]) + raw[-99:])
    refused("crc32", twin, flipped)             # a flipped payload byte
    open(cut, "wb").write(raw[:-4096])
    refused("truncated", twin, cut)             # a truncated file
    if kv != "bf16":                            # a changed fp8 scale, by one ulp
        sc = fp8_scales(cfg.n_layers)
        sc[1] = float(np.nextafter(np.float32(sc[1]), np.float32(1)))
        twin.set_kv_scales(sc)
        try:
            refused("kv_scales_bits", twin, path)
        finally:
            twin.set_kv_scales(fp8_scales(cfg.n_layers))
