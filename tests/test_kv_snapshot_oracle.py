"""tests/kv_snapshot_oracle.py on hand-built cases, and the snapshot file layer (runtime/kv_snapshot.py) on the CPU."""
import os
import types

import numpy as np
import pytest

import kv_snapshot_oracle as O

from aios_amd.runtime import kv_snapshot as S


def tiny_pool():
    """1 layer, 3 blocks + null, 1 head, 2-byte rows: byte = (kv, block, row) spelled out"""
    pool = np.zeros((1, 2, 4, 1, O.KV_BLOCK, 2), np.uint8)
    for kv in range(2):
        for b in range(4):
            pool[0, kv, b, 0, :, 0] = np.arange(O.KV_BLOCK)
            pool[0, kv, b, 0, :, 1] = 16 * kv + b
    return pool


def test_pack_follows_the_table_and_stops_at_n():
    pool = tiny_pool()
    table = np.array([[2, 0, 3], [1, 3, 3]])
    p = O.pack(pool, table, 0, 130)
    assert p.shape == O.payload_shape(1, 1, 130, 1, 2)
    # K: rows 0..127 of block 2, then rows 0..1 of block 0
    assert (p[0, 0, 0, :128, 1] == 2).all() and (p[0, 0, 0, 128:, 1] == 0).all()
    assert (p[0, 1, 0, :128, 1] == 16 + 2).all() and (p[0, 1, 0, 128:, 1] == 16).all()
    assert list(p[0, 0, 0, :, 0]) == list(range(128)) + [0, 1]
    # one position: one row of the first block
    one = O.pack(pool, table, 1, 1)
    assert one.shape[3] == 1 and one[0, 0, 0, 0, 1] == 1 and one[0, 1, 0, 0, 1] == 17


def test_unpack_is_packs_inverse_and_touches_nothing_else():
    pool = O.poison_pool(2, 5, 2, 16, 1, seed=3)
    table = np.array([[4, 1, 5], [0, 2, 3]])
    for n in (1, 127, 128, 129, 300):
        payload = np.random.default_rng(n).integers(0, 256, O.payload_shape(2, 2, n, 16, 1), dtype=np.uint8)
        out = O.unpack(pool, table, 1, payload)
        assert (O.pack(out, table, 1, n) == payload).all()
        m = O.touched_mask(pool.shape, table, 1, n)
        assert (out[~m] == pool[~m]).all()
        assert m.sum() == payload.size
        # the other slot's blocks, the null block and the dead rows of the last block are outside the mask
        assert not m[:, :, [4, 1, 5]].any()
        if n % O.KV_BLOCK:
            assert not m[:, :, int(table[1, (n - 1) // O.KV_BLOCK]), :, n % O.KV_BLOCK:].any()


def test_pack_of_unpack_round_trips_a_slot():
    pool = O.poison_pool(1, 4, 1, 8, 2, seed=5)
    table = np.array([[3, 0, 4], [2, 1, 4]])
    saved = O.pack(pool, table, 0, 200)
    moved = O.unpack(pool, table, 1, saved)
    assert (O.pack(moved, table, 1, 200) == saved).all()
    assert (O.pack(moved, table, 0, 200) == saved).all()


# ---------------------------------------------------------------------------------- the file layer
class FakeEngine:
    def __init__(self, fp8=False, scales=None, head_dim=16, theta=10000.0):
        self.config = types.SimpleNamespace(n_layers=2, n_kv_heads=2, head_dim=head_dim, rope_theta=theta, rope_neox=0,
                                            max_ctx=256)
        self.kv_fp8 = fp8
        self.kv_scales = list(scales or [1.0] * 4)
        self.weight_bytes = 1234
        self.store = {}
        self.restored = []

    def weight_type_summary(self):
        return "Q4_K:10 Q6_K:2"

    def nbytes(self, n):
        return 2 * 2 * 2 * n * self.config.head_dim * (1 if self.kv_fp8 else 2)

    def kv_save(self, slot, n):
        return bytes(np.random.default_rng(slot * 1000 + n).integers(0, 256, self.nbytes(n), dtype=np.uint8))

    def kv_restore(self, slot, data, n):
        assert len(data) == self.nbytes(n)
        self.restored.append((slot, bytes(data), n))


def test_file_round_trip_and_atomic_write(tmp_path):
    eng = FakeEngine()
    path = str(tmp_path / "a.kv")
    toks = list(range(5, 45))
    n, written = S.save_slot(eng, 1, toks, path, "m")
    assert n == 40 and written == os.path.getsize(path)
    assert os.listdir(tmp_path) == ["a.kv"]  # (the temporary file is gone)
    header, payload, size = S.read(path)
    assert header["tokens"] == toks and header["n_tokens"] == 40 and size == written
    assert payload == eng.kv_save(1, 40)
    got, nread = S.restore_slot(eng, 3, path, "m", 256)
    assert got == toks and nread == written and eng.restored == [(3, payload, 40)]


def refused(field, eng, path, model="m", max_ctx=256):
    with pytest.raises(S.SnapshotError) as e:
        S.restore_slot(eng, 0, path, model, max_ctx)
    assert e.value.field == field and str(e.value).startswith(field + ":"), str(e.value)
    assert eng.restored == []


def test_file_refusals_name_the_field(tmp_path):
    path = str(tmp_path / "a.kv")
    S.save_slot(FakeEngine(fp8=True, scales=[0.05, 0.02, 0.05, 0.02]), 0, list(range(30)), path, "m")
    refused("head_dim", FakeEngine(fp8=True, scales=[0.05, 0.02, 0.05, 0.02], head_dim=32), path)
    refused("kv_dtype", FakeEngine(), path)
    bumped = float(np.nextafter(np.float32(0.02), np.float32(1)))  # one ulp: bit for bit
    refused("kv_scales_bits", FakeEngine(fp8=True, scales=[0.05, 0.02, 0.05, bumped]), path)
    refused("rope_theta", FakeEngine(fp8=True, scales=[0.05, 0.02, 0.05, 0.02], theta=1e6), path)
    same = FakeEngine(fp8=True, scales=[0.05, 0.02, 0.05, 0.02])
    refused("model", same, path, model="other")
    refused("tokens", same, path, max_ctx=16)
    other = FakeEngine(fp8=True, scales=[0.05, 0.02, 0.05, 0.02])
    other.weight_bytes = 99
    refused("weight_bytes", other, path)
    raw = open(path, "rb").read()
    flipped = str(tmp_path / "flip.kv")
    open(flipped, "wb").write(raw[:-7] + bytes([raw[-7] ^ 0x10]) + raw[-6:])
    refused("crc32", same, flipped)
    cut = str(tmp_path / "cut.kv")
    open(cut, "wb").write(raw[:-1])
    refused("truncated", same, cut)
    open(cut, "wb").write(raw[:10])
    refused("truncated", same, cut)
    open(cut, "wb").write(b"NOTASNAP" + raw[8:])
    refused("magic", same, cut)
    with pytest.raises(FileNotFoundError):
        S.restore_slot(same, 0, str(tmp_path / "none.kv"), "m", 256)
    S.restore_slot(same, 0, path, "m", 256)  # (and the file itself is fine)
    assert len(same.restored) == 1


@pytest.mark.parametrize("name", ["", "a/b", "../x", "..", "x..y", "a\\b", "a\0b", ".", None, 7, "/etc/passwd"])
def test_snapshot_path_takes_bare_names_only(name, tmp_path):
    with pytest.raises(ValueError, match="filename"):
        S.snapshot_path(str(tmp_path), name)


def test_snapshot_path_joins_a_bare_name(tmp_path):
    assert S.snapshot_path(str(tmp_path), "agent.kv") == os.path.join(str(tmp_path), "agent.kv")
