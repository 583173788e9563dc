"""tests/context_shift_oracle.py against itself in float64: the re-rotation is RoPE at the new position, shifts
compose, both RoPE modes, the block bookkeeping, and a shifted ReferenceModel cache decodes at the new positions."""
import dataclasses

import numpy as np
import pytest

import context_shift_oracle as C
import kv_paging_oracle as P

THETA = 10000.0


def rows(seed, n, hd=64, lead=(2, 3)):
    return np.random.default_rng(seed).standard_normal(lead + (n, hd))


@pytest.mark.parametrize("neox", [False, True])
def test_rotating_back_is_rope_at_the_new_position(neox):
    x = rows(1, 40)
    pos = np.arange(100, 140)
    for d in (1, 37, 100):
        got = C.rotate_back(C.rope(x, pos, THETA, neox), d, THETA, neox)
        want = C.rope(x, pos - d, THETA, neox)
        assert np.abs(got - want).max() < 1e-12
    # and it is a rotation: pair magnitudes are kept
    k = C.rope(x, pos, THETA, neox)
    assert np.abs(C.pair_hypot(C.rotate_back(k, 11, THETA, neox), neox) - C.pair_hypot(k, neox)).max() < 1e-12


@pytest.mark.parametrize("neox", [False, True])
def test_pair_layout(neox):
    """one pair set, everything else zero: only that pair's two elements change"""
    hd, i = 64, 5
    a, b = (i, i + hd // 2) if neox else (2 * i, 2 * i + 1)
    k = np.zeros((1, hd))
    k[0, a], k[0, b] = 1.0, 0.0
    out = C.rotate_back(k, 3, THETA, neox)
    ang = 3 * THETA ** (-2.0 * i / hd)
    assert np.flatnonzero(out[0]).tolist() == [a, b]
    assert abs(out[0, a] - np.cos(ang)) < 1e-15 and abs(out[0, b] + np.sin(ang)) < 1e-15


@pytest.mark.parametrize("neox", [False, True])
def test_shift_rows_and_values(neox):
    n, keep, d = 50, 7, 13
    x, v = rows(2, n), rows(3, n)
    k = C.rope(x, np.arange(n), THETA, neox)
    k2, v2, moved = C.shift_kv(k, v, keep, d, THETA, neox)
    assert k2.shape[-2] == v2.shape[-2] == n - d and moved.tolist() == [p >= keep for p in range(n - d)]
    assert np.array_equal(k2[..., :keep, :], k[..., :keep, :]) and np.array_equal(v2[..., :keep, :], v[..., :keep, :])
    assert np.array_equal(v2[..., keep:, :], v[..., keep + d:, :])
    # a moved key is the unrotated key with RoPE at its new position
    want = C.rope(x[..., keep + d:, :], np.arange(keep, n - d), THETA, neox)
    assert np.abs(k2[..., keep:, :] - want).max() < 1e-12
    # n_keep + n_discard == n: nothing moves
    k3, v3, moved3 = C.shift_kv(k, v, keep, n - keep, THETA, neox)
    assert np.array_equal(k3, k[..., :keep, :]) and np.array_equal(v3, v[..., :keep, :]) and not moved3.any()
    for bad in ((0, 0), (-1, 1), (40, 11)):
        with pytest.raises(ValueError):
            C.shift_kv(k, v, bad[0], bad[1], THETA, neox)


@pytest.mark.parametrize("neox", [False, True])
def test_nested_shifts_compose(neox):
    """two shifts whose moved regions nest: a row that moved twice is rotated by the sum"""
    n, keep, d1, d2 = 60, 4, 9, 20
    x, v = rows(4, n), rows(5, n)
    k = C.rope(x, np.arange(n), THETA, neox)
    k1, v1, _ = C.shift_kv(k, v, keep, d1, THETA, neox)
    k2, v2, _ = C.shift_kv(k1, v1, keep, d2, THETA, neox)
    once, v_once, _ = C.shift_kv(k, v, keep, d1 + d2, THETA, neox)
    assert np.abs(k2 - once).max() < 1e-12 and np.array_equal(v2, v_once)
    # a larger n_keep in the second shift: rows between the keeps moved once, the tail twice
    keep2 = 15
    k3, _, _ = C.shift_kv(k1, v1, keep2, d2, THETA, neox)
    assert np.abs(k3[..., keep:keep2, :] - C.rope(x[..., keep + d1:keep2 + d1, :], np.arange(keep, keep2), THETA, neox)).max() < 1e-12
    assert np.abs(k3[..., keep2:, :] - C.rope(x[..., keep2 + d1 + d2:, :], np.arange(keep2, n - d1 - d2), THETA, neox)).max() < 1e-12


def test_cache_types_round_trip():
    bits = np.arange(0, 0x7F80, 7, dtype=np.uint16)
    vals = C.bf16_decode(bits)
    assert np.array_equal(C.bf16_round(vals), vals)
    # ties to even: half way between two bf16 values (1 and 1 + 2^-7; 1 + 2^-7 and 1 + 2^-6)
    assert C.bf16_round(np.array([1 + 2.0 ** -8]))[0] == 1.0 and C.bf16_round(np.array([1 + 3 * 2.0 ** -8]))[0] == 1 + 2.0 ** -6
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)
    assert C.FP8_E4M3[0x7E] == 448.0 and C.FP8_E4M3[1] == 2.0 ** -9 and np.isnan(C.FP8_E4M3[0x7F])
    v8 = C.fp8_decode(codes, 0.05)
    assert np.array_equal(C.fp8_round(v8, 0.05), v8)
    assert C.fp8_round(np.array([1e3]), 0.05)[0] == 448 * 0.05


def test_block_bookkeeping():
    m = P.PagedKV(512, 4)
    m.prefill(0, 0, 500)
    assert m.block_table(0) == [0, 1, 2, 3]
    C.shift_blocks(m, 0, 500, 5, 130)          # 370 left: the last block goes back
    m.check()
    assert m.block_table(0) == [0, 1, 2, -1] and m.blocks_free == 13
    m.copy_slot(0, 1, 300)                      # blocks 0, 1 shared, a private copy of the partial one
    assert m.block_table(1)[:2] == [0, 1] and m.block_table(1)[2] >= 0
    before = m.block_table(0)
    C.shift_blocks(m, 1, 300, 100, 100)         # writes [100, 200): both shared blocks un-share
    m.check()
    assert m.block_table(0) == before and [o for _, o, _ in m.unshared] == [0, 1]
    assert m.block_table(1)[2] == -1 and not set(m.block_table(1)[:2]) & {0, 1}
    C.shift_blocks(m, 1, 200, 64, 136)          # an empty tail: only the truncation
    m.check()
    assert m.block_table(1)[1:] == [-1, -1, -1]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from aios_amd.models.config import get_preset
    from aios_amd.models.synthetic import write_synthetic_gguf

    return write_synthetic_gguf(str(tmp_path_factory.mktemp("ctxshift") / "small.gguf"), get_preset("test-small"), "Q4_K_M", seed=7)


@pytest.mark.parametrize("neox", [False, True])
def test_shifted_reference_cache_decodes_at_the_new_positions(small, neox):
    from aios_amd.models.config import ROPE_NEOX, ROPE_NORM
    from aios_amd.models.reference import ReferenceModel

    ref = ReferenceModel.from_gguf(small)
    ref.cfg = dataclasses.replace(ref.cfg, rope_mode=ROPE_NEOX if neox else ROPE_NORM)
    toks = [1] + [int(t) for t in np.random.default_rng(6).integers(3, ref.cfg.vocab_size, 40)]
    n, d = 30, 12
    cache = ref.new_cache()
    ref.forward(toks[:n], cache)
    shifted = C.shift_reference_cache(ref, cache, 0, d)
    assert shifted["len"] == n - d and cache["len"] == n and all(k.shape[0] == n - d for k in shifted["k"] + shifted["v"])
    # layer 0's keys see no other token: with n_keep 0 they are those of a prefill of the surviving tokens
    fresh = ref.new_cache()
    ref.forward(toks[d:n], fresh)
    assert float((shifted["k"][0] - fresh["k"][0]).abs().max()) < 1e-4 * float(fresh["k"][0].abs().max())
    assert np.array_equal(shifted["v"][0].numpy(), cache["v"][0][d:].numpy())
    # one more token: it lands at position n - d in both, and the cache grows there
    out = ref.forward([toks[n]], shifted)
    assert shifted["len"] == n - d + 1 and out.shape == (1, ref.cfg.vocab_size) and bool(np.isfinite(out.numpy()).all())
    # a 1-layer view of the same fact: the new token's layer-0 key equals the fresh cache's after the same step
    ref.forward([toks[n]], fresh)
    assert float((shifted["k"][0][-1] - fresh["k"][0][-1]).abs().max()) < 1e-4 * float(fresh["k"][0].abs().max())
    # the control drops the rows and leaves the keys where they were
    plain = C.shift_reference_cache(ref, cache, 0, d, rotate=False)
    assert np.array_equal(plain["k"][1].numpy(), cache["k"][1][d:].numpy())
