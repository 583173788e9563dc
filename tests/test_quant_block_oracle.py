"""The raw-block oracle (quant_block_oracle.py) against the repository's dequantizers, and the conditions the
GPU tests rely on: finite values, max|w| <= 8, at most 0.1 % of a matrix inside the bf16 boundary band."""
import numpy as np
import pytest

import quant_block_oracle as O
from aios_amd.gguf.quants import BLOCK_INFO, GGMLType as T, dequantize, kquant_scale_min, type_size

ROWS, K = 128, 512
TYPES = [T.Q4_K, T.Q5_K, T.Q6_K, T.Q4_0, T.Q8_0, T.F16, T.BF16, T.Q2_K, T.Q3_K, T.IQ4_NL, T.IQ4_XS, T.Q4_1, T.Q5_0,
         T.Q5_1, T.F32]
CASES = [(t, f) for t in TYPES for f in O.families(t)]
IDS = [f"{t.name}-{f}" for t, f in CASES]


@pytest.mark.parametrize("t,family", CASES, ids=IDS)
def test_oracle_matches_dequantize(t, family):
    m = O.matrix(t, ROWS, K, family)
    assert m.raw.dtype == np.uint8 and m.raw.size == type_size(t, ROWS * K)
    ref = dequantize(m.raw, t).reshape(ROWS, K)
    assert np.isfinite(m.w).all() and np.isfinite(ref).all()
    assert np.array_equal(m.w.astype(np.float32), ref)  # (float32(float64 value) == the float32 dequantizer)
    assert np.abs(m.w).max() <= 8.0
    assert (m.a >= 0).all() and (m.bm >= 0).all() and (m.s >= np.abs(m.w) * (1 - 1e-15)).all()
    if t not in O.AFFINE:
        assert np.array_equal(m.s, np.abs(m.w))


@pytest.mark.parametrize("t,family", CASES, ids=IDS)
def test_boundary_band_cap(t, family):
    """elements a correct fp32 decoder may round to either bf16 neighbour: at most 0.1 % of the matrix"""
    m = O.matrix(t, ROWS, K, family)
    assert O.boundary_band(m.w, m.s).mean() <= 1e-3


def test_bf16_round():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -9), 0.0, 3.0e-6])
    r, ulp, dist = O.bf16_round(v)
    assert np.array_equal(r[:4], [1.0, 1.0, 1.0 + 2.0 ** -6, -1.0])  # ties to even; below the tie: down
    assert np.array_equal(ulp[:4], [2.0 ** -7] * 4) and np.array_equal(dist[:3], [2.0 ** -8, 0.0, 0.0])
    assert dist[4] == np.inf and O.bf16_bits(r)[0] == 0x3F80
    import torch

    x = np.random.default_rng(0).standard_normal(4096) * np.exp(np.random.default_rng(1).uniform(-20, 3, 4096))
    x = x.astype(np.float32)  # (fp32 -> bf16 in one rounding: torch agrees)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(O.bf16_bits(O.bf16_round(x.astype(np.float64))[0]), want)


def _fields(t, raw):
    b = raw.reshape(-1, BLOCK_INFO[t][1])
    return [np.ascontiguousarray(b[:, o:o + 2]).view(np.float16).ravel() for o in O.FP16[t]], b


@pytest.mark.parametrize("t", [t for t in TYPES if t not in O.ELEMENT_TYPES], ids=lambda t: t.name)
def test_families_hold_what_they_name(t):
    f, _ = _fields(t, O.matrix(t, ROWS, K, "random").raw)
    for v in f:  # both signs, normal fp16, 2^-13 < |v| < 2^-3
        assert (v > 0).any() and (v < 0).any() and (np.abs(v) > 2.0 ** -13).all() and (np.abs(v) < 2.0 ** -3).all()
    if len(f) == 2:  # signs independent: all four combinations
        assert len({(a > 0, c > 0) for a, c in zip(f[0], f[1])}) == 4
    f, _ = _fields(t, O.matrix(t, ROWS, K, "zeros").raw)
    bits = [v.view(np.uint16) for v in f]
    assert (bits[0] == 0).any() and (bits[0] == 0x8000).any() and ((bits[0] & 0x7FFF) == O.F16_SUBNORMAL).any()
    if len(f) == 2:
        assert (bits[1] == 0).any() and (bits[1] == 0x8000).any()
        assert ((bits[0] == 0) & (bits[1] == 0)).any() and ((bits[0] == 0) & (bits[1] != 0)).any()
    _, b = _fields(t, O.matrix(t, ROWS, K, "saturated").raw)
    for lo, hi in O.REGIONS[t].values():
        assert (b[:, lo:hi] == 0xFF).all(1).any() and (b[:, lo:hi] == 0).all(1).any()
    allr = np.concatenate([b[:, lo:hi] for lo, hi in O.REGIONS[t].values()], 1)
    assert (allr == 0xFF).all(1).any() and (allr == 0).all(1).any()
    if t == T.Q6_K:
        for sc in (0x7F, 0x80):
            for code in (0x00, 0xFF):
                assert ((b[:, 192:208] == sc).all(1) & (b[:, :192] == code).all(1)).any()
    if t == T.Q8_0:
        assert (b[:, 2:] == 0x80).all(1).any() and (b[:, 2:] == 0x7F).all(1).any()
    if t in O.SPLIT_TYPES:
        _, b = _fields(t, O.matrix(t, ROWS, K, "split").raw)
        if t == T.Q2_K:
            sc, mn = b[:, :16] & 15, b[:, :16] >> 4
        else:
            sc, mn = kquant_scale_min(b[:, 4:16])
        assert ((sc == 0) ^ (mn == 0)).all() and (sc == 0).any() and (mn == 0).any()


@pytest.mark.parametrize("kind", O.ACTS)
def test_activations(kind):
    from aios_amd.models.reference import ReferenceModel
    import torch

    x = O.activations(kind, 3, K, int8=True)
    assert x.dtype == np.float32 and x.shape == (3, K) and np.isfinite(x).all()
    v, over = O._q8_units(x)
    v = v[~over.repeat(32, 1)]
    assert (np.abs(np.abs(v - np.floor(v)) - 0.5) >= 1e-3).all()
    assert np.isfinite(ReferenceModel.q8(torch.from_numpy(x)).numpy()).all()
    if kind == "offset":
        assert x.mean() > 7.5
    if kind == "sparse":
        assert not x[1].any() and not x[0, 64:96].any() and not x[0, K - 32:].any() and x[0, 37] == 1e4
    if kind == "tiny":
        assert 0 < np.abs(x[:, 288:320]).max() < 1e-37 and np.abs(x[:, 96:128]).max() < 1e-29
