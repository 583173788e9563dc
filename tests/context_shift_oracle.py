"""The context shift in float64 (csrc/ops.h KvShiftArgs: the rule; kernels/kv_shift.hip, Engine::shift_context).

A slot holds positions [0, n).  Given n_keep >= 0 and n_discard >= 1 with n_keep + n_discard <= n:
positions [0, n_keep) stay, [n_keep, n_keep + n_discard) are forgotten, every position p in
[n_keep + n_discard, n) becomes p - n_discard, and the new length is n - n_discard.  A moved V row is the same
bytes.  A moved K row is the stored row -- which has RoPE applied -- rotated by -n_discard positions: pair i
with stored (x, y) and (c, s) = (cos, sin)(n_discard * theta^(-2i / head_dim)) becomes
    x' = x c + y s,    y' = -x s + y c
with pairs (2i, 2i + 1) (ROPE_NORM) or (i, i + head_dim / 2) (ROPE_NEOX); x', y' are then rounded to the cache
type.  QK-norm and the QKV bias are applied before RoPE and need nothing; rotations compose.  These are
llama.cpp's semantics: kept and moved entries are the ones computed in the original context, repositioned.

Everything here is numpy float64 with the token axis second to last: k, v are [..., n, head_dim].
"""
import numpy as np

KV_BLOCK = 128


# ---- RoPE ---------------------------------------------------------------------------------------------------
def angles(pos, head_dim: int, theta: float) -> np.ndarray:
    """[len(pos), head_dim / 2] rotation angles of the pairs at the positions (any real numbers)"""
    i = np.arange(head_dim // 2, dtype=np.float64)
    return np.asarray(pos, np.float64).reshape(-1, 1) * np.power(np.float64(theta), -2.0 * i / head_dim)


def pairs(x: np.ndarray, neox: bool):
    """(first, second) elements of every pair, each [..., head_dim / 2]"""
    h = x.shape[-1] // 2
    return (x[..., :h], x[..., h:]) if neox else (x[..., 0::2], x[..., 1::2])


def unpairs(a: np.ndarray, b: np.ndarray, neox: bool) -> np.ndarray:
    if neox:
        return np.concatenate([a, b], axis=-1)
    out = np.empty(a.shape[:-1] + (2 * a.shape[-1],), np.float64)
    out[..., 0::2], out[..., 1::2] = a, b
    return out


def rope(x: np.ndarray, pos, theta: float, neox: bool) -> np.ndarray:
    """RoPE at positions pos ([n]) of x [..., n, head_dim]: the forward rotation by +angle"""
    x = np.asarray(x, np.float64)
    ang = angles(pos, x.shape[-1], theta)
    c, s = np.cos(ang), np.sin(ang)
    a, b = pairs(x, neox)
    return unpairs(a * c - b * s, a * s + b * c, neox)


def rotate_back(k: np.ndarray, d: int, theta: float, neox: bool) -> np.ndarray:
    """every row of k [..., n, head_dim] rotated by -d positions (the rule's x', y')"""
    k = np.asarray(k, np.float64)
    ang = angles([d], k.shape[-1], theta)
    c, s = np.cos(ang), np.sin(ang)
    x, y = pairs(k, neox)
    return unpairs(x * c + y * s, -x * s + y * c, neox)


# ---- the shift ----------------------------------------------------------------------------------------------
def check_args(n: int, n_keep: int, n_discard: int) -> None:
    if n < 1 or n_keep < 0 or n_discard < 1 or n_keep + n_discard > n:
        raise ValueError(f"context shift: n {n}, n_keep {n_keep}, n_discard {n_discard}")


def shift_kv(k: np.ndarray, v: np.ndarray, n_keep: int, n_discard: int, theta: float, neox: bool):
    """(k', v', moved) of k, v [..., n, head_dim] as float64, not rounded: the new rows [..., n - n_discard,
    head_dim] and the boolean [n - n_discard] of the rows that moved (K rotated); v' rows are v's, unchanged."""
    k, v = np.asarray(k, np.float64), np.asarray(v, np.float64)
    n = k.shape[-2]
    check_args(n, n_keep, n_discard)
    src = n_keep + n_discard
    k2 = np.concatenate([k[..., :n_keep, :], rotate_back(k[..., src:, :], n_discard, theta, neox)], axis=-2)
    v2 = np.concatenate([v[..., :n_keep, :], v[..., src:, :]], axis=-2)
    moved = np.arange(n - n_discard) >= n_keep
    return k2, v2, moved


def pair_hypot(k: np.ndarray, neox: bool) -> np.ndarray:
    """per element of k [..., head_dim], the magnitude hypot(x, y) of the pair it belongs to"""
    x, y = pairs(np.asarray(k, np.float64), neox)
    h = np.hypot(x, y)
    return unpairs(h, h, neox)


# ---- cache element types ------------------------------------------------------------------------------------
def bf16_decode(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_round(x: np.ndarray) -> np.ndarray:
    """float64 -> the nearest bf16 value (ties to even), as float64"""
    u = np.asarray(x, np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _fp8_table() -> np.ndarray:
    t = np.empty(256, np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        mag = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
        if e == 15 and m == 7:
            mag = np.nan
        t[c] = -mag if c & 0x80 else mag
    return t


FP8_E4M3 = _fp8_table()  # OCP e4m3fn: code -> value (0x7f / 0xff: NaN), largest finite 448


def fp8_decode(codes: np.ndarray, scale: float) -> np.ndarray:
    return FP8_E4M3[np.asarray(codes, np.uint8)] * np.float64(scale)


def fp8_round(x: np.ndarray, scale: float) -> np.ndarray:
    """float64 -> the nearest e4m3 value of x / scale (ties to even, saturating at +-448), times scale"""
    import torch

    t = torch.from_numpy(np.asarray(x, np.float64) / np.float64(scale)).clamp(-448.0, 448.0)
    return t.to(torch.float32).to(torch.float8_e4m3fn).to(torch.float64).numpy() * np.float64(scale)


# ---- a ReferenceModel cache ---------------------------------------------------------------------------------
def shift_reference_cache(ref, cache: dict, n_keep: int, n_discard: int, rotate: bool = True) -> dict:
    """A new cache for aios_amd.models.reference.ReferenceModel that holds `cache` shifted: rows dropped, K
    re-rotated and rounded to the model's cache type (kv_bf16 / kv_fp8 with its scales), "len" set.  The next
    forward(tokens, cache) decodes at the new positions.  rotate=False drops the rows only (a control: what a
    shift without the rotation would leave)."""
    import torch

    from aios_amd.models.config import ROPE_NEOX

    cfg = ref.cfg
    neox = cfg.rope_mode == ROPE_NEOX
    check_args(cache["len"], n_keep, n_discard)
    out = {"k": [], "v": [], "len": cache["len"] - n_discard}
    for l in range(cfg.n_layers):
        k = cache["k"][l].numpy().astype(np.float64).transpose(1, 0, 2)  # [Hkv, S, hd]
        v = cache["v"][l].numpy().astype(np.float64).transpose(1, 0, 2)
        if rotate:
            k2, v2, moved = shift_kv(k, v, n_keep, n_discard, cfg.rope_theta, neox)
            if ref.kv_fp8:
                r = fp8_round(k2, ref.kv_scales[2 * l] if ref.kv_scales else 1.0)
            elif ref.kv_bf16:
                r = bf16_round(k2)
            else:
                r = k2
            k2 = np.where(moved[None, :, None], r, k2)
        else:
            keep = np.r_[0:n_keep, n_keep + n_discard:k.shape[1]]
            k2, v2 = k[:, keep], v[:, keep]
        out["k"].append(torch.from_numpy(np.ascontiguousarray(k2.transpose(1, 0, 2))).to(torch.float32))
        out["v"].append(torch.from_numpy(np.ascontiguousarray(v2.transpose(1, 0, 2))).to(torch.float32))
    return out


# ---- block bookkeeping --------------------------------------------------------------------------------------
def shift_blocks(model, slot: int, n: int, n_keep: int, n_discard: int) -> None:
    """Engine::shift_context on a kv_paging_oracle.PagedKV: the blocks of [n_keep, n - n_discard) mapped and
    un-shared, the blocks wholly above the new length unreferenced and unmapped"""
    check_args(n, n_keep, n_discard)
    model.unshared = []
    n_new = n - n_discard
    model.prepare_write(slot, n_keep, n_new)
    row = model.tables[slot]
    for j in range((n_new + KV_BLOCK - 1) // KV_BLOCK, model.maxb):
        model._unref(row[j])
        row[j] = -1
