"""Host-side sampling for the first token after prefill (the decode steps sample on device).

Semantics match the device sampler (aios::sample_kernel): temperature <= 0 -> greedy argmax,
else sample from softmax(logits / T) restricted to the top-k (if k > 0) and nucleus top-p (if
0 < p < 1), always within the grammar's allowed-token bitmask when one is given.

Logit processors, in the device sampler's order: `apply_logit_bias` (a sparse list of (id, bias), one
fp32 add each, -inf = ban) first, then `apply_penalties` (repeat / presence / frequency over a window
of the row's recent tokens, llama.cpp's rule), both before the mask and everything else;
min-p after top-k / top-p: a survivor stays only while exp((l - M) / T) >= min_p, M the largest
allowed (penalised) logit -- a ratio test on the tempered distribution, so it intersects with the
nucleus instead of renormalising before it.  Greedy ignores min-p.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np


def mask_to_bool(mask: bytes, vocab: int) -> np.ndarray:
    bits = np.unpackbits(np.frombuffer(mask, dtype=np.uint8), bitorder="little")
    return bits[:vocab].astype(bool)


PEN_MAX = 256  # longest penalty window (the device sampler reads one window entry per thread)


def penalty_window(repeat_last_n: int) -> int:
    """the request field `repeat_last_n` as a window length: < 0 or > PEN_MAX clamp to PEN_MAX"""
    n = int(repeat_last_n)
    return PEN_MAX if n < 0 or n > PEN_MAX else n


def apply_penalties(logits: np.ndarray, recent: Sequence[int], repeat_penalty: float = 1.0,
                    presence_penalty: float = 0.0, frequency_penalty: float = 0.0) -> np.ndarray:
    """Penalised copy of `logits`, in fp32 with the device sampler's operations.  For every distinct
    token t with c >= 1 occurrences in `recent` (entries < 0 are empty):
    l[t] = l[t] / repeat_penalty if l[t] > 0 else l[t] * repeat_penalty, then
    l[t] -= c * frequency_penalty + presence_penalty."""
    l = np.array(logits, dtype=np.float32)
    ids = np.asarray([t for t in recent if 0 <= t < l.shape[0]], dtype=np.int64)
    if ids.size == 0:
        return l
    toks, cnt = np.unique(ids, return_counts=True)
    rp, pp, fp = np.float32(repeat_penalty), np.float32(presence_penalty), np.float32(frequency_penalty)
    x = l[toks]
    x = np.where(x > 0, x / rp, x * rp).astype(np.float32)
    l[toks] = x - (cnt.astype(np.float32) * fp + pp)
    return l


BIAS_MAX = 512  # longest logit-bias list (the device sampler reads two list entries per thread)


def check_logit_bias(ids: Sequence[int], vals: Sequence[float], vocab: int) -> None:
    """ValueError unless (ids, vals) is a list the sampler takes: at most BIAS_MAX entries, ids distinct
    and in [0, vocab), every bias a finite number or -inf, fewer bans than the vocabulary has tokens"""
    if len(ids) != len(vals):
        raise ValueError("logit_bias: size mismatch")
    if len(ids) > BIAS_MAX:
        raise ValueError(f"logit_bias: more than {BIAS_MAX} entries")
    if any(not 0 <= int(t) < vocab for t in ids):
        raise ValueError("logit_bias: token out of range")
    if len(set(int(t) for t in ids)) != len(ids):
        raise ValueError("logit_bias: duplicate token")
    if any(np.isnan(v) or v == np.inf for v in vals):
        raise ValueError("logit_bias: bias must be finite or -inf")
    if sum(1 for v in vals if v == -np.inf) >= vocab:
        raise ValueError("logit_bias: every token banned")


def apply_logit_bias(logits: np.ndarray, ids: Sequence[int], vals: Sequence[float]) -> np.ndarray:
    """Biased copy of `logits`: l[id] = l[id] + bias, one fp32 add per entry (the device sampler's
    operation); entries with id < 0 are empty, a -inf bias bans the token.  Applied in front of
    `apply_penalties`, which then sees the biased logit."""
    l = np.array(logits, dtype=np.float32)
    for t, v in zip(ids, vals):
        if 0 <= int(t) < l.shape[0]:
            l[int(t)] = l[int(t)] + np.float32(v)
    return l


def probabilities(logits: np.ndarray, temperature: float, top_k: int = 0, top_p: float = 1.0,
                  mask: Optional[bytes] = None, min_p: float = 0.0) -> np.ndarray:
    """The distribution `sample` draws from at temperature > 0 (fp64): mask, top-k and nucleus top-p
    on softmax(logits / T), then min-p."""
    l = np.asarray(logits, dtype=np.float64).copy()
    if mask is not None:
        allowed = mask_to_bool(mask, l.shape[0])
        if allowed.any():
            l[~allowed] = -np.inf
    l = l / temperature
    if top_k and 0 < top_k < l.shape[0]:
        kth = np.partition(l, -top_k)[-top_k]
        l[l < kth] = -np.inf
    l -= np.max(l)
    p = np.exp(l)
    p /= p.sum()
    if 0.0 < top_p < 1.0:
        order = np.argsort(-p)
        cum = np.cumsum(p[order])
        cut = order[np.searchsorted(cum, top_p) + 1:]
        p[cut] = 0.0
        p /= p.sum()
    if min_p > 0.0:  # (l is (logit - M) / T here: the log of the ratio to the best allowed token)
        p[np.exp(l) < min_p] = 0.0
        p /= p.sum()
    return p


def sample(logits: np.ndarray, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
           mask: Optional[bytes] = None, rng: Optional[np.random.Generator] = None, *, min_p: float = 0.0) -> int:
    if temperature <= 0.0 or (mask is not None and not mask_to_bool(mask, len(logits)).any()):
        l = np.asarray(logits, dtype=np.float64).copy()
        if mask is not None:
            allowed = mask_to_bool(mask, l.shape[0])
            if allowed.any():
                l[~allowed] = -np.inf
        return int(np.argmax(l))
    rng = rng or np.random.default_rng()
    p = probabilities(logits, temperature, top_k, top_p, mask, min_p)
    return int(rng.choice(p.shape[0], p=p))


LOGPROB_MAX_TOP = 20  # alternatives per token (OpenAI's top_logprobs cap; ops.h LOGPROB_MAX_TOP)


def logprobs(logits: np.ndarray, token: int, top_n: int = 0):
    """Per-token log-probabilities of the RAW row (before penalties, mask and temperature), in float64:
    (logprob of `token`, ids, logprobs) with the min(top_n, V) largest logits, value descending, ties
    by the lower id -- the device kernel's rule (csrc/ops.h LogprobArgs)."""
    l = np.asarray(logits, dtype=np.float64)
    V = l.shape[0]
    if not 0 <= int(token) < V:
        raise ValueError(f"logprobs: token {token} outside [0, {V})")
    if not 0 <= int(top_n) <= LOGPROB_MAX_TOP:
        raise ValueError(f"logprobs: top_n outside 0..{LOGPROB_MAX_TOP}")
    m = np.max(l)
    lse = m + np.log(np.sum(np.exp(l - m)))
    # (lexsort: last key first -- value descending, then id ascending)
    ids = np.lexsort((np.arange(V), -l))[:min(int(top_n), V)]
    return float(l[int(token)] - lse), [int(i) for i in ids], [float(x) for x in l[ids] - lse]


def all_allowed(vocab: int) -> bytes:
    m = np.zeros((vocab + 7) // 8, np.uint8) + 0xFF
    return m.tobytes()
