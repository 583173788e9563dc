"""Prompt scoring, the host rule (csrc/ops.h ScoreArgs is the device kernel's): for a raw logits row l[0..V)
and a target id t,

    lse = log sum_i exp(l_i);  lp = l[t] - lse
    rank = #{ i : l_i > l_t, or l_i == l_t and i < t }     (0: the target is the argmax)
    best = the lowest id among the maxima;  best_lp = l[best] - lse
    t < 0: no target -- lp NaN, rank -1, best / best_lp still reported

The RAW distribution, before penalties, the grammar mask and the temperature (sampler.logprobs' convention).
A -inf logit has logprob -inf; a row that is all -inf or holds a NaN is unspecified.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from .sampler import LOGPROB_MAX_TOP


def score_row(logits: np.ndarray, target: int):
    """(lp, rank, best, best_lp) of one row, in float64"""
    l = np.asarray(logits, dtype=np.float64)
    V = l.shape[0]
    if int(target) >= V:
        raise ValueError(f"score_row: target {target} outside [0, {V})")
    m = np.max(l)
    lse = m + np.log(np.sum(np.exp(l - m)))
    best = int(np.argmax(l))  # (the first of the maxima)
    if int(target) < 0:
        return float("nan"), -1, best, float(l[best] - lse)
    t = int(target)
    rank = int(np.count_nonzero(l > l[t]) + np.count_nonzero(l[:t] == l[t]))
    return float(l[t] - lse), rank, best, float(l[best] - lse)


def score_rows(logits: np.ndarray, targets: Sequence[int], top_n: int = 0) -> dict:
    """The native Engine.score_prefill's result for the rows logits[T][V] and their targets: lp, best_lp
    (float32 [T]), rank, best (int32 [T]) and, when top_n > 0, ids (int32 [T][n]) / lps (float32 [T][n]),
    n = min(top_n, V): each row's n largest logits, value descending, ties by the lower id."""
    if not 0 <= int(top_n) <= LOGPROB_MAX_TOP:
        raise ValueError(f"score_rows: top_n outside 0..{LOGPROB_MAX_TOP}")
    L = np.asarray(logits, dtype=np.float64)
    T, V = L.shape
    if len(targets) != T:
        raise ValueError("score_rows: one target per row")
    out = dict(lp=np.zeros(T, np.float32), best_lp=np.zeros(T, np.float32), rank=np.zeros(T, np.int32),
               best=np.zeros(T, np.int32))
    n = min(int(top_n), V)
    if top_n > 0:
        out["ids"] = np.zeros((T, n), np.int32)
        out["lps"] = np.zeros((T, n), np.float32)
    for i in range(T):
        out["lp"][i], out["rank"][i], out["best"][i], out["best_lp"][i] = score_row(L[i], targets[i])
        if top_n > 0:
            m = np.max(L[i])
            lse = m + np.log(np.sum(np.exp(L[i] - m)))
            ids = np.lexsort((np.arange(V), -L[i]))[:n]
            out["ids"][i] = ids
            out["lps"][i] = L[i][ids] - lse
    return out
