"""Float64 oracle of the prompt-scoring rule (csrc/ops.h ScoreArgs), independent of the device kernel and of
runtime/scoring.py: lse by np.logaddexp.reduce, rank and best from a full stable sort.

    lse = log sum_i exp(l_i) over the raw row l[0..V)
    lp = l[t] - lse
    rank = #{ i : l_i > l_t, or l_i == l_t and i < t }     (0: the target is the argmax)
    best = the lowest id among the maxima;  best_lp = l[best] - lse
    t < 0: no target -- lp NaN, rank -1, best / best_lp still reported

A -inf logit has logprob -inf; a row that is all -inf or holds a NaN is unspecified.  The same convention as
logprob_oracle.py: the raw distribution, before penalties, the grammar mask and the temperature.
"""
import numpy as np


def score(logits, target):
    """(lp, rank, best, best_lp) of one row in float64"""
    l = np.asarray(logits, dtype=np.float64)
    assert l.ndim == 1 and l.shape[0] >= 1 and int(target) < l.shape[0]
    lse = np.logaddexp.reduce(l)
    # a stable ascending sort of -l keeps equal values in id order: value descending, then id ascending
    order = np.argsort(-l, kind="stable")
    best = int(order[0])
    with np.errstate(invalid="ignore"):
        best_lp = float(l[best] - lse)
        if int(target) < 0:
            return float("nan"), -1, best, best_lp
        rank = int(np.nonzero(order == int(target))[0][0])
        return float(l[int(target)] - lse), rank, best, best_lp


def score_rows(logits, targets):
    """rows [R][V] (any row stride: pass the view logits[:, :V]) -> lp [R], rank [R], best [R], best_lp [R]"""
    L = np.asarray(logits)
    R = L.shape[0]
    lp, rank = np.zeros(R), np.zeros(R, np.int64)
    best, best_lp = np.zeros(R, np.int64), np.zeros(R)
    for r in range(R):
        lp[r], rank[r], best[r], best_lp[r] = score(L[r], targets[r])
    return lp, rank, best, best_lp
