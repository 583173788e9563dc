"""Float64 oracle of the per-token logprob rule (csrc/ops.h LogprobArgs), independent of the device kernel
and of runtime/sampler.py: lse by np.logaddexp.reduce, the alternatives by a full stable sort.

    lse = log sum_i exp(l_i) over the raw row l[0..V)
    logprob(token) = l[token] - lse
    alternatives: the min(top_n, V) largest l_i, value descending, ties by the lower id, each l_i - lse

A -inf logit has logprob -inf; a row that is all -inf or holds a NaN is unspecified.
"""
import numpy as np

MAX_TOP = 20

# Value tolerance of the device kernel against this oracle (the ids are exact): four times the largest
# |gpu - oracle| measured over every case of tests/test_logprobs_gpu.py on an MI355X, 1.730e-06 (the dense
# N(0, 0.1^2) row at V = 32000; profiles/logprobs.txt has every case).  The margin covers other boxes,
# compilers and math intrinsics.  It has to stay at or below 1e-3: the smallest error an adversarial case
# there produces is ~0.05, so a measured error near 1e-3 would be a bug, not a reason to raise it.
# The cases' values (l, lse, l - lse) reach magnitudes of 16 to 32, where one fp32 ulp is 1.9e-6.
GPU_TOL = 4 * 1.730e-06
assert GPU_TOL <= 1e-3


def logprobs(logits, token, top_n):
    """(logprob of `token`, ids [n], logprobs [n]) in float64, n = min(top_n, V)"""
    l = np.asarray(logits, dtype=np.float64)
    assert l.ndim == 1 and 0 <= int(token) < l.shape[0] and 0 <= int(top_n) <= MAX_TOP
    lse = np.logaddexp.reduce(l)
    # a stable ascending sort of -l keeps equal values in id order: value descending, then id ascending
    order = np.argsort(-l, kind="stable")[:min(int(top_n), l.shape[0])]
    with np.errstate(invalid="ignore"):
        return float(l[int(token)] - lse), order.astype(np.int64), l[order] - lse


def padded(logits, token, top_n):
    """the device layout of one row: (lp [MAX_TOP + 1], id [MAX_TOP + 1]) -- entry 0 the token, then the
    alternatives, then id -1 / logprob -inf"""
    x, ids, lps = logprobs(logits, token, top_n)
    lp = np.full(MAX_TOP + 1, -np.inf)
    idv = np.full(MAX_TOP + 1, -1, np.int64)
    lp[0], idv[0] = x, int(token)
    lp[1:1 + len(ids)] = lps
    idv[1:1 + len(ids)] = ids
    return lp, idv
