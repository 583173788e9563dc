"""Plain float64 reference of the device sampler's contract (the rule above SampleArgs in csrc/ops.h) and
the fixed inputs its tests run on: numpy only, no kernel code.  tests/test_sampler_oracle.py checks the
reference, the comparison and the conditions every input promises; tests/test_sampler_dense_gpu.py checks
the kernel.

This is not host.probabilities (aios_amd.runtime.sampler): the device restricts top-p and min-p to the 256
largest logits when top-k is off and clamps top-k to 256; the host sampler does neither.  Wherever the
host's support has at most 256 tokens the two agree (tested).

Not modelled: the kernel treats values more than 30 * T + 1 below the maximum as absent.  Such tokens have
relative probability below e^-30 and never appear in any sample count used here.

Why not five spikes over a floor: with that input a 4096-token slice publishes a handful of candidates and
the merge never holds more than a few dozen.  The inputs here are dense (randn * 2.5), so every slice fills
its 256 candidate slots, the merge's table overflows past 16 slices, and the nucleus has tens to hundreds
of survivors.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from aios_amd.runtime.sampler import apply_penalties, mask_to_bool

SLICE = 4096  # tokens per sampler workgroup (SAMPLE_SLICE)
KCAP = 256    # candidates a slice publishes; the clamp of top-k; the candidate set of top-p / min-p alone
TABLE = 4096  # candidates the merge's table holds (SAMPLE_MAX_CAND)


# ---------------------------------------------------------------------------------- the oracle
def processed_logits(logits, mask=None, window=None, repeat=1.0, presence=0.0, frequency=0.0):
    """fp32 logits after the penalties (in fp32, as the kernel applies them) and the mask (-inf)."""
    l = np.array(logits, dtype=np.float32)
    if window is not None and len(window):
        l = apply_penalties(l, window, repeat, presence, frequency)
    if mask is not None:
        allowed = mask_to_bool(mask, l.shape[0]) if isinstance(mask, (bytes, bytearray)) else np.asarray(mask, bool)
        l[~allowed] = -np.inf
    return l


def _filtered(l, T, top_k, top_p, min_p, thr_shift=0.0, M=None):
    """The filtered rule on processed fp32 logits l: p[V] in float64.  thr_shift moves the top-K threshold
    (tokens exactly at the K-th value stay); M overrides the maximum the weights and min-p refer to."""
    V = l.shape[0]
    l64 = l.astype(np.float64)
    K = min(top_k, KCAP) if top_k > 0 else KCAP
    finite = np.flatnonzero(l64 > -np.inf)
    p = np.zeros(V, np.float64)
    if finite.size == 0:
        return p
    if finite.size > K:
        kth = np.partition(l64[finite], finite.size - K)[finite.size - K]
        keep = finite[(l64[finite] >= kth + thr_shift) | (l64[finite] == kth)]
    else:
        keep = finite
    v = l64[keep]
    if M is None:
        M = float(np.max(l64[finite]))
    z = (v - M) / T
    e = np.exp(z)
    Z = e.sum()
    ok = np.ones(keep.size, bool)
    if top_p < 1.0:
        order = np.lexsort((keep, -v))  # value descending, index ascending
        before = np.cumsum(e[order]) - e[order]
        ok[order] = before < top_p * Z
    if min_p > 0.0:
        ok &= z >= math.log(min_p)
    if ok.any():
        p[keep[ok]] = e[ok] / e[ok].sum()
    return p


def device_distribution(logits, temperature, top_k, top_p, min_p, mask=None, window=None, repeat=1.0, presence=0.0,
                        frequency=0.0):
    """The distribution the device sampler's contract gives one row: p[V] in float64."""
    l = processed_logits(logits, mask, window, repeat, presence, frequency)
    V = l.shape[0]
    if temperature <= 0.0:
        p = np.zeros(V, np.float64)
        p[int(np.argmax(l))] = 1.0  # (the lowest index on ties)
        return p
    if top_k <= 0 and top_p >= 1.0 and min_p <= 0.0:
        z = l.astype(np.float64) / temperature
        e = np.exp(z - np.max(z))
        return e / e.sum()
    return _filtered(l, temperature, top_k, top_p, min_p)


def ambiguous(logits, temperature, top_k, top_p, min_p, mask=None, window=None, repeat=1.0, presence=0.0,
              frequency=0.0):
    """Token ids whose membership of the support flips when a cut moves by the kernel's own resolution:
    top_p * (1 +- 1e-4), the top-K threshold +- (30 T + 1) * 2^-23, min_p * (1 +- 1e-4).  The GPU tests run
    only on inputs for which this is empty."""
    if temperature <= 0.0 or (top_k <= 0 and top_p >= 1.0 and min_p <= 0.0):
        return set()
    l = processed_logits(logits, mask, window, repeat, presence, frequency)
    base = _filtered(l, temperature, top_k, top_p, min_p) > 0
    d = (30.0 * temperature + 1.0) * 2.0 ** -23
    moved = [(top_p, min_p, -d), (top_p, min_p, d)]
    if top_p < 1.0:
        moved += [(top_p * (1 - 1e-4), min_p, 0.0), (top_p * (1 + 1e-4), min_p, 0.0)]
    if min_p > 0.0:
        moved += [(top_p, min_p * (1 - 1e-4), 0.0), (top_p, min_p * (1 + 1e-4), 0.0)]
    out = set()
    for tp, mp, sh in moved:
        other = _filtered(l, temperature, top_k, tp, mp, thr_shift=sh) > 0
        out |= set(np.flatnonzero(other != base).tolist())
    return out


# ---------------------------------------------------------------------------------- the comparison
def bins(p, V):
    """[(name, bool[V])]: two partitions of the token ids -- by slice quartile (id // 4096, four equal groups
    of slices) and by oracle rank (probability descending, id ascending: rank 1, 2-8, 9-64, the rest)."""
    ids = np.arange(V)
    ns = (V + SLICE - 1) // SLICE
    quart = (ids // SLICE) * 4 // ns
    out = [(f"slices q{q}", quart == q) for q in range(4)]
    rank = np.empty(V, np.int64)
    rank[np.lexsort((ids, -p))] = ids + 1
    for name, lo, hi in [("rank 1", 1, 1), ("ranks 2-8", 2, 8), ("ranks 9-64", 9, 64), ("ranks 65-", 65, V)]:
        out.append((name, (rank >= lo) & (rank <= hi)))
    return out


def bin_tolerance(q, n):
    """5 sigma of the binomial count of a bin of mass q in n samples, + 1e-3 for the kernel's fp32 weights
    and __expf against the oracle's float64.  Nothing here is tuned on the device."""
    return 5.0 * math.sqrt(max(q * (1.0 - q), 0.0) / n) + 1e-3


def check_bins(counts, p, n, label=""):
    """counts[V]: how often each token was sampled in n draws.  Every sampled token lies in the oracle's
    support, exactly; every bin's frequency is within bin_tolerance of its oracle mass.  Prints every
    figure before it asserts; returns them."""
    counts = np.asarray(counts)
    V = p.shape[0]
    assert counts.shape == (V,) and int(counts.sum()) == n
    rows = []
    for name, sel in bins(p, V):
        q, f = float(p[sel].sum()), float(counts[sel].sum()) / n
        rows.append((name, f, q, bin_tolerance(q, n)))
        print(f"{label} {name}: sampled {f:.5f} oracle {q:.5f} tol {rows[-1][3]:.5f}")
    outside = np.flatnonzero((counts > 0) & ~(p > 0))
    assert outside.size == 0, f"{label}: {outside.size} sampled tokens outside the oracle's support, e.g. {outside[:8]}"
    for name, f, q, tol in rows:
        assert abs(f - q) <= tol, f"{label} {name}: sampled {f:.5f}, oracle {q:.5f}, tolerance {tol:.5f}"
    return rows


# ---------------------------------------------------------------------------------- the fixed inputs
Case = namedtuple("Case", "name logits T top_k top_p min_p mask window repeat presence frequency",
                  defaults=(None, None, 1.0, 0.0, 0.0))

SETTINGS = [(0, 0.9, 0.0), (40, 0.95, 0.0), (256, 1.0, 0.0), (1000, 1.0, 0.0), (0, 1.0, 0.05), (64, 0.9, 0.02)]
V_DENSE = 9000              # three slices, the last partial
V_CAPACITY = [69632 + 8, 128256, 262144]  # the 17th full slice is the first past the table; 32 slices; 64
N_ROWS, SEEDS = 4096, (101, 102, 103, 104)
N_SAMPLES = N_ROWS * len(SEEDS)


@functools.lru_cache(maxsize=None)
def _dense(V, seed):
    x = np.random.default_rng(seed).standard_normal(V).astype(np.float32) * np.float32(2.5)
    x.setflags(write=False)
    return x


def dense_logits(V=V_DENSE, seed=11):
    """randn(V) * 2.5 from a seeded generator (read-only: shared between tests)"""
    return _dense(V, seed)


@functools.lru_cache(maxsize=None)
def capacity_logits(V):
    """dense logits with the global maximum planted at V - 2 (the last slice) and the second best in slice 0,
    0.5 and 0.25 above the largest drawn value"""
    x = _dense(V, 1000 + V % 997).copy()
    top = float(x.max())
    x[V - 2] = np.float32(top + 0.5)
    x[1234] = np.float32(top + 0.25)
    x.setflags(write=False)
    return x


TIE_HI, TIE_MID = SLICE + 255, SLICE + 254


@functools.lru_cache(maxsize=None)
def tie_logits():
    """-40 everywhere but slice 1: 400 tokens at exactly 0.0 (the ids with id % 256 < 25), 1.0 and 0.5 at the
    two highest thread positions of the slice"""
    x = np.full(V_DENSE, -40.0, np.float32)
    ids = np.arange(SLICE, 2 * SLICE)
    x[ids[ids % 256 < 25]] = 0.0
    x[TIE_HI], x[TIE_MID] = 1.0, 0.5
    x.setflags(write=False)
    return x


def tie_case():
    return Case("tie overflow", tie_logits(), 0.8, 3, 1.0, 0.0)


def pack_mask(allowed):
    return np.packbits(np.asarray(allowed, np.uint8), bitorder="little").tobytes()


def every_second_mask(V):
    return pack_mask(np.arange(V) % 2 == 0)


FEW_ALLOWED = (8210, 8476, 8579)  # all in the last, partial slice of V_DENSE; the nucleus drops the first


def few_allowed_mask():
    a = np.zeros(V_DENSE, bool)
    a[list(FEW_ALLOWED)] = True
    return pack_mask(a)


def dense_cases():
    x = dense_logits()
    return [Case(f"dense T{T} k{k} p{p} m{m}", x, T, k, p, m) for T in (0.1, 0.8, 3.0) for k, p, m in SETTINGS]


def masked_penalised_case():
    """every second token banned; the penalty window covers the oracle's top five tokens of the masked row"""
    x = dense_logits()
    mask = every_second_mask(V_DENSE)
    top5 = np.argsort(-processed_logits(x, mask), kind="stable")[:5].tolist()
    return Case("dense masked penalised", x, 0.8, 64, 0.9, 0.02, mask, top5 + [top5[0]], 1.3, 0.5, 0.25)


def capacity_cases(V):
    x = capacity_logits(V)
    return [Case(f"capacity V{V} k{k} p{p} m{m}", x, 0.8, k, p, m) for k, p, m in SETTINGS]


def few_allowed_case():
    return Case("few allowed", dense_logits(), 0.8, 40, 0.9, 0.0, few_allowed_mask())


def mixed_cases():
    """the six settings of the mixed launch: row b uses setting b % 6"""
    x = dense_logits()
    top = np.argsort(-x, kind="stable")[:4].tolist()
    return [Case("mixed greedy", x, 0.0, 0, 1.0, 0.0),
            Case("mixed temperature", x, 0.8, 0, 1.0, 0.0),
            Case("mixed top-k", x, 0.8, 40, 1.0, 0.0),
            Case("mixed top-p", x, 0.8, 0, 0.9, 0.0),
            Case("mixed min-p", x, 0.8, 0, 1.0, 0.05),
            Case("mixed all", x, 0.8, 64, 0.9, 0.02, None, top + [top[0]], 1.3, 0.5, 0.25)]


def all_gpu_cases():
    """every fixed input the GPU file samples from (the deterministic equalities reuse capacity_logits)"""
    out = dense_cases() + [masked_penalised_case(), tie_case(), few_allowed_case()] + mixed_cases()
    for V in V_CAPACITY:
        out += capacity_cases(V)
    return out


def oracle_of(c):
    return device_distribution(c.logits, c.T, c.top_k, c.top_p, c.min_p, c.mask, c.window, c.repeat, c.presence,
                               c.frequency)


def ambiguous_of(c):
    return ambiguous(c.logits, c.T, c.top_k, c.top_p, c.min_p, c.mask, c.window, c.repeat, c.presence, c.frequency)


# ---------------------------------------------------------------------------------- the two suspected faults
def _slice_candidates(l, K, order):
    """per slice: the ids at or above the slice's K-th largest value (ties kept), cut to KCAP in `order`
    ("value": the best first; "thread": the kernel's (id % 256, id // 256 % 16) slot order)"""
    out = []
    for s0 in range(0, l.shape[0], SLICE):
        ids = s0 + np.flatnonzero(l[s0:s0 + SLICE] > -np.inf)
        if ids.size > K:
            kth = np.partition(l[ids], ids.size - K)[ids.size - K]
            ids = ids[l[ids] >= kth]
        if order == "thread":
            ids = ids[np.lexsort((ids // 256 % 16, ids % 256))]
        else:
            ids = ids[np.lexsort((ids, -l[ids]))]
        out.append(ids[:KCAP])
    return out


def mutant_distribution(c, fault):
    """What the kernel would sample from with one of the two suspected faults.  "merge": the table keeps,
    slice-major, only the first TABLE of the slices' candidates, while the weights and min-p still refer to
    the true maximum.  "ties": a slice fills its KCAP slots in thread order, not by value."""
    l = processed_logits(c.logits, c.mask, c.window, c.repeat, c.presence, c.frequency)
    K = min(c.top_k, KCAP) if c.top_k > 0 else KCAP
    cand = np.concatenate(_slice_candidates(l, K, "thread" if fault == "ties" else "value"))
    if fault == "merge":
        cand = cand[:TABLE]
    r = np.full_like(l, -np.inf)
    r[cand] = l[cand]
    return _filtered(r, c.T, c.top_k, c.top_p, c.min_p, M=float(l.max()))
