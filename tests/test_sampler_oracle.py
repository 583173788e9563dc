"""The float64 sampler oracle (tests/sampler_oracle.py) against the host sampler where the two must agree,
the documented difference where they must not, the comparison (check_bins) against samples of the oracle
and of the two suspected kernel faults, and the condition every fixed GPU input promises (no token within
the kernel's resolution of a cut).  CPU only."""
import numpy as np
import pytest

import sampler_oracle as O
from aios_amd.runtime import sampler as host

V3 = O.V_DENSE


def spike_logits(V, idx):
    base = np.full(V, -30.0, np.float32)
    for j, i in enumerate(idx):
        base[i] = 1.0 - 0.5 * j
    return base


def draw(p, n, seed):
    return np.bincount(np.random.default_rng(seed).choice(p.shape[0], size=n, p=p), minlength=p.shape[0])


# ---------------------------------------------------------------------------------- oracle == host
@pytest.mark.parametrize("V,top_k,top_p,min_p", [
    (32000, 0, 0.7, 0.0), (32000, 3, 0.9, 0.0), (128256, 4, 1.0, 0.0), (5000, 0, 1.0, 0.0),  # test_kernels_gpu
    (V3, 0, 1.0, 0.2), (V3, 4, 0.9, 0.2)])                                                   # test_sample_processors_gpu
def test_oracle_equals_host_on_spikes(V, top_k, top_p, min_p):
    base = spike_logits(V, [5, 4097, 9000 % V, 20001 % V, V - 2] if V != V3 else [5, 4097, 8500, 4000, 8998])
    p = O.device_distribution(base, 0.8, top_k, top_p, min_p)
    h = host.probabilities(base, 0.8, top_k, top_p, None, min_p)
    assert np.count_nonzero(h > 1e-9) <= 5
    assert np.max(np.abs(p - h)) < 1e-12


def test_oracle_equals_host_on_spikes_masked_and_penalised():
    base = spike_logits(V3, [5, 4097, 8500, 4000, 8998])
    bits = np.ones(V3, bool)
    bits[5] = False
    mask = O.pack_mask(bits)
    assert np.max(np.abs(O.device_distribution(base, 0.8, 0, 1.0, 0.2, mask=mask)
                         - host.probabilities(base, 0.8, 0, 1.0, mask, 0.2))) < 1e-12
    pen = host.apply_penalties(base, [5], 1.0, 1.0, 0.0)
    assert np.max(np.abs(O.device_distribution(base, 0.8, 0, 1.0, 0.2, window=[5], presence=1.0)
                         - host.probabilities(pen, 0.8, 0, 1.0, None, 0.2))) < 1e-12


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("min_p", [0.0, 0.05])
@pytest.mark.parametrize("top_p", [0.5, 0.9, 1.0])
@pytest.mark.parametrize("top_k", [1, 4, 40, 256])
def test_oracle_equals_host_on_dense(top_k, top_p, min_p, masked):
    x = O.dense_logits()
    mask = O.every_second_mask(V3) if masked else None
    h = host.probabilities(x, 0.8, top_k, top_p, mask, min_p)
    assert np.count_nonzero(h) <= 256
    p = O.device_distribution(x, 0.8, top_k, top_p, min_p, mask=mask)
    assert abs(p.sum() - 1.0) < 1e-12
    assert np.max(np.abs(p - h)) < 1e-12


def test_oracle_differs_from_host_as_documented():
    """top-p alone on dense logits: the device's nucleus is taken over the 256 largest logits, the host's
    over the whole vocabulary -- a subset of the top 256, a smaller one, with more mass on each token"""
    x = O.dense_logits()
    p = O.device_distribution(x, 0.8, 0, 0.95, 0.0)
    h = host.probabilities(x, 0.8, 0, 0.95)
    top256 = set(np.argsort(-x, kind="stable")[:256].tolist())
    sp, sh = set(np.flatnonzero(p).tolist()), set(np.flatnonzero(h).tolist())
    assert sp <= top256 and sp < sh
    assert np.max(np.abs(p - h)) > 1e-4


def test_oracle_greedy_and_unfiltered():
    x = O.dense_logits().copy()
    x[100] = x[7000] = 30.0  # a tie: the lowest index
    p = O.device_distribution(x, 0.0, 40, 0.9, 0.1)
    assert p[100] == 1.0 and p.sum() == 1.0
    x = O.dense_logits()
    z = x.astype(np.float64) / 0.8
    want = np.exp(z - z.max())
    assert np.max(np.abs(O.device_distribution(x, 0.8, 0, 1.0, 0.0) - want / want.sum())) < 1e-15
    assert np.array_equal(O.device_distribution(x, 0.8, 1000, 1.0, 0.0), O.device_distribution(x, 0.8, 256, 1.0, 0.0))
    assert np.count_nonzero(O.device_distribution(x, 0.8, 1000, 1.0, 0.0)) == 256


def test_oracle_nucleus_tie_order():
    """equal values rank by index: the nucleus cut between two tied tokens keeps the lower id"""
    x = np.full(600, -20.0, np.float32)
    x[500], x[20], x[300] = 2.0, 1.0, 1.0
    w = np.exp(np.array([0.0, -1.0, -1.0]))
    p = O.device_distribution(x, 1.0, 3, float((w[0] + 0.5 * w[1]) / w.sum()), 0.0)
    assert set(np.flatnonzero(p).tolist()) == {500, 20}
    assert abs(p[500] - w[0] / (w[0] + w[1])) < 1e-12


def test_ambiguous_finds_near_cuts():
    x = np.full(V3, -40.0, np.float32)
    x[10], x[20], x[30], x[40] = 3.0, 2.0, 1.0, np.float32(1.0 - 1e-6)
    assert O.ambiguous(x, 0.8, 3, 1.0, 0.0) == {40}           # within 25 * 2^-23 below the third value
    assert O.ambiguous(x, 0.8, 2, 1.0, 0.0) == set()
    e = np.exp((x[[10, 20, 30, 40]].astype(np.float64) - 3.0) / 0.8)
    assert O.ambiguous(x, 0.8, 4, float(e[0] / e.sum()) * (1 + 5e-5), 0.0) == {20}  # the mass before token 20
    assert O.ambiguous(x, 0.8, 4, 1.0, float(e[1]) * (1 + 5e-5)) == {20}
    assert O.ambiguous(x, 0.0, 4, 0.5, 0.5) == set() and O.ambiguous(x, 0.8, 0, 1.0, 0.0) == set()


# ---------------------------------------------------------------------------------- the fixed GPU inputs
def test_gpu_inputs_are_unambiguous():
    cases = O.all_gpu_cases()
    assert len(cases) == 18 + 3 + 6 + 18
    for c in cases:
        assert O.ambiguous_of(c) == set(), c.name
        p = O.oracle_of(c)
        assert abs(p.sum() - 1.0) < 1e-12, c.name


def test_gpu_inputs_exercise_what_they_claim():
    """the dense cases have nuclei of tens to hundreds of survivors, the capacity inputs keep their best two
    tokens at the two ends of the vocabulary, the penalty window moves the top tokens"""
    sizes = {c.name: np.count_nonzero(O.oracle_of(c)) for c in O.dense_cases()}
    assert sizes["dense T0.8 k0 p0.9 m0.0"] >= 20 and sizes["dense T3.0 k0 p0.9 m0.0"] >= 100
    assert sizes["dense T0.8 k256 p1.0 m0.0"] == 256 == sizes["dense T0.8 k1000 p1.0 m0.0"]
    for V in O.V_CAPACITY:
        x = O.capacity_logits(V)
        order = np.argsort(-x, kind="stable")
        assert order[0] == V - 2 and order[1] == 1234
        for c in O.capacity_cases(V):
            p = O.oracle_of(c)
            assert p[V - 2] == p.max() and p[1234] > 0
            if c.top_k != 40:  # survivors in the slices the table never reached
                assert p[16 * O.SLICE:].sum() > 0.01, c.name
    c = O.masked_penalised_case()
    plain = O.device_distribution(c.logits, c.T, c.top_k, c.top_p, c.min_p, c.mask)
    assert np.argmax(plain) in c.window and np.argmax(O.oracle_of(c)) != np.argmax(plain)
    p = O.oracle_of(O.few_allowed_case())
    assert set(np.flatnonzero(p).tolist()) == set(O.FEW_ALLOWED[1:])
    t = O.oracle_of(O.tie_case())
    assert np.count_nonzero(t) == 402 and t[O.TIE_HI] == t.max()


# ---------------------------------------------------------------------------------- the comparison
@pytest.mark.parametrize("seed", range(20))
def test_check_bins_accepts_the_oracles_own_samples(seed):
    for c in (O.capacity_cases(128256)[0], O.dense_cases()[7], O.tie_case()):
        p = O.oracle_of(c)
        O.check_bins(draw(p, O.N_SAMPLES, seed), p, O.N_SAMPLES, c.name)
    c = O.mixed_cases()[3]
    p = O.oracle_of(c)
    O.check_bins(draw(p, 4096, seed), p, 4096, c.name)  # (the mixed launch's n)


@pytest.mark.parametrize("setting", [0, 2, 3, 4])
def test_check_bins_rejects_a_truncated_merge(setting):
    """fault 1 at V = 128256: the table keeps the first 16 slices' candidates -- every K = 256 setting"""
    c = O.capacity_cases(128256)[setting]
    p, q = O.oracle_of(c), O.mutant_distribution(c, "merge")
    assert q[128256 - 2] == 0 and abs(q.sum() - 1.0) < 1e-12
    with pytest.raises(AssertionError):
        O.check_bins(draw(q, O.N_SAMPLES, 5), p, O.N_SAMPLES, c.name)


@pytest.mark.parametrize("setting", [1, 5])
def test_truncated_merge_is_harmless_at_small_top_k(setting):
    """32 * 40 and 32 * 64 candidates fit the table: the mutant is the oracle"""
    c = O.capacity_cases(128256)[setting]
    assert np.max(np.abs(O.mutant_distribution(c, "merge") - O.oracle_of(c))) < 1e-12


def test_check_bins_rejects_slots_in_thread_order():
    """fault 2 on the tie input: the zeros of threads 0-15 fill the slice's slots, 1.0 and 0.5 are dropped"""
    c = O.tie_case()
    p, q = O.oracle_of(c), O.mutant_distribution(c, "ties")
    assert q[O.TIE_HI] == 0 and q[O.TIE_MID] == 0 and np.count_nonzero(q) == 256
    with pytest.raises(AssertionError):
        O.check_bins(draw(q, O.N_SAMPLES, 5), p, O.N_SAMPLES, c.name)
    # by value, the cap drops tied tokens only
    assert np.count_nonzero(O.mutant_distribution(c, "value")) == 256


def test_check_bins_rejects_a_token_outside_the_support():
    c = O.dense_cases()[6]
    p = O.oracle_of(c)
    counts = draw(p, O.N_SAMPLES, 1)
    i, j = int(np.flatnonzero(p == 0)[0]), int(np.argmax(counts))
    counts[i] += 1
    counts[j] -= 1
    with pytest.raises(AssertionError, match="outside"):
        O.check_bins(counts, p, O.N_SAMPLES)
