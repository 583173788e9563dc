"""The float64 logprob oracle (tests/logprob_oracle.py) against rows worked by hand, and the host rule
(runtime/sampler.py: logprobs) against the oracle."""
import math

import numpy as np
import pytest

import logprob_oracle as O
from aios_amd.runtime import sampler as host


def test_known_probabilities():
    # p = (0.1, 0.2, 0.3, 0.4), shifted by a constant: logprobs are log p, the shift cancels
    p = np.array([0.1, 0.2, 0.3, 0.4])
    x, ids, lps = O.logprobs(np.log(p) + 7.0, 1, 3)
    assert x == pytest.approx(math.log(0.2), abs=1e-12)
    assert list(ids) == [3, 2, 1]
    assert lps == pytest.approx([math.log(0.4), math.log(0.3), math.log(0.2)], abs=1e-12)
    x, ids, lps = O.logprobs(np.log(p), 0, 0)  # top_n = 0: the token alone
    assert x == pytest.approx(math.log(0.1), abs=1e-12) and len(ids) == 0 and len(lps) == 0


def test_tie_goes_to_the_lower_id():
    # ids 1 and 3 tie at the top, ids 0 and 2 tie below: p = (1, e, 1, e) / (2 + 2e)
    x, ids, lps = O.logprobs([0.0, 1.0, 0.0, 1.0], 3, 4)
    z = math.log(2 + 2 * math.e)
    assert list(ids) == [1, 3, 0, 2]
    assert lps == pytest.approx([1 - z, 1 - z, -z, -z], abs=1e-12)
    assert x == pytest.approx(1 - z, abs=1e-12)


def test_minus_infinity_entry():
    # id 1 has probability 0: it closes the list with logprob -inf, and the rest is p = (1/3, 2/3)
    x, ids, lps = O.logprobs([0.0, -np.inf, math.log(2.0)], 1, 3)
    assert x == -np.inf
    assert list(ids) == [2, 0, 1]
    assert lps[:2] == pytest.approx([math.log(2 / 3), math.log(1 / 3)], abs=1e-12) and lps[2] == -np.inf
    # one finite logit: logprob 0, then the -inf entries in id order
    x, ids, lps = O.logprobs([-np.inf, -np.inf, 5.0, -np.inf], 2, 3)
    assert x == 0.0 and list(ids) == [2, 0, 1] and lps[0] == 0.0 and np.all(lps[1:] == -np.inf)


def test_top_n_above_the_vocabulary():
    x, ids, lps = O.logprobs([0.0, 0.0, 0.0], 2, 20)
    assert list(ids) == [0, 1, 2] and lps == pytest.approx([-math.log(3)] * 3, abs=1e-12)
    lp, idv = O.padded([0.0, 0.0, 0.0], 2, 20)
    assert list(idv) == [2, 0, 1, 2] + [-1] * 17
    assert lp[:4] == pytest.approx([-math.log(3)] * 4, abs=1e-12) and np.all(lp[4:] == -np.inf)


@pytest.mark.parametrize("V,top_n", [(5, 20), (512, 0), (512, 5), (4097, 20)])
def test_host_rule_matches_the_oracle(V, top_n):
    rng = np.random.default_rng(V + top_n)
    l = (rng.standard_normal(V) * 2).astype(np.float32)
    l[rng.integers(0, V, 3)] = l.max()          # ties at the top
    l[rng.integers(0, V, 2)] = -np.inf
    for tok in (0, V - 1, int(np.argmax(l))):
        x, ids, lps = host.logprobs(l, tok, top_n)
        ox, oids, olps = O.logprobs(l, tok, top_n)
        assert ids == list(oids)
        assert x == pytest.approx(ox, abs=1e-9) or (x == ox == -np.inf)
        assert np.allclose(lps, olps, rtol=0, atol=1e-9, equal_nan=False) or np.array_equal(lps, olps)


def test_host_rule_rejects_bad_arguments():
    with pytest.raises(ValueError):
        host.logprobs(np.zeros(4, np.float32), 4, 0)
    with pytest.raises(ValueError):
        host.logprobs(np.zeros(4, np.float32), 0, 21)
