"""The prompt-scoring oracle (tests/score_oracle.py) against hand-computed rows and the logprob oracle."""
import math

import numpy as np
import pytest

import logprob_oracle
import score_oracle

LN2, LN3, LN4 = math.log(2.0), math.log(3.0), math.log(4.0)


def test_uniform_row_ties_follow_the_id():
    # four equal logits: lse = c + ln 4; every id ties with the target, the lower ids order before it
    l = [1.5, 1.5, 1.5, 1.5]
    for t in range(4):
        lp, rank, best, best_lp = score_oracle.score(l, t)
        assert lp == pytest.approx(-LN4, abs=1e-15)
        assert (rank, best) == (t, 0)
        assert best_lp == pytest.approx(-LN4, abs=1e-15)


def test_ties_at_and_around_the_target():
    # values: ids 1, 3, 4, 6 tie at 0; id 2 is above, ids 0 and 5 below
    l = [-1.0, 0.0, math.log(2.0), 0.0, 0.0, -1.0, 0.0]
    lse = math.log(2 * math.exp(-1.0) + 4.0 + 2.0)
    # target 4: one value above (id 2), two tied ids below it (1, 3)
    lp, rank, best, best_lp = score_oracle.score(l, 4)
    assert rank == 3 and best == 2
    assert lp == pytest.approx(-lse, abs=1e-15) and best_lp == pytest.approx(LN2 - lse, abs=1e-15)
    assert score_oracle.score(l, 1)[1] == 1   # the lowest of the tied ids: only id 2 before it
    assert score_oracle.score(l, 6)[1] == 4   # the highest: id 2 and the three tied ids
    assert score_oracle.score(l, 2)[1] == 0   # the argmax
    assert score_oracle.score(l, 0)[1] == 5   # everything but id 5 (tied, higher id)
    assert score_oracle.score(l, 5)[1] == 6


def test_duplicated_maximum_reports_the_lowest_id():
    l = [0.0, 2.0, 1.0, 2.0]
    lp, rank, best, best_lp = score_oracle.score(l, 3)
    assert best == 1 and rank == 1
    assert lp == best_lp == pytest.approx(2.0 - math.log(1.0 + 2 * math.exp(2.0) + math.exp(1.0)), abs=1e-15)


def test_minus_inf_target():
    l = [0.0, -np.inf, 0.0]
    lp, rank, best, best_lp = score_oracle.score(l, 1)
    assert lp == -np.inf and rank == 2 and best == 0
    assert best_lp == pytest.approx(-LN2, abs=1e-15)
    # two -inf entries tie with each other, by id
    assert score_oracle.score([-np.inf, 1.0, -np.inf], 2)[1] == 2
    assert score_oracle.score([-np.inf, 1.0, -np.inf], 0)[1] == 1


def test_no_target():
    lp, rank, best, best_lp = score_oracle.score([0.0, math.log(3.0)], -1)
    assert math.isnan(lp) and rank == -1 and best == 1
    assert best_lp == pytest.approx(LN3 - LN4, abs=1e-15)


def test_single_entry_vocabulary():
    assert score_oracle.score([7.25], 0) == (0.0, 0, 0, 0.0)
    lp, rank, best, best_lp = score_oracle.score([7.25], -1)
    assert math.isnan(lp) and (rank, best, best_lp) == (-1, 0, 0.0)


def test_large_magnitudes_do_not_overflow():
    lp, rank, best, best_lp = score_oracle.score([3e4, 3e4 + 1.0], 0)
    assert lp == pytest.approx(-math.log(1.0 + math.e), abs=1e-12) and rank == 1 and best == 1


@pytest.mark.parametrize("V", [1, 2, 257, 4099])
def test_agrees_with_the_logprob_oracle(V):
    rng = np.random.default_rng(V)
    l = rng.standard_normal(V).astype(np.float32)
    if V > 8:  # ties, a duplicated maximum, a -inf
        l[5] = l[3]
        l[7] = l[2] = l.max() + 1.0
        l[1] = -np.inf
    for t in sorted({0, V - 1, int(np.argmax(l)), min(5, V - 1), min(1, V - 1)}):
        lp, rank, best, best_lp = score_oracle.score(l, t)
        x, ids, lps = logprob_oracle.logprobs(l, t, min(20, V))
        assert lp == x or (np.isneginf(lp) and np.isneginf(x))
        assert best == int(ids[0]) and best_lp == float(lps[0])
        if rank < len(ids):
            assert int(ids[rank]) == t
        assert (rank == 0) == (best == t)


def test_rows_helper_takes_strided_views():
    rng = np.random.default_rng(3)
    buf = rng.standard_normal((3, 20))
    lp, rank, best, best_lp = score_oracle.score_rows(buf[:, :17], [4, -1, 16])
    for r, t in enumerate([4, -1, 16]):
        one = score_oracle.score(buf[r, :17], t)
        assert (rank[r], best[r], best_lp[r]) == one[1:]
        assert lp[r] == one[0] or (math.isnan(lp[r]) and math.isnan(one[0]))
