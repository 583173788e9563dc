"""The float64 embedding oracle (tests/embed_oracle.py) against hand-computed cases, and the host rule
(runtime/embedding.py) against the oracle."""
import numpy as np
import pytest

import embed_oracle as O


def test_one_row():
    # x = (3, 4): mean(x^2) = 12.5, h = x / sqrt(12.5); unit(h) = (0.6, 0.8) whatever the RMS
    got = O.embed([[3.0, 4.0]], [1.0, 1.0], 0.0, "mean")
    assert got == pytest.approx([0.6, 0.8], abs=1e-15)
    assert O.embed([[3.0, 4.0]], [1.0, 1.0], 0.0, "last") == pytest.approx([0.6, 0.8], abs=1e-15)
    # eps enters the RMS: h = x / sqrt(12.5 + 12.5) = x / 5
    assert O.embed([[3.0, 4.0]], [1.0, 1.0], 12.5, "none") == pytest.approx(np.array([[0.6, 0.8]]), abs=1e-15)


def test_two_rows_each_normed_before_the_mean():
    # (2, 0) and (0, 200) both have h of length sqrt(2): the mean is (1, 1) / sqrt(2), NOT dominated by the
    # long row
    got = O.embed([[2.0, 0.0], [0.0, 200.0]], [1.0, 1.0], 0.0, "mean")
    assert got == pytest.approx([np.sqrt(0.5), np.sqrt(0.5)], abs=1e-15)


def test_norm_weight():
    # h = (sqrt2 * 3, 0) and (0, sqrt2 * 4): mean ~ (3, 4) -> (0.6, 0.8)
    got = O.embed([[1.0, 0.0], [0.0, 1.0]], [3.0, 4.0], 0.0, "mean")
    assert got == pytest.approx([0.6, 0.8], abs=1e-15)
    # a negative weight flips the component
    assert O.embed([[1.0, 1.0]], [1.0, -1.0], 0.0, "mean") == pytest.approx([np.sqrt(0.5), -np.sqrt(0.5)], abs=1e-15)


def test_zero_row_among_others():
    # the zero row has h = 0 (eps > 0 keeps 0 / sqrt(eps) finite): it only lowers the mean's length
    a = O.embed([[3.0, 4.0], [0.0, 0.0]], [1.0, 1.0], 1e-5, "mean")
    assert a == pytest.approx([0.6, 0.8], abs=1e-12) and np.all(np.isfinite(a))
    rows = O.embed([[3.0, 4.0], [0.0, 0.0]], [1.0, 1.0], 1e-5, "none")
    assert np.all(rows[1] == 0.0)


def test_all_zero_rows_give_the_zero_vector():
    for pooling in ("mean", "last"):
        got = O.embed(np.zeros((3, 4)), np.ones(4), 1e-5, pooling)
        assert got.shape == (4,) and np.all(got == 0.0)
    # opposite rows cancel exactly
    assert np.all(O.embed([[1.0, 2.0], [-1.0, -2.0]], [1.0, 1.0], 0.0, "mean") == 0.0)


def test_last_ignores_earlier_rows():
    a = O.embed([[9.0, -7.0], [1e6, 3.0], [3.0, 4.0]], [1.0, 1.0], 0.0, "last")
    assert a == pytest.approx([0.6, 0.8], abs=1e-15)
    b = O.embed([[np.nan, np.nan], [3.0, 4.0]], [1.0, 1.0], 0.0, "last")
    assert b == pytest.approx([0.6, 0.8], abs=1e-15)


def test_none_is_not_l2_normalised():
    h = O.embed([[3.0, 4.0], [1.0, 0.0]], [2.0, 2.0], 0.0, "none")
    assert h.shape == (2, 2)
    assert h[0] == pytest.approx([6.0 / np.sqrt(12.5), 8.0 / np.sqrt(12.5)], abs=1e-15)
    assert h[1] == pytest.approx([2.0 * np.sqrt(2.0), 0.0], abs=1e-15)
    assert np.linalg.norm(h[0]) == pytest.approx(2.0 * np.sqrt(2.0))  # |g| sqrt(d), not 1


def test_normed_rows_flag_only_averages_and_normalises():
    h = np.array([[1.0, 0.0], [0.0, 3.0]])
    assert O.embed(h, pooling="mean", normed_rows=True) == pytest.approx([1 / np.sqrt(10), 3 / np.sqrt(10)], abs=1e-15)
    assert O.embed(h, pooling="last", normed_rows=True) == pytest.approx([0.0, 1.0], abs=1e-15)
    assert np.array_equal(O.embed(h, pooling="none", normed_rows=True), h)


def test_tolerance_condition():
    assert 0 < O.GPU_TOL <= 1e-3 and O.GPU_TOL == 4 * O.GPU_MEASURED


def test_host_rule_matches_the_oracle():
    from aios_amd.runtime import embedding as H

    rng = np.random.default_rng(0)
    x, g = rng.standard_normal((7, 64)), rng.standard_normal(64)
    h = H.normed_rows(x, g, 1e-5)
    assert h == pytest.approx(O.embed(x, g, 1e-5, "none"), abs=1e-14)
    assert H.unit(h.mean(0)) == pytest.approx(O.embed(x, g, 1e-5, "mean"), abs=1e-14)
    assert H.unit(h[-1]) == pytest.approx(O.embed(x, g, 1e-5, "last"), abs=1e-14)
    assert np.all(H.unit(np.zeros(5)) == 0.0)
    assert H.unit(np.array([1e-200, 0.0])) == pytest.approx([1.0, 0.0])  # no underflow in the squares
    assert H.POOLING == {"none": 0, "mean": 1, "last": 3} and H.pooling_code("last") == 3
    with pytest.raises(ValueError):
        H.pooling_code("cls")
