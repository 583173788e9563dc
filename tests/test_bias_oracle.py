"""The logit-bias rule on the host (aios_amd.runtime.sampler: apply_logit_bias, check_logit_bias) and its place in
the chain -- bias, then penalties, then the grammar mask, then the sampler -- on hand-built rows."""
import numpy as np
import pytest

from aios_amd.runtime import sampler as host


def _mask(V, allowed):
    bits = np.zeros(V, np.uint8)
    bits[list(allowed)] = 1
    return np.packbits(bits, bitorder="little").tobytes()


def test_bias_is_applied_before_the_penalties():
    """logit +0.5, bias -1.0, repeat_penalty 2.0, token in the window: bias first gives -0.5 * 2 = -1.0 (the
    penalty's multiply branch); penalty first would give 0.5 / 2 - 1 = -0.75"""
    l = np.zeros(8, np.float32)
    l[3] = 0.5
    out = host.apply_penalties(host.apply_logit_bias(l, [3], [-1.0]), [3], 2.0, 0.0, 0.0)
    assert out.dtype == np.float32 and out[3] == np.float32(-1.0)
    wrong = host.apply_logit_bias(host.apply_penalties(l, [3], 2.0, 0.0, 0.0), [3], [-1.0])
    assert wrong[3] == np.float32(-0.75)  # (the construction tells the two orders apart)
    assert np.array_equal(np.delete(out, 3), np.delete(l, 3))


def test_one_fp32_add_per_entry():
    l = np.array([0.1, 1e8, -3.25], np.float32)
    out = host.apply_logit_bias(l, [0, 1, 2], [0.2, 1.0, 100.0])
    assert out.dtype == np.float32
    assert out[0] == np.float32(0.1) + np.float32(0.2)  # the fp32 sum of the fp32 operands
    assert out[1] == np.float32(1e8) and out[2] == np.float32(96.75)
    assert l[0] == np.float32(0.1)  # a copy: the caller's row is untouched


def test_a_ban_survives_penalties_and_a_presence_bonus():
    l = np.array([1.0, 2.0, 3.0, -1.0], np.float32)
    b = host.apply_logit_bias(l, [2, 3], [-np.inf, -np.inf])
    assert b[2] == -np.inf and b[3] == -np.inf
    # a negative presence penalty adds to the logit; repeat_penalty divides / multiplies it
    out = host.apply_penalties(b, [2, 3, 3], 1.5, -5.0, -2.0)
    assert out[2] == -np.inf and out[3] == -np.inf and np.isfinite(out[:2]).all()
    assert host.sample(out) == 1
    p = host.probabilities(out, 0.8)
    assert p[2] == 0.0 and p[3] == 0.0 and p[:2].sum() == pytest.approx(1.0)


def test_a_masked_token_with_a_large_bias_stays_out():
    V = 16
    l = np.linspace(-1, 1, V).astype(np.float32)
    m = _mask(V, [1, 4, 9])
    out = host.apply_logit_bias(l, [7], [100.0])
    assert int(np.argmax(out)) == 7
    assert host.sample(out, mask=m) == 9
    p = host.probabilities(out, 1.0, mask=m)
    assert p[7] == 0.0 and set(np.nonzero(p)[0].tolist()) == {1, 4, 9}


def test_empty_list_and_empty_entries_leave_the_row_bit_identical():
    l = np.array([0.0, -0.0, 1.5, -np.inf, 3e-41], np.float32)  # (a negative zero and a denormal among them)
    for ids, vals in (([], []), ([-1, -1], [5.0, -np.inf])):
        out = host.apply_logit_bias(l, ids, vals)
        assert out.tobytes() == l.tobytes()
        assert out is not l


def test_check_logit_bias_refuses_what_the_rule_excludes():
    V = 512
    host.check_logit_bias([], [], V)
    host.check_logit_bias([0, V - 1], [-np.inf, 1e30], V)
    host.check_logit_bias(list(range(host.BIAS_MAX)), [0.5] * host.BIAS_MAX, 1024)
    for ids, vals, what in (([1, 2], [0.0], "size"), ([V], [0.0], "range"), ([-1], [0.0], "range"),
                            ([3, 3], [0.0, 1.0], "duplicate"), ([3], [np.inf], "finite"), ([3], [np.nan], "finite"),
                            (list(range(V)), [-np.inf] * V, "banned")):
        with pytest.raises(ValueError, match=what):
            host.check_logit_bias(ids, vals, V)
    with pytest.raises(ValueError, match="more than"):
        host.check_logit_bias(list(range(host.BIAS_MAX + 1)), [0.0] * (host.BIAS_MAX + 1), 1024)
