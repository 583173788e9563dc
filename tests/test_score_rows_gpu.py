"""The row-scoring kernel (score_rows_kernel in csrc/kernels/score_rows.hip) through the raw op
`_engine.score_rows`, against the float64 oracle of its rule (tests/score_oracle.py): rank and best exact,
values within a tolerance.

Shapes: V from 1 over the 256-thread block's edges (255, 256, 257), below one unrolled pass (1023), a ragged
multi-pass row (4099) to the served vocabularies (32000, 151936); R = 1, 3 and 70 rows; ldl = V, V + 1 and
V + 13, so the row bases take every alignment modulo 16 bytes and the kernel's scalar head and tail run at
every length.  The pad columns [V, ldl) hold +inf and NaN: an over-read shows in lse, best or rank.

Row kinds (every kind at every V with R = 70; the short launches start at different kinds): dense N(0, 1)
with the target at the argmax, id 0, id V - 1 and none (-1); a peaked row (one logit 1e4 above the rest, every
other term underflows); a row near 3e4 (a naive exp overflows); a row with -inf entries, the target among
them; a row whose target ties with 3 other ids, lower and higher, under a duplicated maximum.

Tolerance: logprob_oracle.GPU_TOL for rows with max |l| <= 32 -- the same arithmetic (an fp32 max, a sum of
exp, a log and one subtraction) at the same magnitudes -- and GPU_TOL * max |l| / 32 above (the rows near 3e4
and the peaked rows' 1e4), since one ulp grows with the magnitude.
"""
import numpy as np
import pytest
import torch

import logprob_oracle
import score_oracle as O

pytestmark = pytest.mark.gpu

TOL = logprob_oracle.GPU_TOL
VS = [1, 255, 256, 257, 1023, 4099, 32000, 151936]
RS = [1, 3, 70]
PADS = [0, 1, 13]
SENT_F, SENT_I = 123.0, -7
KINDS = 8


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_row(kind, V, rng, flip):
    """(logits [V] fp32, target) of one row kind"""
    l = rng.standard_normal(V).astype(np.float32)
    if kind == 0:
        return l, int(np.argmax(l))
    if kind == 1:
        return l, 0
    if kind == 2:
        return l, V - 1
    if kind == 3:
        return l, -1
    if kind == 4:  # peaked: every other term underflows against the peak
        p = int(rng.integers(V))
        l[p] += np.float32(1e4)
        return l, p if flip else int(rng.integers(V))
    if kind == 5:  # a naive exp overflows
        return (l + np.float32(3e4)).astype(np.float32), int(rng.integers(V))
    if kind == 6:  # -inf entries, the target one of them on every other such row
        dead = rng.random(V) < 0.25
        dead[int(rng.integers(V))] = False
        l[dead] = -np.inf
        t = int(np.flatnonzero(dead)[len(np.flatnonzero(dead)) // 2]) if (flip and dead.any()) else int(rng.integers(V))
        return l, t
    # ties: the target's value on 4 ids, lower and higher than it, under a maximum held by 2 ids
    if V < 8:
        l[:] = np.float32(0.5)  # everything ties; two ids share the maximum when there is room
        if V >= 3:
            l[1] = l[V - 1] = np.float32(2.0)
        return l, V // 2
    tied = sorted({1, V // 3, V // 2, V - 2})
    l[tied] = np.float32(0.25)
    l[[V // 4, V - 1]] = np.float32(7.0)
    return l, tied[1] if flip else tied[2]


def make_case(V, R, salt):
    rng = np.random.default_rng(1000 * V + 10 * R + salt)
    rows, targets = [], []
    for r in range(R):
        l, t = make_row((3 * r + salt) % KINDS, V, rng, ((r // KINDS) + salt) % 2 == 0)
        rows.append(l)
        targets.append(t)
    return np.stack(rows), targets


def launch(E, logits, targets, pad, max_grid=0):
    """one launch over logits [R][V] copied into rows of V + pad floats, the padding +inf / NaN; one spare
    output row keeps its sentinels"""
    R, V = logits.shape
    buf = np.empty((R, V + pad), np.float32)
    buf[:, :V] = logits
    buf[:, V:] = np.where(np.arange(pad) % 2 == 0, np.inf, np.nan).astype(np.float32)
    d = dict(l=torch.from_numpy(buf).cuda(), t=torch.tensor(targets, dtype=torch.int32, device="cuda"),
             f=torch.full((R + 1, 2), SENT_F, dtype=torch.float32, device="cuda"),
             i=torch.full((R + 1, 2), SENT_I, dtype=torch.int32, device="cuda"))
    E.score_rows(d["l"].data_ptr(), V + pad, R, V, d["t"].data_ptr(), d["f"].data_ptr(), d["i"].data_ptr(), stream(),
                 max_grid)
    torch.cuda.synchronize()
    return d["f"].cpu().numpy(), d["i"].cpu().numpy()


def compare(name, logits, targets, ref, f, i):
    R = logits.shape[0]
    lp, rank, best, best_lp = ref
    assert np.all(f[R] == SENT_F) and np.all(i[R] == SENT_I), f"{name}: a row past R was written"
    assert np.array_equal(i[:R, 0], rank), f"{name}: rank {i[:R, 0].tolist()} want {rank.tolist()}"
    assert np.array_equal(i[:R, 1], best), f"{name}: best {i[:R, 1].tolist()} want {best.tolist()}"
    worst = 0.0  # the largest error relative to the row's tolerance, and in absolute terms
    worst_abs = 0.0
    for r in range(R):
        fin = logits[r][np.isfinite(logits[r])]
        tol = TOL * max(1.0, float(np.max(np.abs(fin))) / 32.0)
        for got, want, what in ((f[r, 0], lp[r], "lp"), (f[r, 1], best_lp[r], "best_lp")):
            if np.isnan(want):
                assert targets[r] < 0 and np.isnan(got), f"{name}: row {r} {what} {got} want NaN"
            elif np.isneginf(want):
                assert np.isneginf(got), f"{name}: row {r} {what} {got} want -inf"
            else:
                assert np.isfinite(got), f"{name}: row {r} {what} {got} want {want}"
                err = abs(float(got) - want)
                worst, worst_abs = max(worst, err / tol), max(worst_abs, err)
                assert err <= tol, f"{name}: row {r} {what} error {err:.3e} above {tol:.2e}"
    print(f"score_rows {name}: max |gpu - oracle| = {worst_abs:.3e} ({worst:.2f} of the row's tolerance)")


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("V", VS)
def test_against_the_oracle(E, V, R):
    logits, targets = make_case(V, R, VS.index(V) + 5 * RS.index(R))
    ref = O.score_rows(logits, targets)  # once per (V, R): the three strides score the same rows
    for pad in PADS:
        f, i = launch(E, logits, targets, pad)
        compare(f"V={V} R={R} ldl=V+{pad}", logits, targets, ref, f, i)


@pytest.mark.parametrize("V", [257, 4099])
def test_every_kind_with_few_rows(E, V):
    # every row kind, both variants, in launches of 1 and 3 rows (R = 70 above covers them in one launch)
    for salt in range(2 * KINDS):
        for R in (1, 3):
            logits, targets = make_case(V, R, salt)
            f, i = launch(E, logits, targets, 1)
            compare(f"V={V} R={R} salt={salt}", logits, targets, O.score_rows(logits, targets), f, i)


def test_grid_stride_matches_one_workgroup_per_row(E):
    logits, targets = make_case(4099, 70, 3)
    f0, i0 = launch(E, logits, targets, 13)
    for grid in (1, 16, 69):
        f, i = launch(E, logits, targets, 13, max_grid=grid)
        assert f.tobytes() == f0.tobytes() and i.tobytes() == i0.tobytes(), f"max_grid={grid}"
    compare("V=4099 R=70 grid=16", logits, targets, O.score_rows(logits, targets), f0, i0)


def test_same_launch_twice_gives_identical_bytes(E):
    logits, targets = make_case(32000, 70, 1)
    f0, i0 = launch(E, logits, targets, 1)
    f1, i1 = launch(E, logits, targets, 1)
    assert f0.tobytes() == f1.tobytes() and i0.tobytes() == i1.tobytes()


def test_launcher_refuses_bad_arguments(E):
    l = torch.zeros(4, 8, device="cuda")
    t = torch.zeros(4, dtype=torch.int32, device="cuda")
    f = torch.zeros(4, 2, device="cuda")
    i = torch.zeros(4, 2, dtype=torch.int32, device="cuda")
    for ldl, R, V in ((7, 4, 8), (8, 0, 8), (8, 4, 0)):
        with pytest.raises(RuntimeError):
            E.score_rows(l.data_ptr(), ldl, R, V, t.data_ptr(), f.data_ptr(), i.data_ptr(), stream())
    with pytest.raises(RuntimeError):
        E.score_rows(0, 8, 4, 8, t.data_ptr(), f.data_ptr(), i.data_ptr(), stream())
