"""The device logprob kernel (logprob_kernel in csrc/kernels/logprobs.hip) through the raw op
`_engine.logprobs`, against the float64 oracle of its rule (tests/logprob_oracle.py): ids exact, values
within TOL.  Shapes are the smallest at which each path can go wrong: fewer tokens than top_n, one slice, a
second slice of one token, a ragged last slice, the served vocabularies and the cap; rows padded to
ldl = V + 37 with the padding poisoned, so an over-read shows in lse or in the ids.

TOL is logprob_oracle.GPU_TOL (measured; see there).
"""
import numpy as np
import pytest
import torch

import logprob_oracle as O

pytestmark = pytest.mark.gpu

TOL = O.GPU_TOL
ROW = O.MAX_TOP + 1
PAD = 37
SENT_LP, SENT_ID = 123.0, -7


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def launch(E, logits, tokens, top_n, poison=1e30):
    """enqueue one launch over logits [B][V] copied into rows of V + PAD floats, the padding poisoned;
    returns the device tensors (outputs pre-filled with the sentinels); no synchronisation"""
    logits = np.asarray(logits, np.float32)
    B, V = logits.shape
    buf = np.full((B, V + PAD), poison, np.float32)
    buf[:, :V] = logits
    d = dict(l=torch.from_numpy(buf).cuda(), t=torch.tensor(tokens, dtype=torch.int32, device="cuda"),
             n=torch.tensor(top_n, dtype=torch.int32, device="cuda"),
             lp=torch.full((B, ROW), SENT_LP, dtype=torch.float32, device="cuda"),
             id=torch.full((B, ROW), SENT_ID, dtype=torch.int32, device="cuda"))
    E.logprobs(d["l"].data_ptr(), V + PAD, B, V, d["t"].data_ptr(), d["n"].data_ptr(), d["lp"].data_ptr(),
               d["id"].data_ptr(), stream())
    return d


def compare(name, logits, tokens, top_n, d):
    """device outputs of `launch` against the oracle, row by row; prints the largest value error"""
    lp, ids = d["lp"].cpu().numpy().astype(np.float64), d["id"].cpu().numpy()
    worst = 0.0
    for b, (tok, n) in enumerate(zip(tokens, top_n)):
        if n < 0:  # row off: nothing written
            assert np.all(lp[b] == SENT_LP) and np.all(ids[b] == SENT_ID), f"{name}: off row {b} was written"
            continue
        olp, oid = O.padded(logits[b], tok, n)
        assert np.array_equal(ids[b], oid), f"{name}: row {b} ids {ids[b].tolist()} want {oid.tolist()}"
        inf = np.isneginf(olp)
        assert np.array_equal(np.isneginf(lp[b]), inf), f"{name}: row {b} -inf entries {lp[b].tolist()}"
        assert np.all(np.isfinite(lp[b][~inf])), f"{name}: row {b} values {lp[b].tolist()}"
        worst = max(worst, float(np.max(np.abs(lp[b][~inf] - olp[~inf]), initial=0.0)))
    print(f"logprobs {name}: max |gpu - oracle| = {worst:.3e}")
    assert worst <= TOL, f"{name}: value error {worst:.3e} above {TOL:.1e}"


def check(E, name, logits, tokens, top_n, poisons=(1e30, float("nan"))):
    logits = np.asarray(logits, np.float32)
    for p in poisons:
        d = launch(E, logits, tokens, top_n, p)
        torch.cuda.synchronize()
        compare(f"{name} pad={p}", logits, tokens, top_n, d)


def dense(V, B, sd, seed):
    return (np.random.default_rng(seed).standard_normal((B, V)) * sd).astype(np.float32)


def spread_tokens(logits):
    """sampled tokens at the row's argmax, argmin and last id, in turn"""
    V = logits.shape[1]
    pick = [lambda r: int(np.argmax(r)), lambda r: int(np.argmin(r)), lambda r: V - 1]
    return [pick[b % 3](r) for b, r in enumerate(logits)]


@pytest.mark.parametrize("V", [5, 20, 21, 4096, 4097, 8191, 32000, 151936, 262144])
def test_vocabulary_sizes(E, V):
    l = dense(V, 3, 2.0, V)
    check(E, f"V={V}", l, spread_tokens(l), [20, 20, 20])


def test_vocabulary_above_the_cap_throws(E):
    V = 262145
    with pytest.raises(RuntimeError):
        launch(E, np.zeros((1, V), np.float32), [0], [20])
    torch.cuda.synchronize()


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V", [4097, 32000])
def test_batch(E, B, V):
    l = dense(V, B, 2.0, 100 * B + V)
    check(E, f"B={B} V={V}", l, spread_tokens(l), [20] * B)


@pytest.mark.parametrize("V", [20, 4097, 8191, 151936])
def test_spikes(E, V):
    # four logits at 0 over a background of -20 (at most V e^-20 = 5e-4 of the mass): losing one spike moves
    # lse by log(4/3); the alternatives behind the spikes are background ties, lowest ids first
    spikes = sorted({min(i, V - 1) for i in (0, 4095, 4096, V - 1)})
    l = np.full((len(spikes), V), -20.0, np.float32)
    l[:, spikes] = 0.0
    check(E, f"spikes V={V}", l, spikes, [20] * len(spikes))


@pytest.mark.parametrize("V", [8191, 151936])
def test_flat(E, V):
    l = np.full((2, V), 1.5, np.float32)
    d = launch(E, l, [0, V - 1], [20, 20])
    torch.cuda.synchronize()
    assert d["id"].cpu().numpy()[:, 1:].tolist() == [list(range(20))] * 2   # the tie rule across slices
    assert np.allclose(d["lp"].cpu().numpy(), -np.log(V), rtol=0, atol=TOL)  # lse = l + log V
    check(E, f"flat V={V}", l, [0, V - 1], [20, 20])


def test_ties_straddling_slices(E):
    V = 4 * 4096 + 5
    rng = np.random.default_rng(7)
    l = rng.standard_normal((2, V)).astype(np.float32)
    ids = np.concatenate([rng.choice(4096, 8, replace=False) + 4096 * s for s in range(3)] + [[V - 1, V - 2, V - 3],
                         [4095, 4096, 8191]])
    assert len(set(ids.tolist())) == 30
    l[:, ids] = 9.0
    d = launch(E, l, [int(ids[0]), 0], [20, 20])
    torch.cuda.synchronize()
    assert d["id"].cpu().numpy()[0, 1:].tolist() == sorted(ids.tolist())[:20]
    check(E, "ties", l, [int(ids[0]), 0], [20, 20])


@pytest.mark.parametrize("V,at", [(4097, 4096), (9000, 5000), (21, 20)])
def test_one_finite_logit(E, V, at):
    l = np.full((1, V), -np.inf, np.float32)
    l[0, at] = 3.25
    d = launch(E, l, [at], [20])
    torch.cuda.synchronize()
    lp, ids = d["lp"].cpu().numpy()[0], d["id"].cpu().numpy()[0]
    assert lp[0] == 0.0 and lp[1] == 0.0 and ids[1] == at
    assert ids[2:].tolist() == list(range(19)) and np.all(np.isneginf(lp[2:]))
    check(E, f"one finite V={V}", l, [at], [20])
    check(E, f"one finite V={V}, token at -inf", l, [0], [3])


@pytest.mark.parametrize("V", [32000, 151936])
@pytest.mark.parametrize("sd", [2.0, 0.1])
def test_dense_rows(E, V, sd):
    l = dense(V, 3, sd, int(V + 10 * sd))
    check(E, f"dense N(0, {sd}^2) V={V}", l, spread_tokens(l), [20, 20, 20])


def test_mixed_top_n_and_off_rows(E):
    V = 4097
    l = dense(V, 4, 2.0, 11)
    check(E, "mixed top_n", l, [1, 2, 4096, 7], [-1, 0, 1, 20])
    check(E, "all off", l, [1, 2, 4096, 7], [-1, -1, -1, -1], poisons=(1e30,))


def test_rearming(E):
    # two launches back to back on the same counters and workspace, different logits: the second is its own
    V, B = 8191, 3
    l1, l2 = dense(V, B, 2.0, 21), dense(V, B, 2.0, 22)
    t1, t2 = spread_tokens(l1), spread_tokens(l2)
    d1 = launch(E, l1, t1, [20] * B)
    d2 = launch(E, l2, t2, [5] * B)
    torch.cuda.synchronize()
    compare("re-arm first", l1, t1, [20] * B, d1)
    compare("re-arm second", l2, t2, [5] * B, d2)
