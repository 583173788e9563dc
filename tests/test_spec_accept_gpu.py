"""The accept kernel of speculative decoding (spec_accept_kernel in csrc/kernels/spec_accept.hip) through the
raw op `_engine.spec_accept`, against the rule in plain Python (tests/spec_oracle.py).  Everything is integer:
every comparison is exact.

Cases: R = 2..8; the accepted count n = 0, every middle value and R - 1; a draft that matches again behind its
first mismatch (the re-match does not count); out aliasing the state's token array (the engine's call) and
apart from it.  Checked per launch: the packed record {n, out[0..n], -1 ...}, row 0 of the step state
{token, pos, seq_len}, rows 1.. of the state untouched, row 0's history entries pos0 + 1 .. pos0 + n + 1 and
nothing else in the history (sentinels before, behind and in row 1).  Two launches back to back on one stream,
the second continuing from the state the first left.
"""
import numpy as np
import pytest
import torch

import spec_oracle as O

pytestmark = pytest.mark.gpu

V = 1000
STRIDE = 64   # history stride (max_ctx + 1 of a 63-token context)
SENT = -77


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.tensor(np.asarray(a, np.int32), dtype=torch.int32, device="cuda")


def case(R, n, rematch, rng):
    """(inp, out): R rows whose first mismatch is at draft n (n == R - 1: none)"""
    out = rng.integers(0, V, R).astype(np.int32)
    inp = np.empty(R, np.int32)
    inp[0] = rng.integers(0, V)
    inp[1:] = out[:-1]                       # every draft right ...
    if n < R - 1:
        inp[n + 1] = (out[n] + 1) % V        # ... but draft n
        if not rematch:                      # and the ones behind it wrong too
            for i in range(n + 2, R):
                inp[i] = (out[i - 1] + 1 + i) % V
    return inp, out


def launch(E, inp, out, pos0, alias, state=None):
    """one launch; returns the device tensors (record, tokens, pos, seq_len, history)"""
    R = len(inp)
    if state is None:
        tokens = dev(out if alias else np.full(O.SPEC_MAX_ROWS, SENT))
        pos = dev([pos0 + i + 1 for i in range(O.SPEC_MAX_ROWS)])     # as the sampler's advance left them
        seq_len = dev([pos0 + i + 2 for i in range(O.SPEC_MAX_ROWS)])
        hist = dev(np.full(2 * STRIDE, SENT))
    else:
        tokens, pos, seq_len, hist = state
        if alias:
            tokens[:R] = dev(out)
    rec = dev(np.full(O.SPEC_RECORD + 2, SENT))
    d_in = dev(inp)
    d_out = tokens if alias else dev(out)
    E.spec_accept(d_in.data_ptr(), d_out.data_ptr(), pos0, R, rec.data_ptr(), tokens.data_ptr(), pos.data_ptr(),
                  seq_len.data_ptr(), hist.data_ptr(), STRIDE, stream())
    return rec, tokens, pos, seq_len, hist, (d_in, d_out)


def check(got, inp, out, pos0, alias, hist_before=None):
    rec, tokens, pos, seq_len, hist = [t.cpu().numpy() for t in got[:5]]
    R = len(inp)
    want = O.state_after(inp, out, pos0)
    assert rec[:O.SPEC_RECORD].tolist() == O.record(inp, out)
    assert np.all(rec[O.SPEC_RECORD:] == SENT)                       # nothing behind the record
    assert (tokens[0], pos[0], seq_len[0]) == (want["token"], want["pos"], want["seq_len"])
    if alias:
        assert tokens[1:R].tolist() == list(out[1:])                  # rows 1.. left as the sampler wrote them
    else:
        assert np.all(tokens[1:] == SENT)
    assert pos[1:].tolist() == [pos0 + i + 1 for i in range(1, O.SPEC_MAX_ROWS)]
    assert seq_len[1:].tolist() == [pos0 + i + 2 for i in range(1, O.SPEC_MAX_ROWS)]
    exp = np.full(2 * STRIDE, SENT, np.int32) if hist_before is None else hist_before.copy()
    for k, t in want["history"].items():
        exp[k] = t
    assert hist.tolist() == exp.tolist()
    return exp


@pytest.mark.parametrize("alias", [True, False])
@pytest.mark.parametrize("R", list(range(2, O.SPEC_MAX_ROWS + 1)))
def test_every_accept_count(E, R, alias):
    rng = np.random.default_rng(100 + R)
    for n in range(R):
        for rematch in ([False, True] if n < R - 2 else [False]):
            inp, out = case(R, n, rematch, rng)
            assert O.accept(inp, out)[0] == n
            if rematch:
                assert all(out[i] == inp[i + 1] for i in range(n + 1, R - 1))  # (the case is what it says)
            pos0 = int(rng.integers(0, STRIDE - 1 - R))
            got = launch(E, inp, out, pos0, alias)
            torch.cuda.synchronize()
            check(got, inp, out, pos0, alias)


def test_history_edge(E):
    """pos0 + R == max_ctx: the last history entry is the row's last one (index max_ctx), row 1's first entry
    behind it stays"""
    rng = np.random.default_rng(7)
    R = 8
    inp, out = case(R, R - 1, False, rng)
    pos0 = STRIDE - 1 - R
    got = launch(E, inp, out, pos0, True)
    torch.cuda.synchronize()
    check(got, inp, out, pos0, True)


def test_bad_rows_throw(E):
    inp, out = case(2, 0, False, np.random.default_rng(1))
    for R in (1, 9, 0):
        with pytest.raises(RuntimeError):
            E.spec_accept(dev(inp).data_ptr(), dev(out).data_ptr(), 0, R, dev([0] * 9).data_ptr(), dev([0] * 8).data_ptr(),
                          dev([0] * 8).data_ptr(), dev([0] * 8).data_ptr(), 0, 0, stream())


def test_two_launches_back_to_back(E):
    """the second launch starts where the first one's row 0 ended, with no synchronisation between them"""
    rng = np.random.default_rng(55)
    inp1, out1 = case(5, 2, True, rng)
    inp2, out2 = case(8, 7, False, rng)
    pos0 = 3
    n1 = O.accept(inp1, out1)[0]
    pos1 = pos0 + n1 + 1
    keep = []
    got1 = launch(E, inp1, out1, pos0, False)
    keep.append(got1[5])
    rec1 = got1[0]
    got2 = launch(E, inp2, out2, pos1, False, state=got1[1:5])
    keep.append(got2[5])
    torch.cuda.synchronize()
    assert rec1.cpu().numpy()[:O.SPEC_RECORD].tolist() == O.record(inp1, out1)
    rec2, tokens, pos, seq_len, hist = [t.cpu().numpy() for t in got2[:5]]
    assert rec2[:O.SPEC_RECORD].tolist() == O.record(inp2, out2)
    w1, w2 = O.state_after(inp1, out1, pos0), O.state_after(inp2, out2, pos1)
    assert (tokens[0], pos[0], seq_len[0]) == (w2["token"], w2["pos"], w2["seq_len"])
    exp = np.full(2 * STRIDE, SENT, np.int32)
    for k, t in {**w1["history"], **w2["history"]}.items():
        exp[k] = t
    assert hist.tolist() == exp.tolist()
    assert sorted({**w1["history"], **w2["history"]}) == list(range(pos0 + 1, pos1 + 8 + 1))  # one unbroken run
