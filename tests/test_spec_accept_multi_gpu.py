"""The segmented accept kernel (spec_accept_multi_kernel in csrc/kernels/spec_accept.hip) through the raw op
`_engine.spec_accept_multi`, against the rule in plain Python (tests/spec_multi_oracle.py).  Everything is
integer: every comparison is exact.

Layouts: S = 1, 2, 3, 4, 8 sequences, segments of 1, 2, 5 and 8 rows mixed, Rt = 2, 8, 9 and 32.  Per layout and
per segment: every accepted count 0..d_s (the other segments' counts drawn at random), with and without a
re-match behind the first mismatch, with out aliasing the state's token array (the engine's call) and apart from
it.  Checked per launch: the S records and nothing behind them, rows 0..S-1 of {token, pos, seq_len}, the poison
in rows S.. of the state, row s's history entries pos0[s] + 1 .. pos0[s] + n_s + 1 and nothing else in the
history (a sentinel everywhere else, the row behind the last sequence's included).  A sequence whose positions
reach the history stride writes only the entries below it.  S = 1 leaves what the single-sequence kernel leaves.
"""
import numpy as np
import pytest
import torch

import spec_multi_oracle as M
import spec_oracle as O

pytestmark = pytest.mark.gpu

V = 1000
STRIDE = 64    # history stride (max_ctx + 1 of a 63-token context)
SENT = -77
ROWS = M.SPEC_MULTI_MAX_ROWS + 2   # state rows allocated: two more than any step has

LAYOUTS = [(2,), (5,), (8,), (1, 1), (8, 1), (1, 8), (2, 5, 2), (5, 1, 2), (8, 8, 8, 8), (1,) * 8,
           (8, 8, 5, 5, 2, 2, 1, 1), (1, 2, 5, 8, 8, 5, 2, 1)]


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.tensor(np.asarray(a, np.int32), dtype=torch.int32, device="cuda")


def segment(R, n, rematch, rng):
    """(inp, out) of one segment of R rows whose first mismatch is at draft n (n == R - 1: none)"""
    out = rng.integers(0, V, R).astype(np.int32)
    inp = np.empty(R, np.int32)
    inp[0] = rng.integers(0, V)
    inp[1:] = out[:-1]
    if n < R - 1:
        inp[n + 1] = (out[n] + 1) % V
        if not rematch:
            for i in range(n + 2, R):
                inp[i] = (out[i - 1] + 1 + i) % V
    return inp, out


def step(lens, ns, rematch, rng):
    parts = [segment(R, n, rematch, rng) for R, n in zip(lens, ns)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def launch(E, inp, out, seg, pos0, alias):
    Rt, S = len(inp), len(pos0)
    tokens = dev(np.full(ROWS, SENT))
    if alias:
        tokens[:Rt] = dev(out)
    pos = dev(np.arange(ROWS) + 5000)        # poison that tells the rows apart
    seq_len = dev(np.arange(ROWS) + 7000)
    hist = dev(np.full((M.SPEC_MULTI_MAX_SEQS + 1) * STRIDE, SENT))
    rec = dev(np.full(M.SPEC_MULTI_MAX_SEQS * M.SPEC_RECORD + 2, SENT))
    d_in = dev(inp)
    d_out = tokens if alias else dev(out)
    E.spec_accept_multi(d_in.data_ptr(), d_out.data_ptr(), list(seg), list(pos0), rec.data_ptr(), tokens.data_ptr(),
                        pos.data_ptr(), seq_len.data_ptr(), hist.data_ptr(), STRIDE, stream())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (rec, tokens, pos, seq_len, hist)]


def check(got, inp, out, seg, pos0, alias):
    rec, tokens, pos, seq_len, hist = got
    Rt, S = len(inp), len(pos0)
    want = M.state_after(inp, out, seg, pos0)
    assert rec[:S * M.SPEC_RECORD].tolist() == M.records(inp, out, seg)
    assert np.all(rec[S * M.SPEC_RECORD:] == SENT)                   # nothing behind the S records
    for s, w in enumerate(want):
        assert (tokens[s], pos[s], seq_len[s]) == (w["token"], w["pos"], w["seq_len"]), s
    if alias:
        assert tokens[S:Rt].tolist() == list(out[S:])                # rows S.. left as the sampler wrote them
        assert np.all(tokens[Rt:] == SENT)
    else:
        assert np.all(tokens[S:] == SENT)
    assert pos[S:].tolist() == (np.arange(S, ROWS) + 5000).tolist()
    assert seq_len[S:].tolist() == (np.arange(S, ROWS) + 7000).tolist()
    exp = np.full((M.SPEC_MULTI_MAX_SEQS + 1) * STRIDE, SENT, np.int32)
    for s, w in enumerate(want):
        for k, t in w["history"].items():
            if k < STRIDE:                                           # entries at or past the stride: never written
                exp[s * STRIDE + k] = t
    assert hist.tolist() == exp.tolist()


@pytest.mark.parametrize("alias", [True, False])
@pytest.mark.parametrize("lens", LAYOUTS, ids=lambda l: "x".join(map(str, l)))
def test_every_mismatch_position_per_segment(E, lens, alias):
    rng = np.random.default_rng(1000 + 31 * len(lens) + sum(lens))
    seg = M.segments(lens)
    for s, R in enumerate(lens):
        for n in range(R):
            for rematch in ([False, True] if n < R - 2 else [False]):
                ns = [int(rng.integers(0, r)) for r in lens]
                ns[s] = n
                inp, out = step(lens, ns, rematch, rng)
                assert [a for a, _ in M.accept(inp, out, seg)] == ns
                pos0 = [int(rng.integers(0, STRIDE - 1 - r)) for r in lens]
                check(launch(E, inp, out, seg, pos0, alias), inp, out, seg, pos0, alias)


def test_chained_rows_across_boundaries_do_not_count(E):
    """out[r] == in[r + 1] on EVERY row, the rows at segment boundaries included: each segment accepts its own
    drafts and nothing more"""
    lens = (2, 5, 1, 8)
    seg = M.segments(lens)
    out = np.arange(100, 100 + 16, dtype=np.int32)
    inp = np.concatenate([[99], out[:-1]]).astype(np.int32)
    assert [a for a, _ in M.accept(inp, out, seg)] == [1, 4, 0, 7]
    pos0 = [3, 40, 0, 20]
    check(launch(E, inp, out, seg, pos0, True), inp, out, seg, pos0, True)


def test_history_stops_at_the_stride(E):
    """a sequence whose entries would pass hist_stride writes only those below it: the next row's first entries
    (what an unclipped store would hit) keep their sentinel.  The other sequence ends exactly on the last entry."""
    lens = (8, 8, 1)
    seg = M.segments(lens)
    rng = np.random.default_rng(9)
    inp, out = step(lens, [7, 7, 0], False, rng)
    pos0 = [STRIDE - 4, STRIDE - 1 - 8, STRIDE - 1]    # entries up to STRIDE + 4 | up to STRIDE - 1 | STRIDE
    for alias in (True, False):
        check(launch(E, inp, out, seg, pos0, alias), inp, out, seg, pos0, alias)


@pytest.mark.parametrize("R", [2, 5, 8])
def test_one_sequence_equals_the_single_sequence_kernel(E, R):
    rng = np.random.default_rng(70 + R)
    for n in range(R):
        inp, out = segment(R, n, n < R - 2, rng)
        pos0 = int(rng.integers(0, STRIDE - 1 - R))
        rec, tokens, pos, seq_len, hist = launch(E, inp, out, [0, R], [pos0], True)
        t1 = dev(np.concatenate([out, np.full(ROWS - R, SENT)]))
        p1, l1 = dev(np.arange(ROWS) + 5000), dev(np.arange(ROWS) + 7000)
        h1 = dev(np.full((M.SPEC_MULTI_MAX_SEQS + 1) * STRIDE, SENT))
        r1 = dev(np.full(O.SPEC_RECORD, SENT))
        d_in = dev(inp)
        E.spec_accept(d_in.data_ptr(), t1.data_ptr(), pos0, R, r1.data_ptr(), t1.data_ptr(), p1.data_ptr(), l1.data_ptr(),
                      h1.data_ptr(), STRIDE, stream())
        torch.cuda.synchronize()
        assert rec[:O.SPEC_RECORD].tolist() == r1.cpu().tolist()
        assert tokens.tolist() == t1.cpu().tolist() and pos.tolist() == p1.cpu().tolist()
        assert seq_len.tolist() == l1.cpu().tolist() and hist.tolist() == h1.cpu().tolist()


def test_bad_layouts_throw(E):
    z = dev([0] * ROWS)
    bad = [([0], []), ([0, 9], [0]), ([0, 0], [0]), ([1, 2], [0]), ([0, 2, 1], [0, 0]), (list(range(10)), [0] * 9),
           ([0, 8, 16, 24, 32, 33], [0] * 5), ([0, 2], [-1]), ([0, 2], [0, 0])]
    for seg, pos0 in bad:
        with pytest.raises(RuntimeError):
            E.spec_accept_multi(z.data_ptr(), z.data_ptr(), seg, pos0, dev([0] * 72).data_ptr(), z.data_ptr(), z.data_ptr(),
                                z.data_ptr(), 0, 0, stream())
