"""The segmented accept rule (tests/spec_multi_oracle.py) against the single-sequence oracle applied segment by
segment and against the rule as the issue states it, written out directly on the flat rows."""
import itertools

import numpy as np

import spec_multi_oracle as M
import spec_oracle as O


def compositions(n):
    """every way to cut n rows into segments of 1..SPEC_MAX_ROWS rows, at most SPEC_MULTI_MAX_SEQS of them"""
    for cuts in itertools.product([0, 1], repeat=n - 1):
        lens, run = [], 1
        for c in cuts:
            if c:
                lens.append(run)
                run = 1
            else:
                run += 1
        lens.append(run)
        if len(lens) <= M.SPEC_MULTI_MAX_SEQS and max(lens) <= M.SPEC_MAX_ROWS:
            yield lens


def direct(inp, out, seg):
    """n_s = the largest k <= d_s with out[seg[s] + i] == in[seg[s] + i + 1] for all i < k"""
    res = []
    for s in range(len(seg) - 1):
        b, d = seg[s], seg[s + 1] - seg[s] - 1
        n = max(k for k in range(d + 1) if all(out[b + i] == inp[b + i + 1] for i in range(k)))
        res.append((n, [int(t) for t in out[b:b + n + 1]]))
    return res


def test_every_segmentation_up_to_12_rows():
    rng = np.random.default_rng(3)
    count = 0
    for n in range(1, 13):
        for lens in compositions(n):
            seg = M.segments(lens)
            # a vocabulary of 3: matches, mismatches and re-matches behind a mismatch all occur often
            inp, out = rng.integers(0, 3, n).tolist(), rng.integers(0, 3, n).tolist()
            got = M.accept(inp, out, seg)
            assert got == direct(inp, out, seg)
            for (b, e), g in zip(zip(seg[:-1], seg[1:]), got):
                if e - b >= 2:
                    assert g == O.accept(inp[b:e], out[b:e])
                else:
                    assert g == (0, [out[b]])
            count += 1
    assert count > 3000


def test_one_row_segments_emit_one_token():
    inp, out = [5, 6, 7], [6, 7, 9]   # flat, the rows would chain: as segments of one row nothing is a draft
    assert M.accept(inp, out, [0, 1, 2, 3]) == [(0, [6]), (0, [7]), (0, [9])]
    assert M.records(inp, out, [0, 1, 2, 3]) == sum(([0, t] + [-1] * 7 for t in out), [])


def test_a_match_across_a_boundary_or_behind_a_mismatch_does_not_count():
    #        seq 0: 10 | 11 12     seq 1: 12 | 13 99 15
    inp = [10, 11, 12, 12, 13, 99, 15]
    out = [11, 12, 12, 13, 14, 15, 16]
    # seq 0: both drafts right, and out[2] == inp[3] across the boundary counts for nothing (n stays 2)
    # seq 1: draft 13 right, 99 wrong (the sampler said 14), 15 right again behind it: n = 1
    assert M.accept(inp, out, [0, 3, 7]) == [(2, [11, 12, 12]), (1, [13, 14])]
    assert M.records(inp, out, [0, 3, 7]) == [2, 11, 12, 12, -1, -1, -1, -1, -1, 1, 13, 14, -1, -1, -1, -1, -1, -1]


def test_state_rows():
    inp = [10, 11, 12, 12, 13, 99, 15, 40]
    out = [11, 12, 12, 13, 14, 15, 16, 41]
    rows = M.state_after(inp, out, [0, 3, 7, 8], [20, 100, 7])
    assert rows[0] == dict(token=12, pos=23, seq_len=24, history={21: 11, 22: 12, 23: 12})
    assert rows[1] == dict(token=14, pos=102, seq_len=103, history={101: 13, 102: 14})
    assert rows[2] == dict(token=41, pos=8, seq_len=9, history={8: 41})
    # one sequence of R rows: the single-sequence oracle's row 0
    assert M.state_after(inp[3:7], out[3:7], [0, 4], [100])[0] == O.state_after(inp[3:7], out[3:7], 100)
    assert M.records(inp[3:7], out[3:7], [0, 4]) == O.record(inp[3:7], out[3:7])
