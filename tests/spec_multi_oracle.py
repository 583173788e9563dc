"""The segmented accept rule of a multi-sequence speculative step in plain Python (csrc/ops.h
SpecAcceptMultiArgs), built on the single-sequence rule (tests/spec_oracle.py).

One step carries S sequences, segment after segment: rows seg[s] .. seg[s + 1] - 1 are sequence s's last
accepted token and its d_s >= 0 drafts, at positions pos0[s] .. pos0[s] + d_s.  Each segment is judged alone by
spec_oracle.accept; a one-row segment (no draft) accepts nothing and emits its one token -- spec_oracle.accept
asks for two rows, so that case is spelled out here.
"""
from typing import List, Sequence, Tuple

import spec_oracle as O

SPEC_MAX_ROWS = O.SPEC_MAX_ROWS
SPEC_RECORD = O.SPEC_RECORD
SPEC_MULTI_MAX_SEQS = 8
SPEC_MULTI_MAX_ROWS = 32


def segments(lengths: Sequence[int]) -> List[int]:
    """row offsets seg[0..S] of segments with these row counts"""
    seg = [0]
    for n in lengths:
        assert 1 <= n <= SPEC_MAX_ROWS
        seg.append(seg[-1] + int(n))
    assert 1 <= len(lengths) <= SPEC_MULTI_MAX_SEQS and seg[-1] <= SPEC_MULTI_MAX_ROWS
    return seg


def accept(inp: Sequence[int], out: Sequence[int], seg: Sequence[int]) -> List[Tuple[int, List[int]]]:
    """(n_s, emitted tokens) per sequence"""
    assert seg[0] == 0 and seg[-1] == len(inp) == len(out)
    res = []
    for b, e in zip(seg[:-1], seg[1:]):
        if e - b == 1:
            res.append((0, [int(out[b])]))
        else:
            res.append(O.accept(inp[b:e], out[b:e]))
    return res


def records(inp, out, seg) -> List[int]:
    """the S packed records, flat: {n_s, out[seg[s] .. seg[s] + n_s], -1 padding} each"""
    flat = []
    for n, toks in accept(inp, out, seg):
        flat += [n] + toks + [-1] * (SPEC_RECORD - 1 - len(toks))
    return flat


def state_after(inp, out, seg, pos0: Sequence[int]) -> List[dict]:
    """rows 0..S-1 of the step state and row s's history entries {index: token} after the accept step"""
    rows = []
    for (n, toks), p in zip(accept(inp, out, seg), pos0):
        rows.append(dict(token=toks[n], pos=p + n + 1, seq_len=p + n + 2,
                         history={p + 1 + i: toks[i] for i in range(n + 1)}))
    return rows
