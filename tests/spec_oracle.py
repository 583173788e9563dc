"""Speculative decoding's two rules in plain Python (csrc/ops.h SpecAcceptArgs, runtime/speculative.py).

accept: a request ran R consecutive positions as the R rows of one step.  inp[0] is its last accepted token,
inp[1:] the draft; out[i] is what the sampler drew after inp[0..i].  Row i saw the right context only if every
draft before it was right, so the accepted count is the length of the agreeing PREFIX -- a match behind the
first mismatch does not count -- and the request emits out[0..n].

lookup_draft: prompt lookup by a naive scan.  For n from ngram_max down to ngram_min, the trailing n-gram of
the context is looked for first in the prediction, then in the context itself; in either, the most recent
occurrence that has at least one token after it wins, and the draft is the up to draft_max tokens behind it.
"""
from typing import List, Optional, Sequence, Tuple

SPEC_MAX_ROWS = 8
SPEC_RECORD = SPEC_MAX_ROWS + 1


def accept(inp: Sequence[int], out: Sequence[int]) -> Tuple[int, List[int]]:
    R = len(inp)
    assert 2 <= R <= SPEC_MAX_ROWS and len(out) == R
    n = 0
    while n < R - 1 and out[n] == inp[n + 1]:
        n += 1
    return n, [int(t) for t in out[:n + 1]]


def record(inp, out) -> List[int]:
    """the packed record the kernel leaves for the host: {n, out[0..n], -1 padding}"""
    n, toks = accept(inp, out)
    return [n] + toks + [-1] * (SPEC_RECORD - 1 - len(toks))


def state_after(inp, out, pos0: int) -> dict:
    """row 0 of the step state and the history entries {index: token} after the accept step"""
    n, toks = accept(inp, out)
    return dict(token=toks[n], pos=pos0 + n + 1, seq_len=pos0 + n + 2,
                history={pos0 + 1 + i: toks[i] for i in range(n + 1)})


def _last_with_follower(seq: Sequence[int], tail: Sequence[int]) -> Optional[int]:
    n = len(tail)
    for j in range(len(seq) - n - 1, -1, -1):  # j + n <= len(seq) - 1: a token follows
        if list(seq[j:j + n]) == list(tail):
            return j
    return None


def lookup_draft(context: Sequence[int], prediction: Sequence[int] = (), ngram_min: int = 2, ngram_max: int = 3,
                 draft_max: int = 4) -> List[int]:
    for n in range(ngram_max, ngram_min - 1, -1):
        if len(context) < n:
            continue
        tail = list(context[-n:])
        for src in (prediction, context):
            j = _last_with_follower(src, tail)
            if j is not None:
                return [int(t) for t in src[j + n:j + n + draft_max]]
    return []
