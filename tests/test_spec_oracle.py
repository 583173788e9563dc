"""The two rules of speculative decoding on the host: the accept rule (tests/spec_oracle.py: accept, the
kernel's and the stub engines' reference) on hand cases, and the incremental prompt-lookup drafter
(runtime/speculative.py) against the naive scan (spec_oracle.lookup_draft)."""
import numpy as np
import pytest

import spec_oracle as O
from aios_amd.runtime.speculative import DRAFT_MAX_LIMIT, LookupDrafter


def test_accept_hand_cases():
    assert O.accept([5, 6, 7, 8], [6, 7, 8, 9]) == (3, [6, 7, 8, 9])          # every draft right: R tokens
    assert O.accept([5, 6, 7, 8], [1, 7, 8, 9]) == (0, [1])                    # the first wrong: the plain step
    assert O.accept([5, 6, 7, 8], [6, 2, 8, 9]) == (1, [6, 2])                 # a match behind the mismatch does not count
    assert O.accept([5, 6, 7, 8], [6, 7, 3, 9]) == (2, [6, 7, 3])
    assert O.accept([5, 6], [6, 0]) == (1, [6, 0])
    assert O.record([5, 6, 7, 8], [6, 2, 8, 9]) == [1, 6, 2, -1, -1, -1, -1, -1, -1]
    assert len(O.record([1] * 8, [1] * 8)) == O.SPEC_RECORD and O.record([1] * 8, [1] * 8) == [7] + [1] * 8
    st = O.state_after([5, 6, 7, 8], [6, 7, 3, 9], 10)
    assert st == dict(token=3, pos=13, seq_len=14, history={11: 6, 12: 7, 13: 3})


def test_lookup_hand_cases():
    # the most recent occurrence wins: "1 2" is followed by 3 first, by 9 later
    assert O.lookup_draft([1, 2, 3, 4, 1, 2, 9, 8, 1, 2], ngram_min=2, ngram_max=2) == [9, 8, 1, 2]
    # a longer n-gram is tried first, although a shorter one has a more recent match
    assert O.lookup_draft([7, 1, 2, 3, 5, 1, 2, 6, 7, 1, 2], ngram_min=2, ngram_max=3, draft_max=2) == [3, 5]
    # overlapping n-grams: the occurrence may overlap the tail itself, and the draft may run into it
    assert O.lookup_draft([4, 4, 4, 4], ngram_min=2, ngram_max=3, draft_max=4) == [4]
    assert O.lookup_draft([1, 2, 1, 2, 1, 2], ngram_min=2, ngram_max=2, draft_max=7) == [1, 2]
    # a match at the very end has nothing behind it: no draft
    assert O.lookup_draft([1, 2, 3, 4, 5, 6], ngram_min=2, ngram_max=3) == []
    assert O.lookup_draft([3, 9], ngram_min=2, ngram_max=3) == []
    # the prediction is searched first, at the same n; the context serves an n the prediction cannot
    ctx = [1, 2, 3, 4, 1, 2]
    assert O.lookup_draft(ctx, prediction=[0, 1, 2, 7, 7, 7], ngram_min=2, ngram_max=2) == [7, 7, 7]
    assert O.lookup_draft(ctx, prediction=[0, 1, 2], ngram_min=2, ngram_max=2) == [3, 4, 1, 2]   # nothing behind it there
    assert O.lookup_draft([9, 4, 1, 2, 5, 5, 4, 1, 2], prediction=[1, 2, 7], ngram_min=2, ngram_max=3, draft_max=1) == [5]
    for case, kw in (([1, 2, 3, 4, 1, 2, 9, 8, 1, 2], dict(ngram_min=2, ngram_max=2)), ([4, 4, 4, 4], {}),
                     ([1, 2, 3, 4, 5, 6], {}), ([7, 1, 2, 3, 5, 1, 2, 6, 7, 1, 2], dict(draft_max=2))):
        assert LookupDrafter(case, **kw).draft() == O.lookup_draft(case, **kw)


def test_incremental_index_equals_the_naive_scan():
    rng = np.random.default_rng(2024)
    drafted = 0
    for trial in range(200):
        n = int(rng.integers(1, 60))
        stream = [int(t) for t in rng.integers(0, 6, n)]
        pred = [int(t) for t in rng.integers(0, 6, int(rng.integers(0, 12)))] if trial % 3 == 0 else []
        kw = dict(ngram_min=int(rng.integers(1, 3)), ngram_max=int(rng.integers(2, 5)), draft_max=int(rng.integers(1, 8)))
        cut = int(rng.integers(0, n))
        d = LookupDrafter(stream[:cut], pred, **kw)   # a prompt, then one token at a time
        for i in range(cut, n + 1):
            want = O.lookup_draft(stream[:i], pred, **kw)
            assert d.draft() == want, (trial, i)
            assert d.draft(2) == want[:2] and d.draft(0) == []
            drafted += bool(want)
            if i < n:
                hint = d.may_draft_after_next()
                d.append(stream[i])
                # the hint is a necessary condition: whatever drafts after the next token was announced
                assert hint or not O.lookup_draft(stream[:i + 1], pred, **kw), (trial, i)
    assert drafted > 1000   # (the alphabet is small enough that most positions draft)


def test_hint_says_no_where_nothing_can_follow():
    """text that never repeats announces no draft, whatever comes next; a repeat announces one"""
    d = LookupDrafter([], ngram_min=2, ngram_max=3)
    for t in range(30):
        assert not d.may_draft_after_next() and d.draft() == []
        d.append(t)
    d.append(5)                                   # 5 was followed by 6 before: a next token 6 would draft
    assert d.may_draft_after_next() and d.draft() == []
    d.append(6)
    assert d.draft() == [7, 8, 9, 10, 11, 12, 13]
    p = LookupDrafter([100, 101], prediction=[3, 101, 7, 8], ngram_min=2, ngram_max=2)
    assert p.may_draft_after_next()               # 101 has two tokens behind it in the prediction
    assert not LookupDrafter([100, 101], prediction=[3, 9, 101, 7], ngram_min=2, ngram_max=2).may_draft_after_next()
    assert LookupDrafter([4], ngram_min=1, ngram_max=1).may_draft_after_next()
    assert not LookupDrafter([], ngram_min=1, ngram_max=1).may_draft_after_next()


def test_drafter_refuses_bad_settings():
    for kw in (dict(ngram_min=0), dict(ngram_min=3, ngram_max=2), dict(draft_max=0), dict(draft_max=DRAFT_MAX_LIMIT + 1),
               dict(ngram_max=9)):
        with pytest.raises(ValueError):
            LookupDrafter([1, 2, 3], **kw)
