"""Drafts for speculative decoding by prompt lookup (no draft model).

Agent and JSON workloads repeat their prompt -- tool names, keys, paths from the catalogue -- so the tokens
that followed the last occurrence of the text's trailing n-gram are a cheap guess at what comes next
(llama.cpp's lookup decoding).  The engine verifies a draft in one step (Engine.spec_decode): every row is
sampled as usual and the longest agreeing prefix is kept, so a wrong draft costs time, never a token.

The rule (tests/spec_oracle.py: lookup_draft is the same rule as a naive scan): for n from ngram_max down to
ngram_min, take the trailing n-gram of the context (prompt + generated tokens) and look for it first in the
request's prediction (OpenAI's Predicted Outputs), then in the context itself; in either, the most recent
occurrence with at least one token after it wins, and the draft is the up to draft_max tokens behind it.

The index is incremental: one dict per n, n-gram -> the last start that has a follower, updated by each
appended token with the one n-gram that token gave a follower to.  O(1) per token, nothing is rescanned.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

DRAFT_MAX_LIMIT = 7  # the engine verifies at most 8 rows: the last token and 7 drafts
NGRAM_MAX_LIMIT = 8  # longest n-gram looked up (one dict per length)
MULTI_SEQS_MAX = 8   # sequences of one multi-sequence speculative step (Engine.spec_decode_multi) ...
MULTI_ROWS_MAX = 32  # ... and its rows, every sequence's last token and draft together


class LookupDrafter:
    def __init__(self, ids: Sequence[int], prediction: Optional[Sequence[int]] = None, ngram_min: int = 2,
                 ngram_max: int = 3, draft_max: int = 7):
        if not 1 <= ngram_min <= ngram_max <= NGRAM_MAX_LIMIT:
            raise ValueError(f"need 1 <= ngram_min <= ngram_max <= {NGRAM_MAX_LIMIT}")
        if not 1 <= draft_max <= DRAFT_MAX_LIMIT:
            raise ValueError(f"draft_max outside 1..{DRAFT_MAX_LIMIT}")
        self.ngram_min, self.ngram_max, self.draft_max = int(ngram_min), int(ngram_max), int(draft_max)
        self.ctx: List[int] = []
        # (one length below ngram_min is indexed too: may_draft_after_next looks the (n - 1)-grams up)
        self._idx: Dict[int, Dict[Tuple[int, ...], int]] = {n: {} for n in range(max(1, self.ngram_min - 1),
                                                                                 self.ngram_max + 1)}
        self.pred: List[int] = [int(t) for t in (prediction or [])]
        self._pidx: Dict[int, Dict[Tuple[int, ...], int]] = {n: {} for n in range(self.ngram_min, self.ngram_max + 1)}
        # the prediction's m-grams that have at least TWO tokens behind them, m = n - 1 (may_draft_after_next)
        self._phint = {m: {tuple(self.pred[j:j + m]) for j in range(len(self.pred) - m - 1)}
                       for m in range(self.ngram_min - 1, self.ngram_max)}
        for n, d in self._pidx.items():
            for j in range(len(self.pred) - n):  # j + n <= len - 1: a token follows; a later start overwrites
                d[tuple(self.pred[j:j + n])] = j
        for t in ids:
            self.append(t)

    def append(self, tok: int) -> None:
        """One more token of the context: it is the follower the n-grams ending just before it lacked."""
        L = len(self.ctx)
        self.ctx.append(int(tok))
        for n, d in self._idx.items():
            if L - n >= 0:
                d[tuple(self.ctx[L - n:L])] = L - n

    def draft(self, limit: Optional[int] = None) -> List[int]:
        """The draft behind the current context, at most min(draft_max, limit) tokens; [] when nothing matches."""
        k = self.draft_max if limit is None else min(self.draft_max, int(limit))
        if k <= 0:
            return []
        for n in range(self.ngram_max, self.ngram_min - 1, -1):
            if len(self.ctx) < n:
                continue
            tail = tuple(self.ctx[-n:])
            for src, idx in ((self.pred, self._pidx[n]), (self.ctx, self._idx[n])):
                j = idx.get(tail)
                if j is not None:
                    return src[j + n:j + n + k]
        return []

    def may_draft_after_next(self) -> bool:
        """Whether draft() can return anything once ONE more token, not known yet, has been appended: a
        necessary condition, O(1).  The trailing n-gram will then end in that token, so its first n - 1 tokens
        -- the context's trailing (n - 1)-gram -- must have occurred before with a token behind them (the one
        the unknown token has to equal; what follows may be the unknown token itself), or in the prediction
        with two tokens behind them.  False: whatever the next token is, nothing will be drafted."""
        for n in range(self.ngram_min, self.ngram_max + 1):
            m = n - 1
            if len(self.ctx) < m:
                continue
            g = tuple(self.ctx[-m:]) if m else ()
            if g in self._phint[m]:
                return True
            if (m == 0 and self.ctx) or (m and g in self._idx[m]):
                return True
        return False
