"""The paged KV cache's block bookkeeping in plain Python (csrc/engine.hip: kv_alloc, kv_unref,
kv_prepare_write, copy_slot, release_slot; the tables' device copies and the cache bytes are not modelled).

A slot has max_ctx / KV_BLOCK table entries, -1 = unmapped.  Blocks are refcounted; the free list is LIFO and
starts so that block 0 is handed out first.  A write to [from, to) maps the unmapped entries it touches and
un-shares (fresh block, the old one's reference dropped) those whose block has other holders.  Nothing un-maps
a block when a sequence is rewound: only copy_slot (onto its dst) and release_slot drop references.

Every operation returns the set of (slot, position) pairs whose K / V the engine stores in it -- for copy_slot
the positions of dst that take src's content.  The step functions issue the prepare_write ranges the engine
issues for them (advance_rows, prefill_run, spec_decode): one range per row, in row order.
"""
from typing import Iterable, List, Sequence, Set, Tuple

KV_BLOCK = 128

Writes = Set[Tuple[int, int]]


class PoolExhausted(RuntimeError):
    pass


class PagedKV:
    def __init__(self, max_ctx: int, max_slots: int):
        self.max_ctx = (max_ctx + KV_BLOCK - 1) // KV_BLOCK * KV_BLOCK
        self.max_slots = max_slots
        self.maxb = self.max_ctx // KV_BLOCK
        self.total = max_slots * self.maxb
        self.tables = [[-1] * self.maxb for _ in range(max_slots)]
        self.refcnt = [0] * self.total
        self.free = list(range(self.total - 1, -1, -1))   # popped from the back: block 0 first
        self.unshared: List[Tuple[int, int, int]] = []    # (slot, old block, new block) of the last operation

    # ---- what the engine reports
    def block_table(self, slot: int) -> List[int]:
        return list(self.tables[slot])

    @property
    def blocks_free(self) -> int:
        return len(self.free)

    def mapped(self) -> Set[int]:
        return {b for row in self.tables for b in row if b >= 0}

    def check(self) -> None:
        """free + distinct mapped == total, and every refcount is the number of table entries that hold the block"""
        holders = [0] * self.total
        for row in self.tables:
            for b in row:
                if b >= 0:
                    holders[b] += 1
        assert len(self.free) == len(set(self.free)), "a block is on the free list twice"
        assert not set(self.free) & self.mapped(), "a mapped block is on the free list"
        assert len(self.free) + len(self.mapped()) == self.total, (len(self.free), len(self.mapped()), self.total)
        assert self.refcnt == holders, (self.refcnt, holders)

    # ---- the allocator
    def _alloc(self) -> int:
        if not self.free:
            raise PoolExhausted("paged KV: pool exhausted")
        b = self.free.pop()
        self.refcnt[b] = 1
        return b

    def _unref(self, b: int) -> None:
        if b < 0:
            return
        self.refcnt[b] -= 1
        if self.refcnt[b] == 0:
            self.free.append(b)

    def _slot(self, slot: int) -> List[int]:
        if not 0 <= slot < self.max_slots:
            raise ValueError("bad slot")
        return self.tables[slot]

    def prepare_write(self, slot: int, frm: int, to: int) -> None:
        row = self._slot(slot)
        if to <= frm:
            return
        for j in range(frm // KV_BLOCK, min((to - 1) // KV_BLOCK, self.maxb - 1) + 1):
            if row[j] < 0:
                row[j] = self._alloc()
            elif self.refcnt[row[j]] > 1:
                nb = self._alloc()
                self.unshared.append((slot, row[j], nb))
                self._unref(row[j])
                row[j] = nb

    # ---- the engine's operations
    def prefill(self, slot: int, start: int, n: int) -> Writes:
        if n < 1 or start < 0 or start + n > self.max_ctx:
            raise ValueError("prefill: range out of the context")
        self.unshared = []
        self.prepare_write(slot, start, start + n)
        return {(slot, p) for p in range(start, start + n)}

    def decode_loop(self, slots: Sequence[int], pos: Sequence[int], n: int) -> Writes:
        """n steps of the rows (slots[b], pos[b]): row b stores positions pos[b] .. pos[b] + n - 1"""
        if len(slots) != len(pos) or n < 1 or any(p < 0 or p + n > self.max_ctx for p in pos):
            raise ValueError("decode: rows out of the context")
        self.unshared = []
        out: Writes = set()
        for s, p in zip(slots, pos):
            self.prepare_write(s, p, min(p + n, self.max_ctx))
            out |= {(s, q) for q in range(p, p + n)}
        return out

    def decode(self, slots: Sequence[int], pos: Sequence[int]) -> Writes:
        return self.decode_loop(slots, pos, 1)

    def spec_decode(self, slot: int, pos0: int, rows: int) -> Writes:
        """rows consecutive positions of one slot as the rows of one step: every row is prepared and stored,
        accepted or not"""
        return self.decode([slot] * rows, list(range(pos0, pos0 + rows)))

    def copy_slot(self, src: int, dst: int, n: int) -> Writes:
        s, d = self._slot(src), self._slot(dst)
        self.unshared = []
        if src == dst:
            return set()
        n = min(n, self.max_ctx)
        for j in range(self.maxb):
            self._unref(d[j])
            d[j] = -1
        full = max(n, 0) // KV_BLOCK
        for j in range(full):
            d[j] = s[j]
            if d[j] >= 0:
                self.refcnt[d[j]] += 1
        if n > 0 and n % KV_BLOCK and s[full] >= 0:
            d[full] = self._alloc()
        return {(dst, p) for p in range(max(n, 0))}

    def release_slot(self, slot: int) -> Writes:
        row = self._slot(slot)
        self.unshared = []
        for j in range(self.maxb):
            self._unref(row[j])
            row[j] = -1
        return set()


def non_monotonic(table: Iterable[int]) -> bool:
    """the mapped entries of a table are not in increasing block order (the free list has been permuted)"""
    m = [b for b in table if b >= 0]
    return any(b <= a for a, b in zip(m, m[1:]))
