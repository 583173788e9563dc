"""tests/kv_paging_oracle.py on cases worked out by hand: the block numbers below follow from the engine's
rules alone (LIFO free list that starts at block 0, whole blocks shared, a partial block copied, writes
un-share), for the GPU tests' pool: max_ctx 512 and 4 slots = 4 entries per slot, 16 blocks."""
import random

import pytest

import kv_paging_oracle as O


def pool():
    return O.PagedKV(512, 4)


def test_pool_starts_empty_in_the_engines_order():
    m = pool()
    assert (m.maxb, m.total, m.blocks_free) == (4, 16, 16)
    assert all(m.block_table(s) == [-1] * 4 for s in range(4))
    assert m.prefill(2, 0, 1) == {(2, 0)} and m.block_table(2) == [0, -1, -1, -1]   # block 0 first
    assert O.PagedKV(500, 2).max_ctx == 512                                          # whole blocks


def test_the_existing_gpu_tests_numbers():
    """400 tokens map 4 blocks; copy_slot(0, 1, 300) shares two, makes one private, leaves one unmapped"""
    m = pool()
    w = m.prefill(0, 0, 400)
    assert w == {(0, p) for p in range(400)}
    assert m.block_table(0) == [0, 1, 2, 3] and m.blocks_free == 12
    w = m.copy_slot(0, 1, 300)
    assert w == {(1, p) for p in range(300)}
    assert m.block_table(1) == [0, 1, 4, -1] and m.block_table(0) == [0, 1, 2, 3]
    assert m.blocks_free == 11 and m.refcnt[:5] == [2, 2, 1, 1, 1]
    # slot 1's own suffix lands in its private block; a rewind of slot 0 into block 0 un-shares it
    m.prefill(1, 300, 60)
    assert m.block_table(1) == [0, 1, 4, -1] and m.unshared == []
    m.prefill(0, 100, 50)
    assert m.unshared == [(0, 0, 5), (0, 1, 6)]          # positions 100..149: entries 0 and 1, both shared
    assert m.block_table(0) == [5, 6, 2, 3] and m.block_table(1) == [0, 1, 4, -1]
    assert m.refcnt[:7] == [1, 1, 1, 1, 1, 1, 1] and m.blocks_free == 9
    for s in range(3):
        m.release_slot(s)
    assert m.blocks_free == 16
    m.check()


def test_copy_onto_a_dst_that_already_shares_with_src():
    m = pool()
    m.prefill(0, 0, 400)
    m.copy_slot(0, 1, 300)                               # [0, 1, 4, -1]
    m.copy_slot(0, 1, 129)
    # dst dropped first: blocks 0 and 1 fall to one holder, 4 goes back on the list and is the next one out
    assert m.block_table(1) == [0, 4, -1, -1] and m.refcnt[:5] == [2, 1, 1, 1, 1]
    assert m.blocks_free == 11
    m.copy_slot(1, 0, 200)                               # the other way: src's blocks survive dst's drop
    assert m.block_table(0) == [0, 3, -1, -1] and m.block_table(1) == [0, 4, -1, -1]
    assert m.refcnt[:5] == [2, 0, 0, 1, 1] and m.blocks_free == 13
    assert m.free[-2:] == [1, 2]                         # 1, 2, 3 pushed in entry order, 3 popped again
    m.check()


@pytest.mark.parametrize("n,table,free,shared", [
    (0, [-1, -1, -1, -1], 13, 0),
    (1, [3, -1, -1, -1], 12, 0),
    (127, [3, -1, -1, -1], 12, 0),
    (128, [0, -1, -1, -1], 13, 1),
    (129, [0, 3, -1, -1], 12, 1),
    (256, [0, 1, -1, -1], 13, 2),
    (300, [0, 1, 3, -1], 12, 2),
    (301, [0, 1, 3, -1], 12, 2),      # past src's content: the partial block is copied all the same
    (384, [0, 1, 2, -1], 13, 3),
    (1 << 20, [0, 1, 2, -1], 13, 3),  # clipped to max_ctx: src's unmapped entry stays unmapped, no partial block
])
def test_copy_slot_lengths(n, table, free, shared):
    m = pool()
    m.prefill(0, 0, 300)                                 # [0, 1, 2, -1]
    w = m.copy_slot(0, 1, n)
    assert w == {(1, p) for p in range(min(n, 512))}
    assert m.block_table(1) == table and m.block_table(0) == [0, 1, 2, -1]
    assert m.blocks_free == free
    assert sum(c == 2 for c in m.refcnt) == shared
    m.check()


def test_copy_slot_onto_itself_and_from_an_empty_slot():
    m = pool()
    m.prefill(0, 0, 300)
    assert m.copy_slot(0, 0, 200) == set() and m.block_table(0) == [0, 1, 2, -1] and m.blocks_free == 13
    m.prefill(1, 0, 10)
    m.copy_slot(2, 1, 200)                               # an empty src: dst is dropped, nothing mapped
    assert m.block_table(1) == [-1] * 4 and m.blocks_free == 13
    m.check()


def test_unsharing_a_block_held_three_times():
    m = pool()
    m.prefill(0, 0, 128)
    m.copy_slot(0, 1, 128)
    m.copy_slot(0, 2, 128)
    assert m.refcnt[0] == 3 and m.blocks_free == 15
    m.prefill(1, 100, 5)
    assert m.unshared == [(1, 0, 1)] and m.refcnt[:2] == [2, 1] and m.block_table(1)[0] == 1
    m.prefill(2, 90, 5)
    assert m.unshared == [(2, 0, 2)] and m.refcnt[:3] == [1, 1, 1] and m.block_table(2)[0] == 2
    m.prefill(0, 80, 5)                                  # the last holder writes in place
    assert m.unshared == [] and m.block_table(0)[0] == 0 and m.blocks_free == 13
    m.check()


def test_two_rows_of_one_step_write_into_the_block_they_share():
    m = pool()
    m.prefill(0, 0, 256)
    m.copy_slot(0, 1, 256)
    assert m.block_table(1) == [0, 1, -1, -1]
    w = m.decode([0, 1], [200, 200])
    assert w == {(0, 200), (1, 200)}
    assert m.unshared == [(0, 1, 2)]                     # the first row un-shares, the second is the last holder
    assert m.block_table(0) == [0, 2, -1, -1] and m.block_table(1) == [0, 1, -1, -1]
    m.check()


def test_step_ranges():
    m = pool()
    m.prefill(0, 0, 125)
    assert m.decode_loop([0], [125], 6) == {(0, p) for p in range(125, 131)}
    assert m.block_table(0) == [0, 1, -1, -1]            # the loop maps the block its later steps reach
    m.prefill(1, 0, 126)
    assert m.spec_decode(1, 126, 4) == {(1, p) for p in range(126, 130)}
    assert m.block_table(1) == [2, 3, -1, -1]            # every row prepared, accepted or not
    m.prefill(2, 0, 127)
    m.prefill(3, 0, 255)
    assert m.decode([2, 3], [127, 255]) == {(2, 127), (3, 255)}
    assert m.block_table(2) == [4, -1, -1, -1] and m.block_table(3) == [5, 6, -1, -1]
    assert m.decode([3, 2], [256, 128]) == {(3, 256), (2, 128)}
    assert m.block_table(3) == [5, 6, 7, -1] and m.block_table(2) == [4, 8, -1, -1]   # mapped in row order
    assert m.decode([2], [511]) == {(2, 511)} and m.block_table(2) == [4, 8, -1, 9]
    with pytest.raises(ValueError):
        m.decode([2], [512])
    with pytest.raises(ValueError):
        m.decode_loop([2], [510], 3)
    m.check()


def test_a_rewind_unmaps_nothing():
    m = pool()
    m.prefill(0, 0, 400)
    m.prefill(0, 10, 5)
    m.decode([0], [3])
    assert m.block_table(0) == [0, 1, 2, 3] and m.blocks_free == 12


def test_release_down_to_an_empty_pool():
    m = pool()
    for s in range(4):
        m.prefill(s, 0, 512)
    assert m.blocks_free == 0 and sorted(m.mapped()) == list(range(16))
    with pytest.raises(O.PoolExhausted):
        m._alloc()
    m.copy_slot(0, 1, 512)                               # sharing in a full pool frees dst's blocks
    assert m.blocks_free == 4 and m.block_table(1) == [0, 1, 2, 3]
    m.decode([1], [511])                                 # and un-sharing takes one back
    assert m.blocks_free == 3 and m.block_table(1)[:3] == [0, 1, 2] and m.block_table(1)[3] == 7
    for s in (2, 0, 3, 1):
        m.release_slot(s)
    m.release_slot(1)                                    # releasing an empty slot changes nothing
    assert m.blocks_free == 16 and sorted(m.free) == list(range(16)) and m.refcnt == [0] * 16
    assert all(m.block_table(s) == [-1] * 4 for s in range(4))
    m.check()


def test_non_monotonic():
    assert not O.non_monotonic([0, 1, -1, -1]) and not O.non_monotonic([-1] * 4) and not O.non_monotonic([3, -1, 9, -1])
    assert O.non_monotonic([5, 2, -1, -1]) and O.non_monotonic([1, -1, 0, -1])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_conservation_over_a_long_random_script(seed):
    """free + distinct mapped == total, refcounts = holders, after every one of 3000 random operations; the
    pool never runs out (a mapping or un-sharing step needs no more blocks than there are table entries);
    every step's write set is the rows' positions"""
    rng = random.Random(seed)
    m = pool()
    seen_shared3 = False
    for i in range(3000):
        op = rng.choice(["prefill", "prefill", "decode", "loop", "spec", "copy", "copy", "release"])
        if op == "prefill":
            start = rng.randrange(0, 512)
            n = rng.randrange(1, 512 - start + 1)
            s = rng.randrange(4)
            assert m.prefill(s, start, n) == {(s, p) for p in range(start, start + n)}
        elif op == "decode":
            rows = rng.sample(range(4), rng.randrange(1, 5))
            pos = [rng.randrange(512) for _ in rows]
            assert m.decode(rows, pos) == set(zip(rows, pos))
        elif op == "loop":
            rows = rng.sample(range(4), rng.randrange(1, 3))
            n = rng.randrange(1, 7)
            pos = [rng.randrange(512 - n + 1) for _ in rows]
            assert m.decode_loop(rows, pos, n) == {(s, p + k) for s, p in zip(rows, pos) for k in range(n)}
        elif op == "spec":
            s, R = rng.randrange(4), rng.randrange(2, 5)
            pos0 = rng.randrange(512 - R + 1)
            assert m.spec_decode(s, pos0, R) == {(s, pos0 + k) for k in range(R)}
        elif op == "copy":
            m.copy_slot(rng.randrange(4), rng.randrange(4), rng.choice([0, 1, 127, 128, 129, 256, 300, 512, 9999]))
        else:
            m.release_slot(rng.randrange(4))
        m.check()
        seen_shared3 |= max(m.refcnt) >= 3
    assert seen_shared3                                   # the script got to the states it is about
    for s in range(4):
        m.release_slot(s)
    m.check()
    assert m.blocks_free == 16
