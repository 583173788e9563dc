"""The engine's paged KV cache under slot churn (csrc/engine.hip: kv_prepare_write, kv_sync, copy_slot,
release_slot), checked bit for bit against a host model of the allocator (tests/kv_paging_oracle.py).

A driver applies a script of operations to the engine and to the model in lockstep, keeps every live slot's
token list and a kv_read snapshot of it, and after EVERY operation asserts
  * bookkeeping: every slot's block_table and kv_blocks_free equal the model's, and so do the tables on the
    device (kv_device_tables: the slot table the stores go through and the row table the decode attention
    reads -- a stale row table changes no cache byte, only what a row attends to);
  * isolation: every position of every live slot that the operation does not write holds the bytes it held
    before (a skipped or wrong copy-on-write, a store through a stale row or slot table, a copy_slot that
    disturbs its source, a release that frees a block in use);
  * copies: after copy_slot(src, dst, n), kv_read(dst, n) == kv_read(src, n);
  * writes land: a position written with another token than it held has other bytes in every layer's K and
    V, and a newly written position has no all-zero K or V row (a zero row is what the null block holds).
At checkpoints and at the end every live slot decodes one step and its logits are compared with a fresh engine
(same file and settings; untouched free list, no sharing, no release) that prefilled the slot's whole token
list and decodes the same token in the same batch, to 2e-2 of the logit scale -- the suite's bound for a shared
prefix against a fresh prefill -- and one slot per script with the fp32 reference model at the same bound.

The null block.  Unmapped table entries point at one extra block on the device.  Every K / V store goes through
a table entry at (slot[row], pos[row]): qkv_post's two kernels and the QKV epilogues of the GEMV, skinny-GEMM
and prefill-GEMM launches.  Each is launched for exactly the rows of the step (the decode graphs are captured
per batch size, so there are no padded rows; the GEMM epilogues drop rows m >= M), and kv_prepare_write maps
every position of a step before it runs -- spec_decode's rejected rows and a loop's later steps included.  So
nothing legitimately stores to the null block, and every script ends by asserting it is still all zero.

test-small (3 layers, 2 KV heads, head_dim 64), max_ctx 512 = 4 blocks per slot, 4 slots = 16 blocks, both
prefill paths, bf16 and fp8 caches (fixed fp8 scales, as test_engine_gpu.test_fp8_kv_cache_matches_reference).
"""
import numpy as np
import pytest

import kv_paging_oracle as O

pytestmark = pytest.mark.gpu

MAX_CTX, SLOTS, BATCH = 512, 4, 4
TWIN_BOUND = 2e-2
WORST = {}          # (kv_dtype, prefill path) -> largest twin / reference error seen, as a fraction of the bound


def fp8_scales(n_layers):
    return [0.05 if i % 2 == 0 else 0.02 for i in range(2 * n_layers)]


def make_engine(path, kv):
    from aios_amd.runtime.loader import load_engine

    eng, cfg, _ = load_engine(path, max_ctx=MAX_CTX, max_slots=SLOTS, max_batch=BATCH, act_q8=False, kv_dtype=kv)
    if kv != "bf16":
        eng.set_kv_scales(fp8_scales(cfg.n_layers))
    return eng, cfg


_REFS = {}


def reference(path, kv):
    from aios_amd.models.config import get_preset
    from aios_amd.models.reference import ReferenceModel

    if kv not in _REFS:
        if kv == "bf16":
            _REFS[kv] = ReferenceModel.from_gguf(path, kv_bf16=True)
        else:
            _REFS[kv] = ReferenceModel.from_gguf(path, kv_fp8=True, kv_scales=fp8_scales(get_preset("test-small").n_layers))
    return _REFS[kv]


@pytest.fixture(scope="module")
def model_file(tmp_path_factory):
    from aios_amd.models.config import get_preset
    from aios_amd.models.synthetic import write_synthetic_gguf

    d = tmp_path_factory.mktemp("kvpaging")
    return write_synthetic_gguf(str(d / "small_Q4_K_M.gguf"), get_preset("test-small"), "Q4_K_M", seed=7)


class Driver:
    def __init__(self, path, kv, key, label, seed):
        self.path, self.kv, self.key, self.label = path, kv, key, label
        self.eng, self.cfg = make_engine(path, kv)
        self.model = O.PagedKV(MAX_CTX, SLOTS)
        assert self.eng.kv_blocks_total == self.model.total == 16
        assert self.eng.kv_blocks_free == self.model.blocks_free
        self.dt = np.uint16 if kv == "bf16" else np.uint8
        self.rng = np.random.default_rng(seed)
        self.toks, self.snap = {}, {}
        self.n_ops = 0
        self.twins = 0

    # ---- helpers
    def rand(self, n):
        return [int(t) for t in self.rng.integers(3, self.cfg.vocab_size, n)]

    def length(self, s):
        return len(self.toks.get(s, ()))

    def read(self, s, n):
        c = self.cfg
        raw = np.frombuffer(self.eng.kv_read(s, n), dtype=self.dt)
        return raw.reshape(c.n_layers, 2, c.n_kv_heads, n, c.head_dim)

    def where(self, desc):
        return f"[{self.label}, op {self.n_ops}: {desc}]"

    def _after(self, desc, writes, new, replaced=(), rows=()):
        """the per-operation checks; new: {slot: its token list now (empty: the slot is no longer live)},
        replaced: slots whose earlier content the operation dropped as a whole, rows: the slots of the step's
        batch rows (None: the operation uploads no table -- release_slot leaves that to the next one)"""
        at = self.where(desc)
        eng, m = self.eng, self.model
        m.check()
        for s in range(SLOTS):
            assert eng.block_table(s) == m.block_table(s), f"{at} slot {s}: table {eng.block_table(s)}, model {m.block_table(s)}"
        assert eng.kv_blocks_free == m.blocks_free, f"{at} {eng.kv_blocks_free} blocks free, model {m.blocks_free}"
        if rows is not None:
            # the device copies kv_sync keeps: the slot table, and the row table the step's attention read
            dev = [int(b) for b in eng.kv_device_tables(len(rows))]
            want = [m.total if b < 0 else b for s in list(range(SLOTS)) + list(rows) for b in m.block_table(s)]
            assert dev == want, f"{at} device tables (slots, then rows {list(rows)}) {dev}, model {want}"
        old, cur = self.toks, dict(self.toks)
        for s, t in new.items():
            if t:
                cur[s] = list(t)
            else:
                cur.pop(s, None)
        snaps = {}
        for s, t in cur.items():
            n_old = len(old[s]) if s in old and s not in replaced else 0
            n_new = len(t)
            now = self.read(s, max(n_old, n_new))
            wr = sorted(p for (ws, p) in writes if ws == s)
            if n_old:
                keep = np.ones(n_old, bool)
                keep[[p for p in wr if p < n_old]] = False
                same = (now[:, :, :, :n_old] == self.snap[s]).all(axis=(0, 1, 2, 4))
                bad = np.flatnonzero(keep & ~same)
                assert bad.size == 0, f"{at} slot {s}: {bad.size} positions the operation does not write changed, first {bad[:8].tolist()}"
            for p in wr:
                if p >= n_new:
                    continue
                row = now[:, :, :, p]                                        # [layer][K, V][head][head_dim]
                if p < n_old:
                    if old[s][p] != t[p]:
                        diff = (row != self.snap[s][:, :, :, p]).any(axis=(2, 3))
                        assert diff.all(), f"{at} slot {s} position {p}: another token, the same bytes in [layer][K, V] {(~diff).tolist()}"
                else:
                    nz = (row != 0).any(axis=3)
                    assert nz.all(), f"{at} slot {s} position {p}: written, but an all-zero row in [layer][K, V][head] {(~nz).tolist()}"
            snaps[s] = now[:, :, :, :n_new].copy()
        self.toks, self.snap = cur, snaps
        self.n_ops += 1

    # ---- operations
    def prefill(self, s, tokens, start=None):
        tokens = self.rand(tokens) if isinstance(tokens, int) else list(tokens)
        start = self.length(s) if start is None else start
        assert 0 <= start <= self.length(s) and start + len(tokens) <= MAX_CTX
        self.eng.prefill(s, tokens, start, False)
        w = self.model.prefill(s, start, len(tokens))
        self._after(f"prefill(slot {s}, {len(tokens)} tokens at {start})", w, {s: self.toks.get(s, [])[:start] + tokens})

    def decode(self, slots, pos=None):
        slots = list(slots)
        pos = [self.length(s) for s in slots] if pos is None else list(pos)
        assert all(0 <= p <= self.length(s) and p < MAX_CTX for s, p in zip(slots, pos))
        tokens = self.rand(len(slots))
        self.eng.decode(slots, tokens, pos)
        w = self.model.decode(slots, pos)
        self._after(f"decode(slots {slots}, pos {pos})", w,
                    {s: self.toks.get(s, [])[:p] + [t] for s, p, t in zip(slots, pos, tokens)}, rows=slots)

    def loop(self, slots, n, graph, pos=None):
        slots, B = list(slots), len(slots)
        pos = [self.length(s) for s in slots] if pos is None else list(pos)
        assert all(0 <= p <= self.length(s) and p + n <= MAX_CTX for s, p in zip(slots, pos))
        first = self.rand(B)
        self.eng.decode_loop_prepare(slots, first, pos)
        self.eng.decode_loop_run(B, n, graph)
        self.eng.synchronize()
        hist = np.asarray(self.eng.decode_loop_history(B, 0, MAX_CTX + 1)).reshape(B, MAX_CTX + 1)
        w = self.model.decode_loop(slots, pos, n)
        new = {s: self.toks.get(s, [])[:p] + [first[b]] + [int(t) for t in hist[b, p + 1:p + n]]
               for b, (s, p) in enumerate(zip(slots, pos))}
        self._after(f"decode_loop({'graph' if graph else 'eager'}, slots {slots}, pos {pos}, {n} steps)", w, new, rows=slots)

    def pipe(self, slots):
        """two pipelined steps: the second forward is queued from the token the first sampler leaves on the
        device, before the host has collected it"""
        slots = list(slots)
        pos = [self.length(s) for s in slots]
        assert all(p + 2 <= MAX_CTX for p in pos)
        first = self.rand(len(slots))
        self.eng.decode_submit(slots, first, pos)
        w = self.model.decode(slots, pos)
        self.eng.decode_sample(b"")
        self.eng.decode_submit(slots, [], [p + 1 for p in pos])
        w |= self.model.decode(slots, [p + 1 for p in pos])
        second = [int(t) for t in self.eng.decode_collect()]
        self.eng.decode_sample(b"")
        self.eng.decode_collect()
        self._after(f"decode_submit x 2(slots {slots}, pos {pos})", w,
                    {s: self.toks.get(s, [])[:p] + [a, b] for s, p, a, b in zip(slots, pos, first, second)}, rows=slots)

    def spec(self, s, tokens):
        """tokens[0] goes in at the slot's length, tokens[1:] are the draft; returns (accepted, emitted)"""
        pos0, R = self.length(s), len(tokens)
        assert pos0 + R <= MAX_CTX
        acc, out = self.eng.spec_decode(s, list(tokens), pos0)
        w = self.model.spec_decode(s, pos0, R)
        self._after(f"spec_decode(slot {s}, pos0 {pos0}, {R} rows) accepted {acc}", w,
                    {s: self.toks.get(s, [])[:pos0] + list(tokens[:acc + 1])}, rows=[s] * R)
        return int(acc), [int(t) for t in out]

    def copy(self, src, dst, n):
        self.eng.copy_slot(src, dst, n)
        w = self.model.copy_slot(src, dst, n)
        desc = f"copy_slot({src}, {dst}, {n})"
        if src == dst:
            return self._after(desc, w, {}, rows=None)
        k = max(0, min(n, self.length(src)))                 # what of dst is a sequence afterwards
        at = self.where(desc)
        self._after(desc, {(d, p) for d, p in w if p < k}, {dst: self.toks.get(src, [])[:k]}, replaced={dst})
        if k:
            assert self.eng.kv_read(dst, k) == self.eng.kv_read(src, k), f"{at} dst's first {k} positions are not src's"

    def release(self, s):
        self.eng.release_slot(s)
        self._after(f"release_slot({s})", self.model.release_slot(s), {s: []}, replaced={s}, rows=None)

    # ---- checkpoints
    def twin(self, ref=False):
        """every live slot decodes one step (in one batch); the same rows on a fresh engine that prefilled the
        slots' token lists; one row against the fp32 reference model when ref"""
        order = [int(s) for s in self.rng.permutation(sorted(self.toks))]
        assert order and all(self.length(s) < MAX_CTX for s in order), "a live slot has no room for the twin's step"
        B = len(order)
        at = self.where(f"twin of slots {order}")
        self.decode(order)
        got = np.asarray(self.eng.last_logits(B)).reshape(B, -1).copy()
        fresh, _ = make_engine(self.path, self.kv)
        for i, s in enumerate(order):
            fresh.prefill(i, self.toks[s][:-1], 0, False)
        fresh.decode(list(range(B)), [self.toks[s][-1] for s in order], [self.length(s) - 1 for s in order])
        tables = [fresh.block_table(i) for i in range(B)]
        mapped = [b for t in tables for b in t if b >= 0]
        assert len(mapped) == len(set(mapped)) and not any(O.non_monotonic(t) for t in tables)
        want = np.asarray(fresh.last_logits(B)).reshape(B, -1)
        for i, s in enumerate(order):
            self._logits(f"{at} slot {s} ({self.length(s)} tokens) against the fresh engine", got[i], want[i])
        if ref:
            s = order[0]
            rl = reference(self.path, self.kv).forward(self.toks[s])[-1].numpy()
            self._logits(f"{at} slot {s} ({self.length(s)} tokens) against the reference model", got[0], rl)
        self.twins += 1

    def _logits(self, at, got, want):
        err, bound = float(np.abs(got - want).max()), TWIN_BOUND * max(float(np.abs(want).max()), 1.0)
        WORST[self.key] = max(WORST.get(self.key, 0.0), err / bound)
        print(f"{at}: error {err:.4g}, bound {bound:.4g} ({err / bound:.3f} of it)")
        assert np.isfinite(got).all() and err < bound, f"{at}: error {err}, bound {bound}"

    def end(self):
        """the script's last checkpoint, the two accessors against each other, the null block, and the pool"""
        self.twin(ref=True)
        c, total = self.cfg, self.eng.kv_blocks_total
        shape = (c.n_layers, 2, c.n_kv_heads, O.KV_BLOCK, c.head_dim)
        for s, t in self.toks.items():
            for j, b in enumerate(self.eng.block_table(s)):
                n = min(len(t) - j * O.KV_BLOCK, O.KV_BLOCK)
                if b >= 0 and n > 0:
                    blk = np.frombuffer(self.eng.kv_read_block(b), dtype=self.dt).reshape(shape)
                    assert np.array_equal(blk[:, :, :, :n], self.snap[s][:, :, :, j * O.KV_BLOCK:j * O.KV_BLOCK + n]), \
                        f"[{self.label}] kv_read_block({b}) is not entry {j} of slot {s}"
        null = np.frombuffer(self.eng.kv_read_block(total), dtype=np.uint8)
        assert null.size == int(np.prod(shape)) * self.dt().itemsize
        assert not null.any(), f"[{self.label}] {int(np.count_nonzero(null))} bytes of the null block were written"
        for s in sorted(self.toks):
            self.release(s)
        assert self.eng.kv_blocks_free == total and all(self.eng.block_table(s) == [-1] * 4 for s in range(SLOTS))
        assert self.twins >= 1 and not self.toks
        print(f"[{self.label}] {self.n_ops} operations; worst logit error so far for {self.key}: {WORST[self.key]:.3f} of the bound")


# ---- the fixed scripts ------------------------------------------------------------------------------
def script_prefill_seams_and_rewinds(d):
    d.prefill(0, [1] + d.rand(99))
    d.prefill(0, 60)                    # 100..159: straddles 128
    d.prefill(0, 96)                    # 160..255: ends exactly on the seam, block 2 stays unmapped
    assert d.length(0) == 256 and d.model.block_table(0)[2] == -1
    d.prefill(0, 140, 250)              # a rewind inside a private block; 250..389 straddles 256 and 384
    d.copy(0, 1, 300)
    d.prefill(1, 30)                    # slot 1's own suffix in its private partial block
    d.prefill(0, 50, 100)               # a rewind inside a shared block (and on into the next one): un-shares both
    assert d.model.unshared == [(0, 0, 5), (0, 1, 6)]
    d.prefill(1, 20, 256)               # a rewind exactly at a block boundary, private block
    d.copy(1, 2, 256)
    d.twin()
    d.prefill(2, 10, 128)               # a rewind exactly at a block boundary, shared block
    assert len(d.model.unshared) == 1
    d.prefill(0, 256 - d.length(0))     # up to the seam again, and no further
    assert d.length(0) == 256
    d.prefill(1, 130, 254)              # 254..383: straddles 256, ends exactly on 384
    assert d.length(1) == 384 and d.model.block_table(1)[3] == -1
    d.prefill(1, 3)                     # 384..386: the first rows of the last block
    d.end()


def script_copy_slot_cases(d):
    d.prefill(0, [1] + d.rand(299))
    d.prefill(2, 200)
    for n in (0, 1, 127, 128, 129, 256, 300):
        # onto an empty dst first; from 129 on, onto a dst that shares block 0 with src
        d.copy(0, 1, n)
        if n:
            d.decode([1])               # dst goes on by itself: its partial block, or a block of its own
        if n == 128:
            assert d.model.block_table(1)[0] == d.model.block_table(0)[0] and d.model.refcnt[d.model.block_table(0)[0]] == 2
    d.copy(0, 0, 100)                   # src == dst: nothing happens
    d.copy(0, 2, 129)                   # onto an occupied dst that shares nothing with src
    d.decode([2, 0, 1])
    d.copy(0, 3, 1 << 20)               # clipped to the context: the whole of src, shared block by block
    d.decode([3, 0])                    # both write into the block they share (src's partial one): one un-shares
    d.copy(3, 1, 0)                     # n = 0 onto an occupied dst: dropped
    assert d.length(1) == 0 and d.model.block_table(1) == [-1] * 4
    d.copy(1, 2, 64)                    # from an empty src: dropped as well
    assert d.length(2) == 0
    d.end()


def script_three_way_share(d):
    d.prefill(0, [1] + d.rand(199))
    d.copy(0, 1, 200)
    d.copy(0, 2, 200)
    b0 = d.model.block_table(0)[0]
    assert d.model.refcnt[b0] == 3
    d.prefill(1, 5, 100)                # each holder writes into the block in turn
    assert d.model.refcnt[b0] == 2 and d.model.unshared == [(1, b0, d.model.block_table(1)[0])]
    d.decode([2], [90])
    assert d.model.refcnt[b0] == 1 and len(d.model.unshared) == 1
    d.prefill(0, 5, 80)                 # the last holder writes in place
    assert d.model.unshared == [] and d.model.block_table(0)[0] == b0
    d.copy(0, 3, 85)
    d.decode([3, 2, 1, 0])
    d.end()


def script_batched_decode(d):
    d.prefill(0, [1] + d.rand(126))     # 127
    d.prefill(1, 255)
    d.prefill(2, 60)
    d.decode([0, 1, 2])                 # positions 127 and 255: the last rows of two blocks, in one step
    assert d.model.block_table(0)[1] == -1 and d.model.block_table(1)[2] == -1
    d.decode([2, 0, 1])                 # positions 128 and 256 map two blocks; the same captured graph, another row table
    assert d.model.block_table(0)[1] >= 0 and d.model.block_table(1)[2] >= 0
    d.decode([1, 2, 0])
    d.copy(0, 3, 128)
    d.prefill(3, 20)
    d.decode([0, 3])                    # two rows that share a prefix block
    d.decode([3, 0])
    d.decode([0, 1, 2, 3])
    d.decode([3, 2, 1, 0])
    d.twin()
    d.copy(1, 2, 256)
    d.decode([1, 2], [200, 200])        # both rows write into the block they share: the first un-shares
    assert len(d.model.unshared) == 1
    d.decode([2, 1])
    d.release(0)
    d.release(3)
    before = d.model.block_table(1)
    d.prefill(0, 140)                   # slot 0 again, in other blocks than it had
    d.decode([0, 1, 2])                 # the B = 3 graph again: row 0's table entries are all new
    assert d.model.block_table(1) == before
    d.decode([2, 1, 0])
    d.end()


def script_decode_paths(d):
    d.prefill(0, [1] + d.rand(124))     # 125
    d.prefill(1, 125)
    d.loop([0], 6, True)                # 125..130: over the seam inside one call
    d.loop([1], 6, False)
    assert d.length(0) == d.length(1) == 131
    d.prefill(2, 125)
    d.copy(2, 3, 125)
    d.loop([2, 3], 6, True)
    d.loop([3, 2], 6, False, [125, 125])  # the same positions again, rows swapped, eager
    d.twin()
    d.release(0)
    d.prefill(0, 127)
    d.pipe([0, 1])                      # 127, 128 and 131, 132: the second forward is queued behind the first sampler
    d.release(2)
    d.prefill(2, 126)
    d.copy(2, 3, 126)
    t0 = d.rand(1)
    acc, out = d.spec(3, t0 + d.rand(3))            # what the 4-row step draws after t0, on a copy
    acc, out = d.spec(2, t0 + [out[0]] + d.rand(2))  # draft 1 right, the others wrong; 126..129 all stored
    assert 1 <= acc < 3, acc
    assert d.length(2) == 126 + acc + 1
    d.decode([2])                       # overwrites the first rejected row's position
    d.decode([2, 3])
    d.end()


def script_churn_and_full_pool(d):
    d.prefill(0, [1] + d.rand(299))
    d.prefill(1, 200)
    d.prefill(2, 140)
    d.release(1)
    d.prefill(3, 400)
    d.release(0)
    d.prefill(1, 390)
    d.copy(1, 0, 200)
    d.release(2)
    d.prefill(0, 100, 150)
    d.prefill(2, 260)
    d.decode([2, 0])
    assert any(O.non_monotonic(d.eng.block_table(s)) for s in d.toks), [d.eng.block_table(s) for s in range(SLOTS)]
    d.twin()
    for s in (3, 1, 0, 2):
        d.release(s)
    for s in (2, 0, 3, 1):
        d.prefill(s, 511)
    assert d.eng.kv_blocks_free == 0
    assert any(O.non_monotonic(d.eng.block_table(s)) for s in range(SLOTS))
    d.end()                             # every slot decodes at position 511 in a full pool, then all are released


def script_random(d, n_ops=40):
    """operations drawn from the fixed scripts' set; lengths stay at or below 500 so that every live slot has
    room for a checkpoint's step"""
    rng, LIM = d.rng, 500
    for i in range(n_ops):
        live = sorted(d.toks)
        empty = [s for s in range(SLOTS) if s not in d.toks]
        room = lambda k: [s for s in live if d.length(s) + k <= LIM]
        ops = ["copy", "copy"] if live else []
        ops += ["new", "new"] if empty else []
        ops += ["release"] if len(live) >= 2 else []
        ops += ["rewind", "rewind", "redecode"] if live else []
        ops += ["extend", "decode", "decode", "decode"] if room(1) else []
        ops += ["loop", "loop", "pipe", "spec"] if room(6) else []
        op = ops[int(rng.integers(len(ops)))]
        pick = lambda xs: xs[int(rng.integers(len(xs)))]
        some = lambda xs, most: [int(s) for s in rng.permutation(xs)[:int(rng.integers(1, min(most, len(xs)) + 1))]]
        if op == "new":
            d.prefill(pick(empty), int(pick([1, 60, 127, 128, 129, 200, 256, 300, int(rng.integers(1, 400))])))
        elif op == "extend":
            s = pick(room(1))
            d.prefill(s, int(rng.integers(1, min(150, LIM - d.length(s)) + 1)))
        elif op == "rewind":
            s = pick(live)
            n = d.length(s)
            start = int(pick([0, n // 128 * 128, max(n - 1, 0), int(rng.integers(0, n))]))
            d.prefill(s, int(rng.integers(1, max(1, min(100, LIM - start)) + 1)), start)
        elif op == "copy":
            src = pick(live)
            n = int(pick([0, 1, 127, 128, 129, 256, d.length(src), int(rng.integers(0, 512))]))
            d.copy(src, int(rng.integers(SLOTS)), n)
        elif op == "release":
            d.release(pick(live))
        elif op == "decode":
            d.decode(some(room(1), 4))
        elif op == "redecode":
            rows = some(live, 4)
            d.decode(rows, [int(rng.integers(0, d.length(s))) for s in rows])
        elif op == "loop":
            d.loop(some(room(6), 4), int(rng.integers(1, 7)), bool(rng.integers(2)))
        elif op == "pipe":
            d.pipe(some(room(6), 4))
        else:
            d.spec(pick(room(6)), d.rand(int(rng.integers(2, 5))))
        if i == n_ops // 2 and d.toks:
            d.twin()
    if not d.toks:
        d.prefill(0, 130)
    d.end()


SCRIPTS = {
    "prefill_seams_and_rewinds": script_prefill_seams_and_rewinds,
    "copy_slot_cases": script_copy_slot_cases,
    "three_way_share": script_three_way_share,
    "batched_decode": script_batched_decode,
    "decode_paths": script_decode_paths,
    "churn_and_full_pool": script_churn_and_full_pool,
    "random_seed_1": script_random,
    "random_seed_2": script_random,
    "random_seed_3": script_random,
}


@pytest.mark.parametrize("script", list(SCRIPTS))
@pytest.mark.parametrize("gemm_prefill", ["0", "1"])
@pytest.mark.parametrize("kv", ["bf16", "fp8_e4m3"])
def test_paged_kv_under_churn(model_file, monkeypatch, kv, gemm_prefill, script):
    monkeypatch.setenv("AIOS_PREFILL_GEMM", gemm_prefill)
    seed = int(script.rsplit("_", 1)[1]) if script.startswith("random") else 100 + list(SCRIPTS).index(script)
    d = Driver(model_file, kv, (kv, "gemm" if gemm_prefill == "1" else "gemv"), f"{script}, seed {seed}, {kv}, gemm {gemm_prefill}", seed)
    SCRIPTS[script](d)
