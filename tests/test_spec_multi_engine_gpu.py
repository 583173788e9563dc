"""Engine.spec_decode_multi on the device: S sequences' consecutive positions side by side as the Rt rows of one
decode step, the sampler on every row, the segmented accept kernel behind it (csrc/engine.hip,
csrc/kernels/spec_accept.hip).

The reference is the engine's own decode() of the same flat rows on copy_slot twins and the accept rule in plain
Python (tests/spec_multi_oracle.py): the same Rt-row kernels run on both sides, the weights are Q4_K_M (no float
atomics in those kernels), so tokens, logits and logprobs are compared for equality, bit for bit.  Each
sequence's draft is a chain built with the existing spec_decode on twins (test_spec_engine_gpu.py's build_chain):
its tokens come from the R-row kernels of THAT step, so the multi step -- other kernels above dec_gemm_min_b_ = 5
rows -- is not held to accepting all of it; what it must give is what decode() of its rows gives.

Two donors hold two prompts; a sequence is a copy_slot prefix of one of them at its own pos0 with its own input
token.  Work slots are copied afresh from the donors before every call, for the call under test and for its
reference alike.
"""
import numpy as np
import pytest

import spec_multi_oracle as M

pytestmark = pytest.mark.gpu

PROMPT_A = [1] + [(37 * i + 11) % 1000 + 3 for i in range(19)]    # 20 tokens
PROMPT_B = [1] + [(61 * i + 5) % 1000 + 3 for i in range(130)]    # 131 tokens: past the first KV block
FILL = 7
A, B = 0, 1                # donors
W = [2, 3, 4, 5]           # work slots


def make(kv_dtype="bf16", max_batch=16):
    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset("test-mistral-shape")
    eng = random_engine(cfg, "Q4_K_M", seed=5, max_ctx=256, max_slots=6, max_batch=max_batch, kv_dtype=kv_dtype)
    ta = int(np.asarray(eng.prefill(A, PROMPT_A, 0, True)).argmax())
    tb = int(np.asarray(eng.prefill(B, PROMPT_B, 0, True)).argmax())
    return eng, cfg, {A: (PROMPT_A, ta), B: (PROMPT_B, tb)}


@pytest.fixture(scope="module")
def engine():
    return make()


class Seq:
    """a sequence: the first pos0 tokens of a donor's prompt in `slot`, t0 the token that goes in at pos0"""

    def __init__(self, donors, donor, pos0, slot, rows):
        prompt, nxt = donors[donor]
        self.donor, self.pos0, self.slot, self.rows = donor, pos0, slot, rows
        self.t0 = nxt if pos0 == len(prompt) else prompt[pos0]
        self.kw = dict(temperature=0.0, top_k=0, top_p=1.0, seed=0)
        self.chain = None


def fresh(eng, seqs, slots=None):
    for i, q in enumerate(seqs):
        eng.copy_slot(q.donor, q.slot if slots is None else slots[i], q.pos0)


def build_chain(eng, q, spare):
    """c[0] = t0 and c[i + 1] = the token row i of a rows-row spec_decode samples when the drafts before it are right"""
    c = [q.t0]
    for j in range(q.rows - 1):
        eng.copy_slot(q.donor, spare, q.pos0)
        acc, out = eng.spec_decode(spare, c + [FILL] * (q.rows - len(c)), q.pos0, **q.kw)
        assert acc >= j
        c.append(int(out[j]))
    q.chain = c
    return c


def call_multi(eng, seqs, toks, **kw):
    fresh(eng, seqs)
    res = eng.spec_decode_multi([q.slot for q in seqs], toks, [q.pos0 for q in seqs],
                                [q.kw["temperature"] for q in seqs], [q.kw["top_k"] for q in seqs],
                                [q.kw["top_p"] for q in seqs], [q.kw["seed"] for q in seqs], **kw)
    return [(int(a), [int(t) for t in o]) for a, o in res]


def call_decode(eng, seqs, toks, mask=b""):
    """the same flat rows through decode() on fresh twins"""
    fresh(eng, seqs)
    slots, flat, pos, T, K, P, sd = [], [], [], [], [], [], []
    for q, t in zip(seqs, toks):
        for i, x in enumerate(t):
            slots.append(q.slot); flat.append(x); pos.append(q.pos0 + i)
            T.append(q.kw["temperature"]); K.append(q.kw["top_k"]); P.append(q.kw["top_p"]); sd.append(q.kw["seed"])
    return [int(t) for t in eng.decode(slots, flat, pos, T, K, 0, mask, P, sd)], flat


def bits(x):
    return np.asarray(x).view(np.uint32)


def compare(eng, seqs, toks):
    """spec_decode_multi against decode() + the oracle; returns the multi call's results"""
    Rt = sum(len(t) for t in toks)
    got = call_multi(eng, seqs, toks)
    lg = np.asarray(eng.last_logits(Rt)).copy()
    dec, flat = call_decode(eng, seqs, toks)
    assert np.array_equal(bits(lg), bits(eng.last_logits(Rt)))
    want = M.accept(flat, dec, M.segments([len(t) for t in toks]))
    print("segments", [len(t) for t in toks], "accepted", [a for a, _ in got], "decode rows", dec)
    assert got == want
    return got


def layout(eng, donors, spec, spare=5):
    """sequences for [(donor, pos0, rows), ...] in work slots W[0..], their chains built"""
    seqs = [Seq(donors, d, p, W[i], r) for i, (d, p, r) in enumerate(spec)]
    for q in seqs:
        build_chain(eng, q, spare)
    return seqs


LAYOUTS = {
    "4+1": [(A, 20, 4), (B, 131, 1)],           # Rt = 5
    "2+2": [(A, 20, 2), (B, 131, 2)],           # Rt = 4: below dec_gemm_min_b_
    "2+2+2": [(A, 20, 2), (B, 131, 2), (A, 13, 2)],
    "8+8": [(B, 131, 8), (A, 20, 8)],           # Rt = 16 = max_batch
    "5+1+3": [(A, 17, 5), (B, 100, 1), (A, 20, 3)],
}


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layouts_and_every_corruption(engine, name, sampled):
    """(the random-init model's greedy token hardly varies, so every layout also runs sampled, each sequence
    with its own seed: there the rows' tokens differ and a token from the wrong row or segment would show)"""
    eng, cfg, donors = engine
    V = cfg.vocab_size
    seqs = [Seq(donors, d, p, W[i], r) for i, (d, p, r) in enumerate(LAYOUTS[name])]
    for i, q in enumerate(seqs):
        if sampled:
            q.kw = dict(temperature=0.9, top_k=50, top_p=0.95, seed=100 + i)
        build_chain(eng, q, 5)
    toks = [q.chain for q in seqs]
    full = compare(eng, seqs, toks)
    assert sum(a for a, _ in full) >= 1     # (the chains are not all rejected: the cases below mean something)
    for s, q in enumerate(seqs):
        for j in range(q.rows - 1):          # draft j of sequence s wrong
            bad = [list(t) for t in toks]
            bad[s][j + 1] = (bad[s][j + 1] + 1) % V
            got = compare(eng, seqs, bad)
            for t in range(len(seqs)):
                if t != s:
                    assert got[t] == full[t]                           # the others: identical
            n = min(j, full[s][0])
            assert got[s] == (n, full[s][1][:n + 1])                   # that segment stops there


def test_sampled_rows_draw_what_decode_draws(engine):
    """temperature > 0, each sequence its own parameters and seed: the RNG is keyed (seed, position)"""
    eng, cfg, donors = engine
    seqs = [Seq(donors, A, 20, W[0], 5), Seq(donors, B, 131, W[1], 4), Seq(donors, A, 15, W[2], 1)]
    seqs[0].kw = dict(temperature=0.8, top_k=40, top_p=0.9, seed=1234567)
    seqs[1].kw = dict(temperature=1.1, top_k=0, top_p=1.0, seed=42)
    seqs[2].kw = dict(temperature=0.6, top_k=10, top_p=0.95, seed=777)
    for q in seqs:
        build_chain(eng, q, 5)
    got = compare(eng, seqs, [q.chain for q in seqs])
    compare(eng, seqs, [seqs[0].chain[:2] + [FILL] * 3, seqs[1].chain, seqs[2].chain])
    seqs[1].kw = dict(seqs[1].kw, seed=43)   # another seed on one sequence changes that sequence alone
    other = compare(eng, seqs, [q.chain for q in seqs])
    assert other[0] == got[0] and other[2] == got[2] and other[1] != got[1]


def test_fp8_kv():
    eng, cfg, donors = make(kv_dtype="fp8")
    seqs = layout(eng, donors, [(A, 20, 4), (B, 131, 3)])
    toks = [q.chain for q in seqs]
    full = compare(eng, seqs, toks)
    bad = [list(t) for t in toks]
    bad[0][2] = (bad[0][2] + 1) % cfg.vocab_size
    got = compare(eng, seqs, bad)
    assert got[1] == full[1] and got[0][0] == min(1, full[0][0])


def test_block_boundary_and_shared_prefix(engine):
    """sequence 0 runs rows 125..132 of a slot copied from donor B, across the 128-token KV block, while donor B
    and a second sequence (B's first 131 tokens: block 0 shared with the donor) hold the same prefix; the donor's
    next decode gives the logits it gave before"""
    eng, cfg, donors = engine
    eng.copy_slot(B, 5, 131)
    eng.decode([5], [donors[B][1]], [131])
    ref = np.asarray(eng.last_logits(1)).copy()
    seqs = layout(eng, donors, [(B, 125, 8), (B, 131, 3)])
    compare(eng, seqs, [q.chain for q in seqs])
    call_multi(eng, seqs, [q.chain for q in seqs])
    t0, t1, td = eng.block_table(seqs[0].slot), eng.block_table(seqs[1].slot), eng.block_table(B)
    m0 = [b for b in t0 if b >= 0]
    assert len(m0) == 2 and not set(m0) & set(td)      # a partial block is copied, the new one is its own
    assert t1[0] == td[0] and t1[1] != td[1] and t1[1] >= 0   # block 0 shared, the written block un-shared
    eng.copy_slot(B, 5, 131)
    eng.decode([5], [donors[B][1]], [131])
    assert np.array_equal(bits(ref), bits(eng.last_logits(1)))


def test_rt_32():
    eng, cfg, donors = make(max_batch=32)
    spec = [(A, 20, 8), (B, 131, 8), (A, 11, 8), (B, 77, 8)]
    seqs = [Seq(donors, d, p, W[i], r) for i, (d, p, r) in enumerate(spec)]
    for q in seqs:   # no spare slot: a chain is built in the sequence's own work slot
        build_chain(eng, q, q.slot)
    toks = [q.chain for q in seqs]
    full = compare(eng, seqs, toks)
    assert sum(a for a, _ in full) >= 1
    bad = [list(t) for t in toks]
    bad[3][5] = (bad[3][5] + 1) % cfg.vocab_size
    got = compare(eng, seqs, bad)
    assert got[:3] == full[:3] and got[3][0] == min(4, full[3][0])
    with pytest.raises(RuntimeError):   # 33 rows: over SPEC_MULTI_MAX_ROWS, with max_batch 32
        eng.spec_decode_multi([0, 1, 2, 3, 4], toks + [[5]], [20, 131, 11, 77, 3])


def test_pipelined_step_continues_from_the_device_tokens(engine):
    """after the call the step state is S rows whose tokens are on the device: decode_submit(tokens = {}) with
    B = S returns what a host-fed decode at the advanced positions returns on twins"""
    eng, cfg, donors = engine
    V = cfg.vocab_size
    seqs = layout(eng, donors, [(A, 20, 5), (B, 131, 3)], spare=4)
    c0, c1 = seqs[0].chain, seqs[1].chain
    for toks in ([c0, c1], [c0[:2] + [(c0[2] + 1) % V] + c0[3:], c1], [c0, [c1[0], (c1[1] + 1) % V, c1[2]]]):
        res = call_multi(eng, seqs, toks)
        slots = [q.slot for q in seqs]
        nxt = [q.pos0 + a + 1 for q, (a, _) in zip(seqs, res)]
        for q, tw, n in zip(seqs, (4, 5), nxt):
            eng.copy_slot(q.slot, tw, n)
        eng.decode_submit(slots, [], nxt)
        eng.decode_sample()
        got = [int(t) for t in eng.decode_collect()]
        lg = np.asarray(eng.last_logits(2)).copy()
        want = [int(t) for t in eng.decode([4, 5], [o[-1] for _, o in res], nxt)]
        assert got == want
        assert np.array_equal(bits(lg), bits(eng.last_logits(2)))
        for s, (a, o) in enumerate(res):   # row s's history: the emitted tokens, then the pipelined step's
            h = eng.decode_loop_history(2, seqs[s].pos0 + 1, a + 2)[s * (a + 2):(s + 1) * (a + 2)]
            assert h == o + [got[s]]


def test_refusals_change_nothing(engine):
    eng, cfg, donors = engine
    V, ctx = cfg.vocab_size, 256
    ta = donors[A][1]
    mb = (V + 7) // 8

    def plain():
        eng.copy_slot(A, W[0], 20)
        tok = int(eng.decode([W[0]], [ta], [20])[0])
        return tok, np.asarray(eng.last_logits(1)).copy()

    before = plain()
    ok = dict(slots=[W[0], W[1]], tokens=[[ta, 5, 6], [ta, 8]], pos0=[20, 20])
    eng.copy_slot(A, W[0], 20)
    eng.copy_slot(A, W[1], 20)
    eng.spec_decode_multi(**ok)                                    # (the base call is served)
    refused = [
        dict(slots=[], tokens=[], pos0=[]),                                             # S = 0
        dict(slots=list(range(9)), tokens=[[ta]] * 9, pos0=[20] * 9),                   # S = 9
        dict(ok, tokens=[[ta] * 9, [ta]]),                                              # a segment of 9 rows
        dict(ok, tokens=[[ta, 5], []]),                                                 # an empty segment
        dict(slots=[W[0], W[1], W[2]], tokens=[[ta] * 8, [ta] * 8, [ta]], pos0=[20] * 3),   # Rt = 17 > max_batch
        dict(ok, slots=[W[0], W[0]]),                                                   # a slot named twice
        dict(ok, slots=[W[0], 99]),                                                     # a bad slot
        dict(ok, slots=[-1, W[1]]),
        dict(ok, pos0=[20, ctx - 1]),                                                   # pos0 + rows > max_ctx
        dict(ok, tokens=[[ta, V], [ta, 8]]),                                            # a token out of range
        dict(ok, masks=b"\xff" * (4 * mb)),                                             # masks for 4 of 5 rows
        dict(ok, temperature=[0.5]),                                                    # parameters for one sequence
    ]
    for kw in refused:
        with pytest.raises(RuntimeError):
            eng.spec_decode_multi(**kw)
        after = plain()
        assert after[0] == before[0] and np.array_equal(bits(after[1]), bits(before[1])), kw
    eng.copy_slot(A, 5, 20)
    eng.decode_submit([5], [ta], [20])
    eng.decode_sample()
    with pytest.raises(RuntimeError):
        eng.spec_decode_multi(**ok)                                # a pipelined step in flight
    eng.decode_collect()
    after = plain()
    assert after[0] == before[0] and np.array_equal(bits(after[1]), bits(before[1]))


def test_staged_processors_and_logprobs(engine):
    """processors and top_logprobs staged for Rt rows: decode()'s contract, decode()'s results"""
    eng, cfg, donors = engine
    seqs = layout(eng, donors, [(A, 20, 4), (B, 131, 1), (A, 16, 2)])
    for q, sd in zip(seqs, (99, 5, 31)):
        q.kw = dict(temperature=0.7, top_k=20, top_p=0.9, seed=sd)
    toks = [q.chain for q in seqs]
    Rt = sum(len(t) for t in toks)
    windows = [donors[q.donor][0][:q.pos0][-6:] + t[:i + 1] for q, t in zip(seqs, toks) for i in range(len(t))]
    topn = [3, 3, -1, 2, 5, 0, 3]

    def stage():
        eng.set_sample_processors([0.05] * Rt, [1.3] * Rt, [0.2] * Rt, [0.1] * Rt, windows)
        eng.set_logprobs(topn)

    stage()
    got = call_multi(eng, seqs, toks)
    glp = eng.last_logprobs()
    assert len(glp) == 3 and glp[0].shape == (Rt,)
    stage()
    dec, flat = call_decode(eng, seqs, toks)
    wlp = eng.last_logprobs()
    assert got == M.accept(flat, dec, M.segments([len(t) for t in toks]))
    for a, b in zip(glp, wlp):
        assert np.array_equal(bits(a), bits(b))
    # one shot: nothing is staged for the next launch, and a staging for other rows is refused
    call_multi(eng, seqs, toks)
    assert len(eng.last_logprobs()) == 0
    eng.set_logprobs([3] * (Rt - 1))
    with pytest.raises(RuntimeError):
        call_multi(eng, seqs, toks)
