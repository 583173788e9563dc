"""Engine.spec_decode on the device: one request's R consecutive positions as the R rows of one decode step,
the sampler on every row, the accept kernel behind it (csrc/engine.hip, csrc/kernels/spec_accept.hip).

The reference is the engine's own decode() on a copy_slot twin with the same rows -- ([slot] * R, tokens,
pos0 .. pos0 + R - 1) -- and the accept rule in plain Python (tests/spec_oracle.py): the same batched kernels
run on both sides, the weights are Q4_K_M (no float atomics in those GEMVs), so tokens, logits and logprobs
are compared for equality, bit for bit.  A fully accepted draft (a "chain") is built with spec_decode itself:
R - 1 calls on fresh twins, each extending the draft by the token the call before returned, so every chain
token comes from the R-row kernels it is later verified with.  R = 2 and 4 run the LDS GEMV engine's rows,
5 and 8 the ring-GEMM rows (the engine's dec_gemm_min_b_ is 5).
"""
import numpy as np
import pytest

import spec_oracle as O

pytestmark = pytest.mark.gpu

PROMPT = [1] + [(37 * i + 11) % 1000 + 3 for i in range(11)]   # 12 tokens: pos0 = 12
FILL = 7
DONOR, WORK, TWIN, AUX = 0, 1, 2, 3


def make(kv_dtype="bf16", max_ctx=256):
    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset("test-mistral-shape")
    eng = random_engine(cfg, "Q4_K_M", seed=5, max_ctx=max_ctx, max_slots=4, max_batch=8, kv_dtype=kv_dtype)
    return eng, cfg


@pytest.fixture(scope="module")
def engine():
    return make()


def prefill_donor(eng, prompt=PROMPT):
    lg = np.asarray(eng.prefill(DONOR, prompt, 0, True))
    return int(lg.argmax())


def twin(eng, dst, n):
    eng.copy_slot(DONOR, dst, n)
    return dst


def build_chain(eng, t0, pos0, R, **kw):
    """c[0..R-1]: c[0] = t0 and c[i + 1] = the token row i samples when the drafts before it are right"""
    c = [t0]
    for j in range(R - 1):
        toks = c + [FILL] * (R - len(c))
        acc, out = eng.spec_decode(twin(eng, WORK, pos0), toks, pos0, **kw)
        assert acc >= j and len(out) == acc + 1
        c.append(int(out[j]))
    return c


@pytest.mark.parametrize("R", [2, 4, 5, 8])
def test_chain_accepts_and_every_corruption_stops_there(engine, R):
    eng, cfg = engine
    V, pos0 = cfg.vocab_size, len(PROMPT)
    t0 = prefill_donor(eng)
    c = build_chain(eng, t0, pos0, R)
    acc, out = eng.spec_decode(twin(eng, WORK, pos0), c, pos0)
    assert acc == R - 1 and list(out[:R - 1]) == c[1:]                         # (a) the whole chain
    full = [int(t) for t in out]
    lg_spec = np.asarray(eng.last_logits(R))
    # (b) the same rows through decode() on a twin: tokens row by row, logits bit for bit
    dec = eng.decode([twin(eng, TWIN, pos0)] * R, c, list(range(pos0, pos0 + R)))
    assert [int(t) for t in dec] == full
    assert np.array_equal(lg_spec.view(np.uint32), np.asarray(eng.last_logits(R)).view(np.uint32))
    for j in range(R - 1):                                                     # (a) draft j wrong
        bad = list(c)
        bad[j + 1] = (c[j + 1] + 1) % V
        acc, out = eng.spec_decode(twin(eng, WORK, pos0), bad, pos0)
        assert acc == j and [int(t) for t in out] == full[:j + 1]


def test_rejected_tail_leaves_nothing_behind(engine):
    """(c) two twins, the same accepted prefix, different junk behind the mismatch: three B = 1 steps later
    their logits are still equal bit for bit -- nothing reads the rejected rows' K/V"""
    eng, cfg = engine
    V, pos0, R = cfg.vocab_size, len(PROMPT), 8
    t0 = prefill_donor(eng)
    c8 = build_chain(eng, t0, pos0, R)      # (from the R-row kernels the two calls below run)
    c = c8[:3]                              # c1, c2 right; draft 2 (row 3's input) is not c3 on either twin
    tails = [[(c8[3] + 1 + k) % V for k in range(R - 3)], [(c8[3] + 400 + 3 * k) % V for k in range(R - 3)]]
    res = []
    for slot, tail in zip((WORK, TWIN), tails):
        acc, out = eng.spec_decode(twin(eng, slot, pos0), c + [(int(x)) for x in tail], pos0)
        res.append((acc, [int(t) for t in out]))
    assert res[0] == res[1] and res[0][0] == 2
    tok, pos = res[0][1][-1], pos0 + 3
    for step in range(3):
        a = eng.decode([WORK], [tok], [pos + step])
        la = np.asarray(eng.last_logits(1)).copy()
        b = eng.decode([TWIN], [tok], [pos + step])
        lb = np.asarray(eng.last_logits(1))
        assert int(a[0]) == int(b[0]) and np.array_equal(la.view(np.uint32), lb.view(np.uint32)), step
        tok = int(a[0])


def test_block_boundary_and_shared_donor(engine):
    """(d) pos0 = 125, R = 8: the rows cross the 128-token KV block on a slot copied from a donor; the donor's
    next decode gives the logits it gave before it was shared"""
    eng, cfg = engine
    pos0, R = 125, 8
    prompt = [1] + [(53 * i + 29) % 1000 + 3 for i in range(pos0 - 1)]
    t0 = prefill_donor(eng, prompt)
    eng.decode([DONOR], [t0], [pos0])
    ref = np.asarray(eng.last_logits(1)).copy()
    c = build_chain(eng, t0, pos0, R)
    acc, out = eng.spec_decode(twin(eng, WORK, pos0), c, pos0)
    assert acc == R - 1
    mapped = [b for b in eng.block_table(WORK) if b >= 0]
    assert len(mapped) == 2 and not set(mapped) & set(eng.block_table(DONOR))
    lg = np.asarray(eng.last_logits(R)).copy()
    dec = eng.decode([twin(eng, TWIN, pos0)] * R, c, list(range(pos0, pos0 + R)))
    assert [int(t) for t in dec] == [int(t) for t in out]
    assert np.array_equal(lg.view(np.uint32), np.asarray(eng.last_logits(R)).view(np.uint32))
    eng.decode([DONOR], [t0], [pos0])
    assert np.array_equal(ref.view(np.uint32), np.asarray(eng.last_logits(1)).view(np.uint32))


def test_refusals_change_nothing(engine):
    """(e) every refusal throws before any state changes: the same plain decode before and after"""
    eng, cfg = engine
    V, pos0, ctx = cfg.vocab_size, len(PROMPT), 256
    t0 = prefill_donor(eng)
    before = eng.decode([twin(eng, WORK, pos0)], [t0], [pos0])
    lb = np.asarray(eng.last_logits(1)).copy()
    mb = (V + 7) // 8
    with pytest.raises(RuntimeError):
        eng.spec_decode(WORK, [t0] * 4, ctx - 3)              # pos0 + R > max_ctx
    eng.spec_decode(twin(eng, AUX, pos0), [t0] * 2, pos0)     # (R = 2 is served)
    with pytest.raises(RuntimeError):
        eng.spec_decode(WORK, [t0], pos0)                     # R = 1
    with pytest.raises(RuntimeError):
        eng.spec_decode(WORK, [t0] * 9, pos0)                 # R = 9
    with pytest.raises(RuntimeError):
        eng.spec_decode(WORK, [t0, V], pos0)                  # a token out of range
    with pytest.raises(RuntimeError):
        eng.spec_decode(WORK, [t0] * 3, pos0, masks=b"\xff" * (2 * mb))   # masks for 2 rows
    eng.decode_submit([twin(eng, AUX, pos0)], [t0], [pos0])
    eng.decode_sample()
    with pytest.raises(RuntimeError):
        eng.spec_decode(WORK, [t0] * 3, pos0)                 # a pipelined step in flight
    eng.decode_collect()
    after = eng.decode([twin(eng, WORK, pos0)], [t0], [pos0])
    assert int(before[0]) == int(after[0])
    assert np.array_equal(lb.view(np.uint32), np.asarray(eng.last_logits(1)).view(np.uint32))


def test_sampled_rows_draw_what_decode_draws(engine):
    """(f) temperature 0.8, top-k 40, top-p 0.9, one seed on every row: the RNG is keyed (seed, position)"""
    eng, cfg = engine
    pos0, R, seed = len(PROMPT), 8, 1234567
    t0 = prefill_donor(eng)
    kw = dict(temperature=0.8, top_k=40, top_p=0.9, seed=seed)
    c = build_chain(eng, t0, pos0, R, **kw)
    for toks in (c, c[:3] + [FILL] * (R - 3)):
        acc, out = eng.spec_decode(twin(eng, WORK, pos0), toks, pos0, **kw)
        dec = [int(t) for t in eng.decode([twin(eng, TWIN, pos0)] * R, toks, list(range(pos0, pos0 + R)), [0.8] * R,
                                          [40] * R, 0, b"", [0.9] * R, [seed] * R)]
        n, emitted = O.accept(toks, dec)
        assert (acc, [int(t) for t in out]) == (n, emitted)
    assert acc >= 2
    greedy = build_chain(eng, t0, pos0, R)
    assert greedy != c                                        # (it samples)


def test_fp8_kv_chain():
    """(g) the chain case on an fp8 KV cache"""
    eng, cfg = make(kv_dtype="fp8")
    V, pos0, R = cfg.vocab_size, len(PROMPT), 5
    t0 = prefill_donor(eng)
    c = build_chain(eng, t0, pos0, R)
    acc, out = eng.spec_decode(twin(eng, WORK, pos0), c, pos0)
    assert acc == R - 1 and [int(t) for t in out[:R - 1]] == c[1:]
    full = [int(t) for t in out]
    for j in range(R - 1):
        bad = list(c)
        bad[j + 1] = (c[j + 1] + 1) % V
        acc, out = eng.spec_decode(twin(eng, WORK, pos0), bad, pos0)
        assert acc == j and [int(t) for t in out] == full[:j + 1]


def test_staged_processors_and_logprobs(engine):
    """(h) processors and top_logprobs = 3 staged for R rows: decode()'s contract, decode()'s results"""
    eng, cfg = engine
    V, pos0, R = cfg.vocab_size, len(PROMPT), 4
    t0 = prefill_donor(eng)
    c = build_chain(eng, t0, pos0, R)
    windows = [PROMPT[-6:] + c[:i + 1] for i in range(R)]

    def stage():
        eng.set_sample_processors([0.05] * R, [1.3] * R, [0.2] * R, [0.1] * R, windows)
        eng.set_logprobs([3] * R)

    stage()
    acc, out = eng.spec_decode(twin(eng, WORK, pos0), c, pos0, temperature=0.7, top_k=20, top_p=0.9, seed=99)
    got = eng.last_logprobs()
    assert len(got) == 3 and got[0].shape == (R,)
    stage()
    dec = [int(t) for t in eng.decode([twin(eng, TWIN, pos0)] * R, c, list(range(pos0, pos0 + R)), [0.7] * R, [20] * R,
                                      0, b"", [0.9] * R, [99] * R)]
    want = eng.last_logprobs()
    n, emitted = O.accept(c, dec)
    assert (acc, [int(t) for t in out]) == (n, emitted)
    # rows behind the accepted ones hold the sampler's tokens on both sides: all R rows compare
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    # one shot: nothing is staged for the next launch, and a staging for other rows is refused
    eng.spec_decode(twin(eng, WORK, pos0), c, pos0)
    assert len(eng.last_logprobs()) == 0
    eng.set_logprobs([3] * (R - 1))
    with pytest.raises(RuntimeError):
        eng.spec_decode(twin(eng, WORK, pos0), c, pos0)


def test_pipelined_step_continues_from_the_device_token(engine):
    """(i) after spec_decode the step state is one row whose token is on the device"""
    eng, cfg = engine
    V, pos0, R = cfg.vocab_size, len(PROMPT), 5
    t0 = prefill_donor(eng)
    c = build_chain(eng, t0, pos0, R)
    for toks in (c, c[:2] + [(c[2] + 1) % V] + c[3:]):
        acc, out = eng.spec_decode(twin(eng, WORK, pos0), toks, pos0)
        nxt = pos0 + acc + 1
        eng.copy_slot(WORK, TWIN, nxt)
        eng.decode_submit([WORK], [], [nxt])
        eng.decode_sample()
        got = int(eng.decode_collect()[0])
        lg = np.asarray(eng.last_logits(1)).copy()
        want = int(eng.decode([TWIN], [int(out[-1])], [nxt])[0])
        assert got == want
        assert np.array_equal(lg.view(np.uint32), np.asarray(eng.last_logits(1)).view(np.uint32))
        assert eng.decode_loop_history(1, pos0 + 1, acc + 2) == [int(t) for t in out] + [got]
