"""Engine.shift_context (csrc/kernels/kv_shift.hip) against tests/context_shift_oracle.py: prefill random tokens,
snapshot the slot with kv_read, shift, read again and compare with the oracle applied to the snapshot.

  * kept rows and every V row: bit for bit;
  * a moved bf16 K element: within 2^-8 * hypot(x, y) of the float64 result, (x, y) its stored pair -- half a
    bf16 ulp is at most 2^-9 of the magnitude, the factor 2 covers the fp32 arithmetic;
  * a moved fp8 K element: within 2^-3 * hypot + 2^-9 * scale (3 mantissa bits, and the subnormal step), after the
    test has asserted hypot < 448 * scale for every pair, so that saturation cannot hide in the bound;
  * block_table and kv_blocks_free equal the host arithmetic, the null block stays all zero;
  * a shared prefix is never written through; every refusal leaves tables, pool and bytes as they were.

test-small (3 layers, 2 KV heads, head_dim 64), max_ctx 512 = 4 blocks per slot; ROPE_NORM from the synthetic file
of test_kv_paging_gpu (seed 7, fp8 scales 0.05 / 0.02), ROPE_NEOX from the same weights written as arch qwen2 (the
architecture is what selects the pairing at load).
One tile of the kernel is 128 (bf16) / 256 (fp8) positions at this head size.

Measured on the MI355X: the worst moved bf16 element lies at 0.98 .. 0.99 of its bound (half a bf16 ulp reaches
2^-8 of an element that sits just above a power of two and carries the pair's whole magnitude), the worst fp8
element at 0.47 of its bound.
"""
import dataclasses

import numpy as np
import pytest

import context_shift_oracle as C
import kv_paging_oracle as P

pytestmark = pytest.mark.gpu

MAX_CTX, SLOTS, BATCH = 512, 4, 4
KVS = ["bf16", "fp8_e4m3"]
ROPES = ["norm", "neox"]

# (n, n_keep, n_discard)
CASES = [
    (500, 0, 1),        # n_discard below any tile
    (500, 5, 130),      # unaligned, crosses blocks
    (384, 128, 128),    # fully aligned
    (300, 200, 99),     # keep and tail inside one block
    (512, 1, 255),      # a full window with llama.cpp's numbers: (512 - 1) // 2
    (200, 64, 136),     # empty tail
]


def fp8_scales(n_layers):
    return [0.05 if i % 2 == 0 else 0.02 for i in range(2 * n_layers)]


@pytest.fixture(scope="module")
def model_file(tmp_path_factory):
    """{rope: path}"""
    from aios_amd.models.config import ROPE_NEOX, get_preset
    from aios_amd.models.synthetic import write_synthetic_gguf

    d = tmp_path_factory.mktemp("kvshift")
    small = get_preset("test-small")
    neox = dataclasses.replace(small, arch="qwen2", rope_mode=ROPE_NEOX)
    return {"norm": write_synthetic_gguf(str(d / "small_Q4_K_M.gguf"), small, "Q4_K_M", seed=7),
            "neox": write_synthetic_gguf(str(d / "small_neox_Q4_K_M.gguf"), neox, "Q4_K_M", seed=7)}


def make_engine(paths, kv, rope):
    from aios_amd.runtime.loader import load_engine

    eng, cfg, _ = load_engine(paths[rope], max_ctx=MAX_CTX, max_slots=SLOTS, max_batch=BATCH, act_q8=False, kv_dtype=kv)
    if kv != "bf16":
        eng.set_kv_scales(fp8_scales(cfg.n_layers))
    assert eng.config.rope_neox == (1 if rope == "neox" else 0)
    return eng, cfg


_ENGINES = {}


@pytest.fixture
def engine(model_file, request):
    kv, rope = request.param
    if (kv, rope) not in _ENGINES:
        _ENGINES[(kv, rope)] = make_engine(model_file, kv, rope)
    eng, cfg = _ENGINES[(kv, rope)]
    for s in range(SLOTS):
        eng.release_slot(s)
    assert eng.kv_blocks_free == eng.kv_blocks_total == 16
    return eng, cfg, kv, rope


ENGINES = pytest.mark.parametrize("engine", [(kv, r) for kv in KVS for r in ROPES], indirect=True,
                                  ids=[f"{kv}-{r}" for kv in KVS for r in ROPES])


def rand_tokens(cfg, seed, n):
    return [1] + [int(t) for t in np.random.default_rng(seed).integers(3, cfg.vocab_size, n - 1)]


def read(eng, cfg, kv, slot, n):
    raw = np.frombuffer(eng.kv_read(slot, n), dtype=np.uint16 if kv == "bf16" else np.uint8)
    return raw.reshape(cfg.n_layers, 2, cfg.n_kv_heads, n, cfg.head_dim)


def decode_k(cfg, kv, bits):
    """[layer][head][token][hd] float64 of the K half of a snapshot"""
    if kv == "bf16":
        return C.bf16_decode(bits[:, 0])
    sc = fp8_scales(cfg.n_layers)
    return np.stack([C.fp8_decode(bits[l, 0], sc[2 * l]) for l in range(cfg.n_layers)])


def state(eng):
    return [eng.block_table(s) for s in range(SLOTS)], eng.kv_blocks_free


def null_block_is_zero(eng):
    return not np.frombuffer(eng.kv_read_block(eng.kv_blocks_total), dtype=np.uint8).any()


def shift_and_check(eng, cfg, kv, rope, slot, n, keep, d, label):
    """snapshot, shift, compare with the oracle; returns the new length"""
    neox = rope == "neox"
    before = read(eng, cfg, kv, slot, n)
    tables, free = state(eng)
    k0 = decode_k(cfg, kv, before)
    hyp = C.pair_hypot(k0, neox)
    if kv != "bf16":  # the precondition of the fp8 bound: no pair can saturate on the way back
        for l in range(cfg.n_layers):
            lim = 448.0 * fp8_scales(cfg.n_layers)[2 * l]
            assert hyp[l].max() < lim, f"{label}: layer {l} holds a pair of magnitude {hyp[l].max()} >= {lim}"
    n_new = eng.shift_context(slot, n, keep, d)
    assert n_new == n - d
    # bookkeeping: this slot's blocks are private here, so the table only loses the entries above the new length
    want = list(tables[slot])
    gone = 0
    for j in range((n_new + C.KV_BLOCK - 1) // C.KV_BLOCK, len(want)):
        gone += want[j] >= 0
        want[j] = -1
    assert eng.block_table(slot) == want, f"{label}: table {eng.block_table(slot)}, expected {want}"
    assert eng.kv_blocks_free == free + gone
    for s in range(SLOTS):
        if s != slot:
            assert eng.block_table(s) == tables[s]
    dev = [int(b) for b in eng.kv_device_tables(0)]
    assert dev == [eng.kv_blocks_total if b < 0 else b for s in range(SLOTS) for b in eng.block_table(s)]
    after = read(eng, cfg, kv, slot, n_new)
    src = keep + d
    # V rows and kept rows: the same bytes
    assert np.array_equal(after[:, 1, :, :keep], before[:, 1, :, :keep]), f"{label}: a kept V row changed"
    assert np.array_equal(after[:, 1, :, keep:], before[:, 1, :, src:]), f"{label}: a moved V row is not its source's bytes"
    assert np.array_equal(after[:, 0, :, :keep], before[:, 0, :, :keep]), f"{label}: a kept K row changed"
    if n_new > keep:
        want_k, _, moved = C.shift_kv(k0, k0, keep, d, cfg.rope_theta, neox)
        got_k = decode_k(cfg, kv, after)
        err = np.abs(got_k - want_k)[:, :, keep:]
        h = hyp[:, :, src:]
        if kv == "bf16":
            bound = 2.0 ** -8 * h
        else:
            sc = np.asarray(fp8_scales(cfg.n_layers)[0::2]).reshape(-1, 1, 1, 1)
            bound = 2.0 ** -3 * h * 1 + 2.0 ** -9 * sc
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{label}: worst moved-K error {worst:.3f} of the bound, {int(moved.sum())} rows moved")
        assert np.isfinite(got_k).all() and (err <= bound).all(), f"{label}: moved K off by {worst} of the bound"
        # and the rotation was applied at all: with hypot > 0 a row rotated by d differs from its source
        assert (after[:, 0, :, keep:] != before[:, 0, :, src:]).any()
    assert null_block_is_zero(eng), f"{label}: the null block was written"
    return n_new


@ENGINES
@pytest.mark.parametrize("case", CASES, ids=[f"n{n}-keep{k}-discard{d}" for n, k, d in CASES])
def test_shift_matches_oracle(engine, case):
    eng, cfg, kv, rope = engine
    n, keep, d = case
    eng.prefill(0, rand_tokens(cfg, 11, n), 0, False)
    shift_and_check(eng, cfg, kv, rope, 0, n, keep, d, f"[{kv}, {rope}, n {n}, keep {keep}, discard {d}]")


@ENGINES
def test_two_shifts_in_a_row(engine):
    eng, cfg, kv, rope = engine
    eng.prefill(1, rand_tokens(cfg, 12, 500), 0, False)
    n = shift_and_check(eng, cfg, kv, rope, 1, 500, 5, 130, f"[{kv}, {rope}, first]")
    n = shift_and_check(eng, cfg, kv, rope, 1, n, 40, 100, f"[{kv}, {rope}, second]")
    assert n == 270 and eng.block_table(1)[3] == -1 and eng.block_table(1)[2] >= 0
    # the slot goes on from there: a decode step at the new length writes one more row and moves nothing else
    snap = read(eng, cfg, kv, 1, n)
    eng.decode([1], [7], [n])
    now = read(eng, cfg, kv, 1, n + 1)
    assert np.array_equal(now[:, :, :, :n], snap) and (now[:, :, :, n] != 0).any(axis=-1).all()


@ENGINES
def test_shared_prefix_is_not_written_through(model_file, engine):
    _, cfg, kv, rope = engine
    eng, cfg = make_engine(model_file, kv, rope)  # (a fresh free list: the block model runs in lockstep)
    m = P.PagedKV(MAX_CTX, SLOTS)
    eng.prefill(0, rand_tokens(cfg, 13, 300), 0, False)
    m.prefill(0, 0, 300)
    eng.copy_slot(0, 1, 300)
    m.copy_slot(0, 1, 300)
    src = eng.kv_read(0, 300)
    assert eng.kv_read(1, 300) == src and eng.block_table(1)[:2] == eng.block_table(0)[:2]
    dst = read(eng, cfg, kv, 1, 300)
    assert eng.shift_context(1, 300, 100, 100) == 200
    C.shift_blocks(m, 1, 300, 100, 100)
    m.check()
    assert [eng.block_table(s) for s in range(SLOTS)] == [m.block_table(s) for s in range(SLOTS)]
    assert eng.kv_blocks_free == m.blocks_free and len(m.unshared) == 2
    assert eng.kv_read(0, 300) == src, "the shift of dst changed src"
    now = read(eng, cfg, kv, 1, 200)
    assert np.array_equal(now[:, :, :, :100], dst[:, :, :, :100]) and np.array_equal(now[:, 1, :, 100:], dst[:, 1, :, 200:])
    want, _, _ = C.shift_kv(decode_k(cfg, kv, dst), decode_k(cfg, kv, dst), 100, 100, cfg.rope_theta, rope == "neox")
    tol = 2.0 ** -8 if kv == "bf16" else 2.0 ** -3
    h = C.pair_hypot(decode_k(cfg, kv, dst), rope == "neox")[:, :, 200:]
    sub = 0.0 if kv == "bf16" else 2.0 ** -9 * 0.05
    assert (np.abs(decode_k(cfg, kv, now) - want)[:, :, 100:] <= tol * h + sub).all()
    assert null_block_is_zero(eng)


@ENGINES
def test_refusals_change_nothing(engine):
    eng, cfg, kv, rope = engine
    n = 300
    eng.prefill(2, rand_tokens(cfg, 14, n), 0, False)
    tables, free = state(eng)
    snap = eng.kv_read(2, n)
    bad = [(-1, n, 0, 10), (SLOTS, n, 0, 10),            # a bad slot
           (2, 0, 0, 1), (2, MAX_CTX + 1, 0, 10),        # n_tokens outside [1, max_ctx]
           (2, n, -1, 10),                               # n_keep < 0
           (2, n, 10, 0), (2, n, 10, -5),                # n_discard < 1
           (2, n, 200, 101), (2, n, n, 1)]               # n_keep + n_discard > n_tokens
    for args in bad:
        with pytest.raises(RuntimeError):
            eng.shift_context(*args)
        assert state(eng) == (tables, free) and eng.kv_read(2, n) == snap, f"shift_context{args} changed something"
    # a pipelined step in flight: sampled and not yet collected
    eng.decode_submit([2], [5], [n])
    eng.decode_sample(b"")
    tables, free = state(eng)
    snap = eng.kv_read(2, n + 1)
    with pytest.raises(RuntimeError, match="in flight"):
        eng.shift_context(2, n + 1, 0, 10)
    assert state(eng) == (tables, free) and eng.kv_read(2, n + 1) == snap
    eng.decode_collect()
    assert eng.shift_context(2, n + 1, 0, 10) == n - 9   # and afterwards it goes through
    assert null_block_is_zero(eng)


def test_unfinalized_engine_refuses():
    from aios_amd.models.config import get_preset
    from aios_amd.runtime import native

    m = native.require()
    eng = m.Engine(native.engine_config(get_preset("test-small"), max_ctx=MAX_CTX, max_slots=SLOTS, max_batch=BATCH))
    with pytest.raises(RuntimeError, match="not finalized"):
        eng.shift_context(0, 10, 0, 1)
