"""Engine.embed_prefill on the GPU: the pooled vector against the engine's own normed rows (sharp), against
the fp32 reference model (wiring), and the call contract.

Sharp: for the same slot and call pattern, pooling=mean must equal the oracle's mean + normalise of the rows
pooling=none returned (embed_oracle.embed(..., normed_rows=True): nothing is normed twice).  The device
pools in fp32, so the bound is measured, not zero: SHARP_TOL is four
times the largest ||mean - oracle(none rows)||_2 seen on an MI355X, SHARP_MEASURED (the case is named at the
constant; profiles/embeddings.txt has every case), and has to stay at or below 1e-4.  What that bound can
see: the test computes, on the CPU from ReferenceModel.hidden, the smallest distance by which leaving any one
row out of the T = 70 prompt's mean moves the reference embedding, prints it, and requires 10 x SHARP_TOL
below it.

Wiring: mean and last against embed_oracle(ReferenceModel.hidden(tokens), output_norm, eps) of the same GGUF,
cosine distance, bound REF_TOL = four times the largest seen (REF_MEASURED).  Condition, from the reference
alone: REF_TOL <= m / 4, m the smallest cosine distance between the reference embedding and the embeddings
under the wrong rules (first token dropped, last token dropped, no norm weight, mean and last swapped).
"""
import numpy as np
import pytest

import embed_oracle as O
from aios_amd.models.config import get_preset

pytestmark = pytest.mark.gpu

NONE, MEAN, LAST = 0, 1, 3
SHARP_MEASURED = 1.808e-07  # test-small, T = 70 as 33 + 37 (mean)
SHARP_TOL = 4 * SHARP_MEASURED
REF_MEASURED = 6.152e-06   # T = 5, mean (the nearest wrong rule there: 4.458e-03)
REF_TOL = 4 * REF_MEASURED
# one prompt under two call patterns (40 rows at once; 10 + 30): other GEMM kernels, so the forwards differ by
# their bf16 / fp32 rounding, not by SHARP_TOL's pooling noise.  Each is within REF_TOL (cosine) of the exact
# embedding, i.e. within an angle sqrt(2 REF_TOL); the two are then within twice that angle of each other,
# a cosine distance of 4 REF_TOL
CROSS_TOL = 4 * REF_TOL

MODELS = ["test-tiny", "test-small", "test-mistral-shape"]
RECIPES = ["Q4_K_M", "BF16"]
T_SINGLE = [1, 4, 5, 32, 33, 65]   # GEMV path, below / at gm_min_rows_, short-fused limit, prefill GEMM, past prefill_rows_
SPLITS = [1, 4, 33, 69]
T_SPLIT = 70


def prompt(cfg, T, seed=21):
    ids = np.random.default_rng(seed).integers(3, cfg.vocab_size, T)
    ids[0] = cfg.bos_id
    return [int(t) for t in ids]


@pytest.fixture(scope="module", params=[(m, r) for m in MODELS for r in RECIPES], ids=lambda p: f"{p[0]}-{p[1]}")
def eng(request):
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset(request.param[0])
    return random_engine(cfg, request.param[1], seed=6, max_ctx=128, max_slots=3, max_batch=2), cfg


def run(e, slot, ids, cuts, pooling):
    """embed_prefill over ids split at `cuts`; the final call's result"""
    edges = [0] + list(cuts) + [len(ids)]
    out = None
    for k in range(len(edges) - 1):
        a, b = edges[k], edges[k + 1]
        out = np.asarray(e.embed_prefill(slot, ids[a:b], a, pooling, b == len(ids)))
        if b != len(ids):
            assert out.size == 0
    return out


def sharp(e, cfg, name, ids, cuts):
    rows = run(e, 1, ids, cuts, NONE)
    assert rows.shape == (len(ids), cfg.d_model) and np.all(np.isfinite(rows)) and e.embed_tokens() == len(ids)
    mean = run(e, 1, ids, cuts, MEAN)
    last = run(e, 1, ids, cuts, LAST)
    assert mean.shape == last.shape == (cfg.d_model,)
    assert abs(np.linalg.norm(mean.astype(np.float64)) - 1) < 1e-5 and abs(np.linalg.norm(last.astype(np.float64)) - 1) < 1e-5
    dm = float(np.linalg.norm(mean - O.embed(rows, pooling="mean", normed_rows=True)))
    dl = float(np.linalg.norm(last - O.embed(rows, pooling="last", normed_rows=True)))
    print(f"embed engine {name}: ||mean - oracle(none rows)|| = {dm:.3e}, ||last - oracle(none rows)|| = {dl:.3e}")
    assert dm <= SHARP_TOL and dl <= SHARP_TOL, f"{name}: {dm:.3e} / {dl:.3e} above {SHARP_TOL:.1e}"


def test_sharp_tolerance_condition():
    """The condition set for the measured bound: at most 1e-4.  An embedding's forward pins the prefill
    GEMM's split to 1 (no float-atomic partial sums), so two runs of it agree bit for bit and what is left is
    the pooling's fp32 rounding against the float64 oracle.  With prefill()'s own split-K plans the same
    comparison measured up to 9.3e-05 on the BF16 engines (profiles/embeddings.txt)."""
    assert SHARP_TOL <= 1e-4


@pytest.mark.parametrize("T", T_SINGLE)
def test_single_call_equals_the_pooled_none_rows(eng, T):
    e, cfg = eng
    sharp(e, cfg, f"{cfg.name} T={T}", prompt(cfg, T), [])


@pytest.mark.parametrize("a", SPLITS)
def test_two_calls_equal_the_pooled_none_rows(eng, a):
    e, cfg = eng
    sharp(e, cfg, f"{cfg.name} T={T_SPLIT} a={a}", prompt(cfg, T_SPLIT), [a])


@pytest.mark.parametrize("T,cuts", [(5, []), (32, []), (T_SPLIT, [33])])
def test_the_same_prompt_twice_gives_the_same_bytes(eng, T, cuts):
    # From gm_min_rows_ = 5 rows a chunk goes through the GEMMs: the ring / skinny ones sum their split in a
    # fixed order, the prefill GEMM (33 + 37 rows) runs its plan without fp32-atomic partials.  Shorter
    # prompts take the GEMV path, whose bf16 kernels add row partials with LDS float atomics: measured NOT
    # byte-reproducible at T = 1, 3, 4 on the BF16 engines (profiles/embeddings.txt), and not claimed.
    e, cfg = eng
    ids = prompt(cfg, T)
    for pooling in (MEAN, NONE, LAST):
        one, two = run(e, 2, ids, cuts, pooling), run(e, 2, ids, cuts, pooling)
        assert one.tobytes() == two.tobytes(), f"{cfg.name} pooling {pooling}: two runs differ"


def test_fp8_kv_engine():
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset("test-small")
    e = random_engine(cfg, "Q4_K_M", seed=6, max_ctx=128, max_slots=2, max_batch=2, kv_dtype="fp8")
    assert e.kv_fp8
    sharp(e, cfg, "test-small fp8 KV T=70 a=33", prompt(cfg, T_SPLIT), [33])


# ---- the fp32 reference ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_setup(tmp_path_factory):
    from aios_amd.models.reference import ReferenceModel
    from aios_amd.models.synthetic import write_synthetic_gguf
    from aios_amd.runtime.loader import load_engine

    cfg = get_preset("test-small")
    path = write_synthetic_gguf(str(tmp_path_factory.mktemp("emb") / "small.gguf"), cfg, "Q4_K_M", seed=9)
    e, _, _ = load_engine(path, max_ctx=128, max_slots=2, max_batch=2)
    ref = ReferenceModel.from_gguf(path, kv_bf16=True, act_q8=True)
    return e, ref, cfg


def cosd(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def test_dropping_a_row_is_visible_to_the_sharp_bound(ref_setup):
    _, ref, cfg = ref_setup
    ids = prompt(cfg, T_SPLIT)
    x = ref.hidden(ids).double().numpy()
    g = ref.w["output_norm.weight"].double().numpy()
    full = O.embed(x, g, cfg.norm_eps, "mean")
    least = min(float(np.linalg.norm(O.embed(np.delete(x, i, axis=0), g, cfg.norm_eps, "mean") - full))
                for i in range(T_SPLIT))
    print(f"embed engine: a row left out of the T={T_SPLIT} mean moves the reference embedding by >= {least:.3e} "
          f"(SHARP_TOL {SHARP_TOL:.1e})")
    assert least >= 10 * SHARP_TOL


@pytest.mark.parametrize("T", [3, 5, 33])
def test_against_the_reference_model(ref_setup, T):
    e, ref, cfg = ref_setup
    ids = prompt(cfg, T, seed=40 + T)
    x = ref.hidden(ids).double().numpy()
    g = ref.w["output_norm.weight"].double().numpy()
    eps = cfg.norm_eps
    want = {p: O.embed(x, g, eps, p) for p in ("mean", "last")}
    wrong = {"mean": [O.embed(x[1:], g, eps, "mean"), O.embed(x[:-1], g, eps, "mean"),
                      O.embed(x, np.ones_like(g), eps, "mean"), want["last"]],
             "last": [O.embed(x[:-1], g, eps, "last"), O.embed(x, np.ones_like(g), eps, "last"), want["mean"]]}
    m = min(cosd(want[p], w) for p in want for w in wrong[p])
    got = {"mean": run(e, 0, ids, [], MEAN), "last": run(e, 0, ids, [], LAST)}
    for p in want:
        c = cosd(got[p], want[p])
        print(f"embed engine vs reference T={T} {p}: cosine distance {c:.3e} (nearest wrong rule {m:.3e})")
    assert REF_TOL <= m / 4, f"the wrong rules are not separable: m = {m:.3e}"
    for p in want:
        assert cosd(got[p], want[p]) <= REF_TOL


# ---- contract ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset("test-small")
    return random_engine(cfg, "Q4_K_M", seed=6, max_ctx=128, max_slots=3, max_batch=2), cfg


def greedy(e, slot, first_pos, tok, n):
    out = []
    for i in range(n):
        tok = int(e.decode([slot], [tok], [first_pos + i])[0])
        out.append(tok)
    return out


def test_call_contract(small):
    e, cfg = small
    ids = prompt(cfg, 40)
    assert np.asarray(e.embed_prefill(0, ids[:10], 0, MEAN, False)).size == 0
    for start in (9, 11, 0 + 20):               # repeated, skipped, far off
        with pytest.raises(RuntimeError, match="start_pos"):
            e.embed_prefill(0, ids[start:], start, MEAN, True)
    # (a refused call ran nothing: the state still stands at 10 and the right continuation goes through)
    cont = np.asarray(e.embed_prefill(0, ids[10:], 10, MEAN, True))
    assert cont.shape == (cfg.d_model,) and e.embed_tokens() == 40
    with pytest.raises(RuntimeError, match="pooling"):
        e.embed_prefill(0, ids, 0, 2, True)
    a = np.asarray(e.embed_prefill(0, ids[:10], 0, MEAN, False))
    with pytest.raises(RuntimeError, match="start_pos"):   # another pooling does not continue a mean
        e.embed_prefill(0, ids[10:], 10, NONE, True)
    assert a.size == 0
    # start_pos = 0 resets: the result is the fresh prompt's, whatever was pooled before
    e.embed_prefill(0, prompt(cfg, 17, seed=5), 0, MEAN, False)
    one = np.asarray(e.embed_prefill(0, ids, 0, MEAN, True))
    assert e.embed_tokens() == 40 and cosd(one, cont) <= CROSS_TOL
    two = np.asarray(e.embed_prefill(0, ids, 0, MEAN, True))
    assert one.tobytes() == two.tobytes()
    # the slots' states are separate
    e.embed_prefill(1, ids[:7], 0, MEAN, False)
    e.embed_prefill(2, prompt(cfg, 9, seed=8), 0, MEAN, True)
    assert e.embed_tokens() == 9
    rest = np.asarray(e.embed_prefill(1, ids[7:], 7, MEAN, True))
    assert e.embed_tokens() == 40 and cosd(rest, one) <= CROSS_TOL


def test_none_prompts_on_two_slots_share_one_staging_buffer(small):
    e, cfg = small
    a, b = prompt(cfg, 40, seed=31), prompt(cfg, 12, seed=32)
    alone = np.asarray(e.embed_prefill(0, a, 0, NONE, True))
    e.embed_prefill(0, a[:10], 0, NONE, False)
    rows_b = np.asarray(e.embed_prefill(1, b, 0, NONE, True))     # overwrites rows [0, 12) of the buffer
    assert rows_b.shape == (12, cfg.d_model)
    with pytest.raises(RuntimeError, match="start_pos"):          # slot 0's prompt cannot be continued
        e.embed_prefill(0, a[10:], 10, NONE, True)
    # a mean state on another slot is not touched by it, and the same slot may go on
    e.embed_prefill(2, a[:10], 0, MEAN, False)
    e.embed_prefill(1, b[:5], 0, NONE, False)
    mean = np.asarray(e.embed_prefill(2, a[10:], 10, MEAN, True))
    rest = np.asarray(e.embed_prefill(1, b[5:], 5, NONE, True))
    assert mean.shape == (cfg.d_model,) and rest.shape == (12, cfg.d_model)
    assert cosd(rest.reshape(-1), rows_b.reshape(-1)) <= CROSS_TOL
    again = np.asarray(e.embed_prefill(0, a, 0, NONE, True))      # from position 0 the slot starts over
    assert again.tobytes() == alone.tobytes()


def test_slot_decodes_after_embed_prefill_as_after_prefill(small):
    e, cfg = small
    ids = prompt(cfg, 37, seed=2)
    first = int(np.argmax(np.asarray(e.prefill(0, ids, 0, True))))
    want = greedy(e, 0, len(ids), first, 6)
    e.embed_prefill(1, ids[:20], 0, MEAN, False)
    e.embed_prefill(1, ids[20:], 20, MEAN, True)
    assert greedy(e, 1, len(ids), first, 6) == want
    # one call of 37 rows: the prefill GEMM without split-K, the one place where the embedding's forward is
    # not prefill's own
    e.embed_prefill(2, ids, 0, MEAN, True)
    assert greedy(e, 2, len(ids), first, 6) == want


def test_embed_prefill_between_another_slots_decode_steps(small):
    e, cfg = small
    ids = prompt(cfg, 23, seed=3)
    first = int(np.argmax(np.asarray(e.prefill(0, ids, 0, True))))
    want = greedy(e, 0, len(ids), first, 8)
    first2 = int(np.argmax(np.asarray(e.prefill(0, ids, 0, True))))
    assert first2 == first
    got = greedy(e, 0, len(ids), first, 3)
    v = np.asarray(e.embed_prefill(1, prompt(cfg, 66, seed=4), 0, MEAN, True))
    assert v.shape == (cfg.d_model,)
    got += greedy(e, 0, len(ids) + 3, got[-1], 5)
    assert got == want
