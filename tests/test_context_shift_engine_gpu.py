"""Decoding after Engine.shift_context, against the reference model on a cache the oracle shifted
(tests/context_shift_oracle.py: shift_reference_cache).

Prefill, a few decode steps (the B = 1 graph is captured), shift, one decode step at the new position: its logits
lie within 2e-2 of the logit scale (TWIN_BOUND of test_kv_paging_gpu) of ReferenceModel.forward on the shifted
cache.  The control is computed on the CPU with the reference alone: the same cache with the rows dropped and K
NOT re-rotated misses that bound on this input, so the input sees a missing rotation.  For that the synthetic
test-small file scales attn_q by 4 and attn_k by 2 (plain 0.02-std weights attend almost uniformly: the control
then differs by a third of the bound).  Also: a B = 2 step with one shifted and one untouched slot (the row
table's refresh under a replayed graph), and a second shift followed by another step.
"""
import dataclasses

import numpy as np
import pytest

import context_shift_oracle as C

pytestmark = pytest.mark.gpu

MAX_CTX, SLOTS, BATCH = 512, 4, 4
TWIN_BOUND = 2e-2


def fp8_scales(n_layers):
    return [0.05 if i % 2 == 0 else 0.02 for i in range(2 * n_layers)]


@pytest.fixture(scope="module")
def model_files(tmp_path_factory):
    """{rope: path}; ROPE_NEOX is the same weights written as arch qwen2 (the architecture selects the pairing)"""
    from aios_amd.models.config import ROPE_NEOX, get_preset
    from aios_amd.models.synthetic import write_synthetic_gguf

    d = tmp_path_factory.mktemp("ctxshift_engine")
    small = get_preset("test-small")
    scale = {"attn_q.weight": 4.0, "attn_k.weight": 2.0}
    return {"norm": write_synthetic_gguf(str(d / "small_Q4_K_M.gguf"), small, "Q4_K_M", seed=7, tensor_scale=scale),
            "neox": write_synthetic_gguf(str(d / "small_neox_Q4_K_M.gguf"),
                                         dataclasses.replace(small, arch="qwen2", rope_mode=ROPE_NEOX), "Q4_K_M", seed=7,
                                         tensor_scale=scale)}


def close(label, got, want):
    err, bound = float(np.abs(got - want).max()), TWIN_BOUND * max(float(np.abs(want).max()), 1.0)
    print(f"{label}: error {err:.4g}, bound {bound:.4g} ({err / bound:.3f} of it)")
    assert np.isfinite(got).all() and err < bound, f"{label}: error {err}, bound {bound}"


@pytest.mark.parametrize("kv,rope", [("bf16", "norm"), ("fp8_e4m3", "norm"), ("bf16", "neox"), ("fp8_e4m3", "neox")])
def test_decode_after_shift_matches_reference(model_files, kv, rope):
    from aios_amd.models.config import ROPE_NEOX
    from aios_amd.models.reference import ReferenceModel
    from aios_amd.runtime.loader import load_engine

    model_file = model_files[rope]
    eng, cfg, _ = load_engine(model_file, max_ctx=MAX_CTX, max_slots=SLOTS, max_batch=BATCH, act_q8=False, kv_dtype=kv)
    if kv == "bf16":
        ref = ReferenceModel.from_gguf(model_file, kv_bf16=True)
    else:
        eng.set_kv_scales(fp8_scales(cfg.n_layers))
        ref = ReferenceModel.from_gguf(model_file, kv_fp8=True, kv_scales=fp8_scales(cfg.n_layers))
    rng = np.random.default_rng(21)
    toks = [1] + [int(t) for t in rng.integers(3, cfg.vocab_size, 400)]
    other = [1] + [int(t) for t in rng.integers(3, cfg.vocab_size, 150)]
    n0, steps = 300, 4
    N, keep, d = n0 + steps, 5, 130

    # the reference: the cache of the same tokens, shifted by the oracle; and the control without the rotation
    cache = ref.new_cache()
    ref.forward(toks[:N], cache)
    if kv != "bf16":  # the precondition of an fp8 shift (test_kv_shift_gpu): no pair near saturation
        for l in range(cfg.n_layers):
            k = cache["k"][l].numpy().astype(np.float64)
            assert C.pair_hypot(k, rope == "neox").max() < 448.0 * fp8_scales(cfg.n_layers)[2 * l]
    shifted = C.shift_reference_cache(ref, cache, keep, d)
    control = C.shift_reference_cache(ref, cache, keep, d, rotate=False)
    want = ref.forward([toks[N]], shifted)[-1].numpy()
    ctrl = ref.forward([toks[N]], control)[-1].numpy()
    bound = TWIN_BOUND * max(float(np.abs(want).max()), 1.0)
    assert float(np.abs(ctrl - want).max()) >= bound, "this input cannot see a missing rotation"

    assert (ref.cfg.rope_mode == ROPE_NEOX) == (rope == "neox") == bool(eng.config.rope_neox)

    # the engine: prefill, decode steps through the captured B = 1 graph, shift, one step at the new position
    eng.prefill(0, toks[:n0], 0, False)
    for i in range(steps):
        eng.decode([0], [toks[n0 + i]], [n0 + i])
    eng.prefill(1, other[:140], 0, False)
    eng.decode([0, 1], [toks[N], other[140]], [N, 140])      # captures B = 2; row 0's position is written again below
    assert eng.shift_context(0, N, keep, d) == N - d
    eng.decode([0], [toks[N]], [N - d])
    close(f"[{kv}, {rope}] B = 1 step after the shift", np.asarray(eng.last_logits(1)).reshape(-1), want)

    # B = 2: the shifted slot and an untouched one, through the graph replayed with another row table
    want0 = ref.forward([toks[N + 1]], shifted)[-1].numpy()
    oc = ref.new_cache()
    ref.forward(other[:141], oc)
    want1 = ref.forward([other[141]], oc)[-1].numpy()
    eng.decode([0, 1], [toks[N + 1], other[141]], [N - d + 1, 141])
    got = np.asarray(eng.last_logits(2)).reshape(2, -1)
    close(f"[{kv}, {rope}] B = 2, the shifted slot", got[0], want0)
    close(f"[{kv}, {rope}] B = 2, the untouched slot", got[1], want1)

    # a second shift (n_keep grows, the regions nest) and another step
    N2 = shifted["len"]
    assert N2 == N - d + 2
    keep2, d2 = 40, 90
    shifted2 = C.shift_reference_cache(ref, shifted, keep2, d2)
    want2 = ref.forward([toks[N + 2]], shifted2)[-1].numpy()
    assert eng.shift_context(0, N2, keep2, d2) == N2 - d2
    eng.decode([0], [toks[N + 2]], [N2 - d2])
    close(f"[{kv}, {rope}] after the second shift", np.asarray(eng.last_logits(1)).reshape(-1), want2)
