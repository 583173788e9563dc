"""Engine.set_logprobs / last_logprobs on the device: every sampler launch that can carry the logprob launch
(sample_first, decode, the pipelined decode_sample with the next forward already queued, resample), against
the float64 oracle (tests/logprob_oracle.py) applied to that step's logits and the returned tokens; the
tokens themselves must be those of the same run without logprobs.  Presets: test-tiny (V = 512, one slice)
and test-qwen3-shape (V = 151,936, 38 slices)."""
import numpy as np
import pytest

import logprob_oracle as O
from aios_amd.runtime import sampler as host

pytestmark = pytest.mark.gpu

STEPS = 6
PROMPTS = [[1, 30, 40, 50, 60, 70, 80, 90], [1, 31, 41, 51, 61, 71, 81, 91], [1, 32, 42, 52, 62, 72, 82, 92]]
SEEDS = [11, 12, 13]


@pytest.fixture(scope="module", params=["test-tiny", "test-qwen3-shape"])
def engine(request):
    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset(request.param)
    return random_engine(cfg, "Q4_K_M", seed=3, max_ctx=64, max_slots=3, max_batch=3), cfg


def check_rows(got, logits, tokens, top_n, where):
    """last_logprobs() of one launch against the oracle on the launch's logits rows"""
    assert len(got) == 3, f"{where}: no logprobs reported"
    lp, ids, lps = got
    assert lp.shape == (len(tokens),) and ids.shape == lps.shape == (len(tokens), O.MAX_TOP)
    for b, tok in enumerate(tokens):
        x, oid, olp = O.logprobs(logits[b], tok, top_n)
        n = len(oid)
        assert ids[b, :n].tolist() == oid.tolist(), f"{where}: row {b} ids"
        assert np.all(ids[b, n:] == -1) and np.all(np.isneginf(lps[b, n:]))
        err = max(abs(float(lp[b]) - x), float(np.max(np.abs(lps[b, :n] - olp), initial=0.0)))
        print(f"logprobs engine {where} row {b}: max |gpu - oracle| = {err:.3e}")
        assert err <= O.GPU_TOL, f"{where}: row {b} value error {err:.3e} above {O.GPU_TOL:.1e}"


def generate(eng, V, B, temp, top_n, pipelined, ref=None):
    """prefill 8 tokens per row, the first token by sample_first, then STEPS decode steps; top_n None: no
    logprobs staged.  Returns (tokens [1 + STEPS][B], logits [1 + STEPS][B][V]); with logprobs staged every
    launch's report is checked -- against `ref`'s logits where the launch's own are gone (pipelined)."""
    slots, toks, logits = list(range(B)), [], []
    first, rows = [], []
    for s in slots:
        lg = np.asarray(eng.prefill(s, PROMPTS[s], 0, True))
        if top_n is not None:
            eng.set_logprobs([top_n])
        first.append(int(eng.sample_first(7, temp, 0, 1.0, SEEDS[s], b"")))
        if top_n is not None:
            check_rows(eng.last_logprobs(), [lg], [first[-1]], top_n, f"sample_first slot {s}")
        else:
            assert len(eng.last_logprobs()) == 0
        rows.append(lg)
    toks.append(first)
    logits.append(np.stack(rows))
    temps, topk, topp = [temp] * B, [0] * B, [1.0] * B
    for i in range(STEPS):
        pos = [8 + i] * B
        if pipelined:
            if i == 0:
                eng.decode_submit(slots, toks[-1], pos, temps, topk, 0, topp, SEEDS[:B])
            if top_n is not None:
                eng.set_logprobs([top_n] * B)
            eng.decode_sample(b"")
            if i + 1 < STEPS:  # the next step's forward, from the tokens the sampler leaves on the device
                eng.decode_submit(slots, [], [p + 1 for p in pos], temps, topk, 0, topp, SEEDS[:B])
            out = [int(t) for t in eng.decode_collect()]
            # (this step's own logits are gone: the next forward is queued and overwrites them.  `ref` is the
            # plain run of the same prompts, seeds and settings; its logits stand in for this step's only
            # because the forward is deterministic -- the same graph, fixed-order reductions -- and the
            # tokens, asserted equal below step by step, are therefore the same inputs)
            lg = ref[1][i + 1] if ref is not None else None
        else:
            if top_n is not None:
                eng.set_logprobs([top_n] * B)
            out = [int(t) for t in eng.decode(slots, toks[-1], pos, temps, topk, 0, b"", topp, SEEDS[:B])]
            lg = np.asarray(eng.last_logits(B)).reshape(B, V)
        if top_n is not None:
            if ref is not None:
                assert out == ref[0][i + 1], f"step {i}: tokens differ from the plain run"
            check_rows(eng.last_logprobs(), lg, out, top_n, f"step {i}")
        else:
            assert len(eng.last_logprobs()) == 0  # one-shot / nothing staged: nothing reported
        toks.append(out)
        logits.append(lg)
    return toks, logits


@pytest.mark.parametrize("temp", [0.0, 0.8])
@pytest.mark.parametrize("B", [1, 3])
def test_every_launch_matches_the_oracle(engine, B, temp):
    eng, cfg = engine
    V = cfg.vocab_size
    plain = generate(eng, V, B, temp, 20, False)
    bare = generate(eng, V, B, temp, None, False)
    assert bare[0] == plain[0]                       # the same tokens without logprobs
    piped = generate(eng, V, B, temp, 20, True, ref=plain)
    assert piped[0] == plain[0]
    assert generate(eng, V, B, temp, None, True)[0] == plain[0]
    if temp > 0:
        assert len({t for step in plain[0] for t in step}) > 2   # (it samples)


def test_logprobs_with_processors_in_one_step(engine):
    """staged together with a repeat penalty: the token follows the penalised sampler, the logprobs are the
    raw row's"""
    eng, cfg = engine
    V, B = cfg.vocab_size, 2
    toks, _ = generate(eng, V, B, 0.0, None, False)
    seqs = [PROMPTS[b] + [step[b] for step in toks] for b in range(B)]
    last, pos = [s[-1] for s in seqs], [len(s) - 1 for s in seqs]
    wins = [s[-16:] for s in seqs]
    eng.set_sample_processors([0.0] * B, [1.3] * B, [0.0] * B, [0.0] * B, wins)
    eng.set_logprobs([20, 0])
    out = [int(t) for t in eng.decode([0, 1], last, pos, [0.0] * B, [0] * B, 0, b"")]
    lg = np.asarray(eng.last_logits(B)).reshape(B, V)
    assert out == [int(np.argmax(host.apply_penalties(lg[b], wins[b], 1.3, 0.0, 0.0))) for b in range(B)]
    got = eng.last_logprobs()
    check_rows((got[0][:1], got[1][:1], got[2][:1]), lg[:1], out[:1], 20, "penalised row 0")
    check_rows((got[0][1:], got[1][1:], got[2][1:]), lg[1:], out[1:], 0, "penalised row 1")


def test_resample_and_off_rows(engine):
    eng, cfg = engine
    V = cfg.vocab_size
    toks, _ = generate(eng, V, 2, 0.0, None, False)
    lg = np.asarray(eng.last_logits(2)).reshape(2, V)
    eng.set_logprobs([-1, 5])
    out = [int(t) for t in eng.resample(2, [0.0, 0.0], [0, 0], 0, b"")]
    assert out == toks[-1]
    lp, ids, lps = eng.last_logprobs()
    assert np.isnan(lp[0]) and np.all(ids[0] == -1) and np.all(np.isneginf(lps[0]))   # the off row
    check_rows((lp[1:], ids[1:], lps[1:]), lg[1:], out[1:], 5, "resample row 1")
    assert eng.resample(2, [0.0, 0.0], [0, 0], 0, b"") == out and len(eng.last_logprobs()) == 0


def test_errors(engine):
    eng, cfg = engine
    toks, _ = generate(eng, cfg.vocab_size, 1, 0.0, None, False)
    with pytest.raises(RuntimeError, match="top_n above"):
        eng.set_logprobs([21])
    with pytest.raises(RuntimeError, match="batch out of range"):
        eng.set_logprobs([1] * 4)
    eng.set_logprobs([20, 20])   # staged for two rows, launched with one: refused, and dropped
    with pytest.raises(RuntimeError, match="another batch size"):
        eng.decode([0], toks[-1], [8 + STEPS], [0.0], [0], 0, b"")
    out = eng.decode([0], toks[-1], [8 + STEPS], [0.0], [0], 0, b"")
    assert 0 <= out[0] < cfg.vocab_size and len(eng.last_logprobs()) == 0
    # sample_first and resample refuse it too, before their sampler is enqueued, and drop it
    eng.set_logprobs([20, 20])
    with pytest.raises(RuntimeError, match="another batch size"):
        eng.sample_first(7, 0.0, 0, 1.0, 1, b"")
    eng.set_logprobs([20, 20])
    with pytest.raises(RuntimeError, match="another batch size"):
        eng.resample(1, [0.0], [0], 0, b"")
    assert eng.resample(1, [0.0], [0], 0, b"") == out and len(eng.last_logprobs()) == 0
    # a call that throws for another reason drops the staging as well: it never reaches a later launch
    eng.set_logprobs([20])
    with pytest.raises(RuntimeError, match="position out of range"):
        eng.decode([0], out, [10 ** 6], [0.0], [0], 0, b"")
    eng.decode([0], out, [9 + STEPS], [0.0], [0], 0, b"")
    assert len(eng.last_logprobs()) == 0
    eng.set_logprobs([20])       # a graph-replayed loop carries no logprob launch: dropped, not kept
    eng.decode_loop_prepare([0], [out[0]], [10 + STEPS])
    eng.decode_loop_run(1, 1, True)
    eng.synchronize()
    assert eng.resample(1, [0.0], [0], 0, b"") and len(eng.last_logprobs()) == 0


def test_kernel_is_built_without_scratch():
    """metadata of the built extension only (tools/kernel_resources.py)"""
    from tools.kernel_resources import hot_with_scratch, kernels

    rows = kernels()
    mine = [r for r in rows if "logprob_kernel" in r["name"]]
    assert mine, "logprob_kernel is not in the built extension"
    assert all(r["scratch"] == 0 for r in mine)
    assert not [r for r in hot_with_scratch(rows) if "logprob_kernel" in r["name"]]
