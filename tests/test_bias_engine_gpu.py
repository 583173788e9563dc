"""Engine.set_sample_processors with logit-bias lists on the device: every sampler launch that takes the staged
processors (decode, the pipelined decode_sample, sample_first, the sampler inside spec_decode) against the host
rule (aios_amd.runtime.sampler.apply_logit_bias) applied to that launch's logits; the lists are one-shot, the
logprobs staged beside them stay those of the raw row, and every malformed list is refused.  Presets: test-tiny
(V = 512) and test-mistral-shape (V = 1024), Q4_K_M."""
import numpy as np
import pytest

import logprob_oracle as LO
import spec_oracle as SO
from aios_amd.runtime import sampler as host

pytestmark = pytest.mark.gpu

PROMPTS = [[1, 30, 40, 50, 60, 70, 80, 90], [1, 31, 41, 51, 61, 71, 81, 91]]
NEUTRAL = ([0.0], [1.0], [0.0], [0.0], [[]])


@pytest.fixture(scope="module", params=["test-tiny", "test-mistral-shape"])
def engine(request):
    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset(request.param)
    return random_engine(cfg, "Q4_K_M", seed=3, max_ctx=64, max_slots=4, max_batch=4), cfg


def neutral(B):
    return [x * B for x in NEUTRAL]


def biased(logits, ids, vals):
    return int(np.argmax(host.apply_logit_bias(logits, ids, vals)))


def lists_for(V, ban, seed, n=300):
    """a row's list: `ban` banned, n - 1 further distinct ids with biases in [-4, 4], a few of them banned too"""
    rng = np.random.default_rng(seed)
    ids = [int(ban)] + [int(i) for i in rng.permutation(V) if int(i) != ban][:n - 1]
    vals = [-np.inf] + [float(-np.inf if rng.random() < 0.05 else rng.uniform(-4, 4)) for _ in ids[1:]]
    return ids, vals


@pytest.mark.parametrize("pipelined", [False, True])
def test_decode_one_shot(engine, pipelined):
    """B = 2: a plain step, the same step with lists that ban its tokens, the plain step again"""
    eng, cfg = engine
    V, B = cfg.vocab_size, 2
    last = [int(np.argmax(np.asarray(eng.prefill(s, PROMPTS[s], 0, True)))) for s in range(B)]
    pos = [len(p) for p in PROMPTS]

    def step(lists):
        if lists is not None:
            eng.set_sample_processors(*neutral(B), [l[0] for l in lists], [l[1] for l in lists])
        if pipelined:
            eng.decode_submit([0, 1], last, pos, [0.0] * B, [0] * B, 0)
            eng.decode_sample(b"")
            out = eng.decode_collect()
        else:
            out = eng.decode([0, 1], last, pos, [0.0] * B, [0] * B, 0, b"")
        lg = np.asarray(eng.last_logits(B)).reshape(B, V)
        for b in range(B):
            want = int(np.argmax(lg[b])) if lists is None else biased(lg[b], *lists[b])
            assert int(out[b]) == want, (b, lists is not None)
        return [int(t) for t in out]

    plain = step(None)
    # row 0: a 300-entry list; row 1: the ban alone (the rows' strides differ: row 1 is padded with empty entries)
    lists = [lists_for(V, plain[0], 1), ([plain[1]], [-np.inf])]
    moved = step(lists)
    assert all(moved[b] != plain[b] for b in range(B))
    assert step(None) == plain                                           # one shot
    assert step([([], []), lists[1]]) == [plain[0], moved[1]]            # an empty list is neutral
    assert step([([], []), ([], [])]) == plain


def test_sample_first(engine):
    eng, cfg = engine
    V = cfg.vocab_size
    logits = np.asarray(eng.prefill(0, PROMPTS[0], 0, True))
    order = np.argsort(-logits)
    best, fifth = int(order[0]), int(order[4])
    ids, vals = [best, fifth], [-np.inf, float(logits[order[1]] - logits[fifth]) + 0.5]
    assert biased(logits, ids, vals) == fifth
    eng.set_sample_processors(*NEUTRAL, [ids], [vals])
    assert eng.sample_first(7, 0.0, 0, 1.0, 1, b"") == fifth
    assert eng.sample_first(7, 0.0, 0, 1.0, 1, b"") == best
    # with a mask: a masked token stays out whatever its bias, and the ban holds among the allowed ones
    allowed = [int(t) for t in order[:3]]
    bits = np.zeros(V, np.uint8)
    bits[allowed] = 1
    mask = np.packbits(bits, bitorder="little").tobytes()
    eng.set_sample_processors(*NEUTRAL, [[best, fifth]], [[-np.inf, 100.0]])
    assert eng.sample_first(7, 0.0, 0, 1.0, 1, mask) == int(order[1])


@pytest.mark.parametrize("sampled", [False, True])
def test_spec_decode_emits_what_sequential_biased_decode_emits(engine, sampled):
    """R = 4: four sequential B = 1 decode steps, each with the list staged, give t1..t4; spec_decode over
    [t0, t1, t2, t3] with the list on every row accepts the whole draft and emits the same four tokens.  A wrong
    draft stops there, and the rows are those of decode() with the same lists (the accept rule of spec_oracle)."""
    eng, cfg = engine
    V, R, pos0, seed = cfg.vocab_size, 4, len(PROMPTS[0]), 4321
    kw = dict(temperature=0.8, top_k=40, top_p=0.9, seed=seed) if sampled else {}
    dec_kw = ([0.8], [40], 0, b"", [0.9], [seed]) if sampled else ([0.0], [0], 0, b"")
    t0 = int(np.argmax(np.asarray(eng.prefill(0, PROMPTS[0], 0, True))))
    # the unbiased continuation's tokens are what the list bans: the biased run has to leave it
    eng.copy_slot(0, 1, pos0)
    free, t = [], t0
    for i in range(R):
        t = int(eng.decode([1], [t], [pos0 + i], *dec_kw)[0])
        free.append(t)
    ids = sorted(set(free)) + [i for i in range(5, 45) if i not in free]
    vals = [-np.inf] * len(set(free)) + [float(x) for x in np.linspace(-3, 3, len(ids) - len(set(free)))]
    eng.copy_slot(0, 1, pos0)
    seq, t = [], t0
    for i in range(R):
        eng.set_sample_processors(*NEUTRAL, [ids], [vals])
        t = int(eng.decode([1], [t], [pos0 + i], *dec_kw)[0])
        seq.append(t)
    assert not set(seq) & set(free)
    draft = [t0] + seq[:R - 1]

    def spec(toks):
        eng.copy_slot(0, 2, pos0)
        eng.set_sample_processors(*neutral(R), [ids] * R, [vals] * R)
        acc, out = eng.spec_decode(2, toks, pos0, **kw)
        return int(acc), [int(x) for x in out]

    assert spec(draft) == (R - 1, seq)
    bad = list(draft)
    bad[2] = (draft[2] + 1) % V
    acc, out = spec(bad)
    assert acc == 1 and out == seq[:2]
    eng.copy_slot(0, 3, pos0)
    eng.set_sample_processors(*neutral(R), [ids] * R, [vals] * R)
    rows = ([0.8] * R, [40] * R, 0, b"", [0.9] * R, [seed] * R) if sampled else ([0.0] * R, [0] * R, 0, b"")
    dec = [int(x) for x in eng.decode([3] * R, bad, list(range(pos0, pos0 + R)), *rows)]
    assert (acc, out) == SO.accept(bad, dec)
    # one shot: the next speculative step is unbiased
    eng.copy_slot(0, 2, pos0)
    acc, out = eng.spec_decode(2, [t0] + free[:R - 1], pos0, **kw)
    assert int(acc) == R - 1 and [int(x) for x in out] == free


def test_logprobs_beside_a_bias_report_the_raw_row(engine):
    eng, cfg = engine
    V, B = cfg.vocab_size, 2
    last = [int(np.argmax(np.asarray(eng.prefill(s, PROMPTS[s], 0, True)))) for s in range(B)]
    pos = [len(p) for p in PROMPTS]
    plain = [int(t) for t in eng.decode([0, 1], last, pos, [0.0] * B, [0] * B, 0, b"")]
    lists = [lists_for(V, plain[0], 2, n=64), ([plain[1], 7], [-np.inf, 2.0])]
    eng.set_sample_processors(*neutral(B), [l[0] for l in lists], [l[1] for l in lists])
    eng.set_logprobs([5, 0])
    out = [int(t) for t in eng.decode([0, 1], last, pos, [0.0] * B, [0] * B, 0, b"")]
    lg = np.asarray(eng.last_logits(B)).reshape(B, V)
    assert out == [biased(lg[b], *lists[b]) for b in range(B)] and all(out[b] != plain[b] for b in range(B))
    lp, ids, lps = eng.last_logprobs()
    for b, n in enumerate((5, 0)):
        x, oid, olp = LO.logprobs(lg[b], out[b], n)  # the unbiased row
        err = max(abs(float(lp[b]) - x), float(np.max(np.abs(lps[b, :len(oid)] - olp), initial=0.0)))
        print(f"bias engine logprobs row {b}: max |gpu - oracle on the raw row| = {err:.3e}")
        assert err <= LO.GPU_TOL
        assert ids[b, :len(oid)].tolist() == oid.tolist()
    assert int(ids[0, 0]) == plain[0]  # the raw best alternative is the token the list banned


def test_refusals(engine):
    eng, cfg = engine
    V = cfg.vocab_size
    logits = np.asarray(eng.prefill(0, PROMPTS[0], 0, True))
    best = int(np.argmax(logits))
    bad = [
        ([[1], [2]], [[0.0], [0.0]], "size mismatch"),             # two lists for one row
        ([[1]], [], "size mismatch"),
        ([[1, 2]], [[0.0]], "size mismatch"),                      # ids and values of different lengths
        ([[0] * 513], [[0.0] * 513], "logit bias longer than 512"),
        ([[3, 9, 3]], [[0.0, 1.0, 2.0]], "duplicate"),
        ([[V]], [[0.0]], "out of range"),
        ([[-1]], [[0.0]], "out of range"),
        ([[3]], [[np.inf]], "finite or -inf"),
        ([[3]], [[np.nan]], "finite or -inf"),
    ]
    if V <= 512:  # (test-tiny: a list can name the whole vocabulary)
        bad.append(([list(range(V))], [[-np.inf] * V], "bans every token"))
    for ids, vals, what in bad:
        with pytest.raises(RuntimeError, match=what):
            eng.set_sample_processors(*NEUTRAL, ids, vals)
        assert eng.sample_first(7, 0.0, 0, 1.0, 1, b"") == best  # nothing was staged
    # the longest list, every entry but one a ban
    n = min(V, 512)
    ids = [i for i in range(V) if i != best][:n - 1] + [best]
    eng.set_sample_processors(*NEUTRAL, [ids], [[-np.inf] * (n - 1) + [-1e-3]])
    assert eng.sample_first(7, 0.0, 0, 1.0, 1, b"") == biased(logits, ids, [-np.inf] * (n - 1) + [-1e-3])
    # staged for two rows, launched with one: refused, and dropped
    eng.set_sample_processors(*neutral(2), [[best], []], [[-np.inf], []])
    with pytest.raises(RuntimeError, match="another batch size"):
        eng.sample_first(7, 0.0, 0, 1.0, 1, b"")
    assert eng.sample_first(7, 0.0, 0, 1.0, 1, b"") == best
