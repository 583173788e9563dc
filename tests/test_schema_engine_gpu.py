"""Engine.set_grammar_rows on test-tiny: the tokens of steps whose masks the device computes from (grammar id,
state) are the tokens of the same steps fed the host rule's mask bytes -- greedy and sampled, host-fed decode and
the pipelined decode_submit / decode_sample / decode_collect, sample_first and resample, B = 1 and B = 3 (a free
row, a JsonGrammar row with host mask bytes, a schema row); the staging is one-shot; grammar ids are reused
safely; a vocabulary that cannot spell the grammar is refused at load."""
import numpy as np
import pytest

import schema_oracle as SO
from aios_amd.runtime import json_schema as JS
from aios_amd.runtime import sampler as host

pytestmark = pytest.mark.gpu

PROMPTS = [[1, 30, 40, 50, 60, 70, 80, 90], [1, 31, 41, 51, 61, 71, 81, 91], [1, 32, 42, 52, 62, 72, 82, 92]]
EOS = (2,)


@pytest.fixture(scope="module")
def setup():
    from aios_amd.models.config import get_preset
    from aios_amd.runtime import native
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset("test-tiny")
    eng = random_engine(cfg, "Q4_K_M", seed=3, max_ctx=96, max_slots=4, max_batch=4)
    tokens, eos = SO.make_vocab(cfg.vocab_size, seed=9, eos=EOS)
    eng.grammar_vocab(tokens, eos)
    vocab = JS.Vocab(tokens, eos)
    dfa = JS.compile_schema(SO.BOUNDED["tool_call"])
    gid = eng.grammar_load(dfa.byte_class, dfa.trans, dfa.accept)
    jg = native.load(build_if_missing=False).JsonGrammar(tokens, eos[0])
    return eng, cfg, JS.SchemaGrammar(dfa, vocab), gid, jg, tokens


def _sampling(B, sampled):
    return ([0.9] * B, [30] * B, 0) if sampled else ([0.0] * B, [0] * B, 0)


def _generate(setup, device_masks, sampled, pipelined, B, steps=12):
    """B rows (row 0 free, row 1 JsonGrammar with host bytes, the last row the schema; B = 1: the schema row
    alone) for `steps` steps; returns the rows' tokens and the schema row's state trail"""
    eng, cfg, g, gid, jg, _ = setup
    V = cfg.vocab_size
    full = host.all_allowed(V)
    kinds = ["schema"] if B == 1 else ["free", "json", "schema"]
    seeds = [11, 22, 33][:B]
    states = [g.initial() if k == "schema" else jg.initial() if k == "json" else None for k in kinds]
    last = [int(np.argmax(np.asarray(eng.prefill(s, PROMPTS[s], 0, True)))) for s in range(B)]
    pos = [len(PROMPTS[s]) for s in range(B)]
    out, trail = [[] for _ in range(B)], []
    temps, topk, seed = _sampling(B, sampled)
    for _ in range(steps):
        rows = []
        for k, st in zip(kinds, states):
            if k == "free":
                rows.append(full)
            elif k == "json":
                rows.append(jg.mask(st))
            else:
                rows.append(full if device_masks and B > 1 else b"" if device_masks else g.mask(st))
        trail.append(states[-1].s)
        if device_masks:
            eng.set_grammar_rows([gid if k == "schema" else -1 for k in kinds],
                                 [st.s if k == "schema" else 0 for k, st in zip(kinds, states)])
        mask = b"".join(rows)
        if pipelined:
            eng.decode_submit(list(range(B)), last, pos, temps, topk, seed, [0.95] * B, seeds)
            eng.decode_sample(mask)
            toks = eng.decode_collect()
        else:
            toks = eng.decode(list(range(B)), last, pos, temps, topk, seed, mask, [0.95] * B, seeds)
        toks = [int(t) for t in toks]
        done = False
        for b, (k, st, t) in enumerate(zip(kinds, states, toks)):
            out[b].append(t)
            if k == "schema":
                if t in EOS:
                    assert g.accepting(st)
                    done = True
                else:
                    assert g.accept_token(st, t), (b, t)  # the sampler stayed inside the mask
                    done = done or g.complete(st)
            elif k == "json" and (not jg.accept_token(st, t) or jg.complete(st)):
                states[b] = jg.initial()  # (its object closed: the row starts another)
        last, pos = toks, [p + 1 for p in pos]
        if done:
            break
    return out, trail


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("sampled", [False, True])
def test_device_masks_give_the_tokens_of_host_masks(setup, sampled, pipelined, B):
    want, trail_h = _generate(setup, False, sampled, pipelined, B)
    got, trail_d = _generate(setup, True, sampled, pipelined, B)
    print(f"B={B} sampled={sampled} pipelined={pipelined}: {len(want[-1])} steps, schema row {want[-1]}")
    assert got == want and trail_d == trail_h and len(want[-1]) >= 3


def test_the_mask_matters_and_the_staging_is_one_shot(setup):
    eng, cfg, g, gid, _, _ = setup
    V = cfg.vocab_size
    logits = np.asarray(eng.prefill(0, PROMPTS[0], 0, True))
    free = int(np.argmax(logits))
    allowed = host.mask_to_bool(g.mask_of(1), V)
    assert not allowed[free]  # (random weights do not open a tool call on their own)
    want = int(np.argmax(np.where(allowed, logits, -np.inf)))
    eng.set_grammar_rows([gid], [1])
    assert eng.sample_first(7, 0.0, 0, 1.0, 1, b"") == want
    assert eng.sample_first(7, 0.0, 0, 1.0, 1, b"") == free          # one shot
    # decode, then resample of the same logits under the grammar, then plain again
    t = [int(x) for x in eng.decode([0], [free], [8], [0.0], [0], 0, b"")]
    lg = np.asarray(eng.last_logits(1)).reshape(-1)
    assert t == [int(np.argmax(lg))]
    st = 5
    ok = host.mask_to_bool(g.mask_of(st), V)
    eng.set_grammar_rows([gid], [st])
    assert [int(x) for x in eng.resample(1, [0.0], [0], 0, b"")] == [int(np.argmax(np.where(ok, lg, -np.inf)))]
    assert [int(x) for x in eng.resample(1, [0.0], [0], 0, b"")] == t
    # a row with id -1 beside a host mask keeps the host's bytes
    only = np.zeros(V, np.uint8)
    only[[40, 41]] = 1
    eng.set_grammar_rows([-1], [0])
    got = eng.sample_first(7, 0.0, 0, 1.0, 1, np.packbits(only, bitorder="little").tobytes())
    assert got == (40 if logits[40] >= logits[41] else 41)
    # staged for two rows, launched with one: refused and dropped
    eng.set_grammar_rows([gid, -1], [1, 0])
    with pytest.raises(RuntimeError, match="another batch size"):
        eng.sample_first(7, 0.0, 0, 1.0, 1, b"")
    assert eng.sample_first(7, 0.0, 0, 1.0, 1, b"") == free
    for gids, states, what in (([gid], [0], "state out of range"), ([gid], [g.dfa.n_states], "state out of range"),
                               ([63], [1], "unknown grammar"), ([gid], [1, 2], "size mismatch"),
                               ([gid] * 5, [1] * 5, "batch out of range")):
        with pytest.raises(RuntimeError, match=what):
            eng.set_grammar_rows(gids, states)
        assert eng.sample_first(7, 0.0, 0, 1.0, 1, b"") == free      # nothing was staged


def test_grammar_masks_and_id_reuse(setup):
    eng, cfg, g, gid, _, _ = setup
    nb = (cfg.vocab_size + 7) // 8
    states = list(range(g.dfa.n_states))
    got = eng.grammar_masks(gid, states)
    assert got == b"".join(g.mask_of(s) for s in states)
    n0 = eng.grammars_loaded
    other = JS.compile_schema(SO.BOUNDED["flags"])
    og = JS.SchemaGrammar(other, g.vocab)
    a = eng.grammar_load(other.byte_class, other.trans, other.accept)
    assert a != gid and eng.grammars_loaded == n0 + 1
    assert eng.grammar_masks(a, [1, 2]) == og.mask_of(1) + og.mask_of(2)
    eng.grammar_free(a)
    for call in (lambda: eng.grammar_masks(a, [1]), lambda: eng.set_grammar_rows([a], [1]), lambda: eng.grammar_free(a)):
        with pytest.raises(RuntimeError, match="unknown grammar"):
            call()
    third = JS.compile_schema(SO.BOUNDED["choice"])
    b = eng.grammar_load(third.byte_class, third.trans, third.accept)
    assert b == a and eng.grammars_loaded == n0 + 1                   # the freed id serves the next grammar
    assert eng.grammar_masks(b, [1]) == JS.SchemaGrammar(third, g.vocab).mask_of(1)
    assert eng.grammar_masks(gid, [1]) == g.mask_of(1) and len(got) == nb * len(states)  # the first one is untouched
    eng.grammar_free(b)
    bad = other.trans.copy()
    bad[1, 0] = other.n_states
    for bc, tr, ac, what in ((other.byte_class, bad, other.accept, "transition out of range"),
                             (other.byte_class + other.n_classes, other.trans, other.accept, "byte class out of range"),
                             (other.byte_class, other.trans, other.accept[:-1], "expected")):
        with pytest.raises(RuntimeError, match=what):
            eng.grammar_load(bc, tr, ac)
    assert eng.grammars_loaded == n0


def test_a_vocabulary_that_cannot_spell_the_grammar_is_refused():
    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset("test-tiny")
    eng = random_engine(cfg, "Q4_K_M", seed=3, max_ctx=32, max_slots=1, max_batch=1)
    dfa = JS.compile_schema({"type": "boolean"})
    with pytest.raises(RuntimeError, match="no vocabulary"):
        eng.grammar_load(dfa.byte_class, dfa.trans, dfa.accept)
    tokens = [b""] * cfg.vocab_size
    for i, w in enumerate((b"t", b"r", b"e", b"f", b"a", b"l", b"s"), start=3):  # no "u": true cannot be finished
        tokens[i] = w
    eng.grammar_vocab(tokens, [2])
    dead = JS.SchemaGrammar(dfa, JS.Vocab(tokens, [2])).token_dead_states()
    assert dead
    with pytest.raises(RuntimeError, match=f"state {dead[0]} allows no token"):
        eng.grammar_load(dfa.byte_class, dfa.trans, dfa.accept)
    assert eng.grammars_loaded == 0
    tokens[10] = b"u"
    eng.grammar_vocab(tokens, [2])
    assert eng.grammar_load(dfa.byte_class, dfa.trans, dfa.accept) == 0
