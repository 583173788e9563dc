#!/usr/bin/env python3
"""Speculative decoding's step cost and pay-off (Engine.spec_decode beside the B = 1 step of the same build).

Per model and context (keys already in the slot): the host-synchronous time of one spec_decode call for
R = 2..8 rows and of one plain decode() call, measured interleaved (round-robin over R, several rounds, the
median of the rounds' means); from those the break-even number of accepted drafts per step, t_R / t_1 - 1,
and tokens per second at forced acceptance of 0 / 25 / 50 / 100 % -- a fully accepted chain of drafts,
corrupted at row round(a * (R - 1)), so a step emits that many drafts plus one token.  The models are
random-init: their text does not repeat, so real acceptance rates are not measured here.

  python tools/bench_spec.py --model mistral-7b --keys 128,4096

--multi: the same for Engine.spec_decode_multi -- S = 2, 3, 4 sequences with d = 0, 3, 7 drafts each (Rt =
S (1 + d) rows) beside one plain decode() of S rows, every sequence at the same context.  Break-even is per
sequence: the accepted drafts each sequence needs per step, t_multi / t_plain - 1; tokens per second count all
S sequences, S (k + 1) per step at k forced accepted drafts per sequence against S per plain step.

  python tools/bench_spec.py --model mistral-7b --keys 128,4096 --multi
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def chain(eng, t0, pos0, R, slot):
    """R tokens, each the one the row before it samples (greedy), from the R-row kernels themselves"""
    c = [t0]
    for j in range(R - 1):
        acc, out = eng.spec_decode(slot, c + [0] * (R - len(c)), pos0)
        c.append(int(out[j]))
    return c


def multi_chains(eng, slots, t0, pos0, d):
    """per sequence 1 + d tokens, each the one the row before it samples (greedy), from the Rt-row kernels"""
    cs = [[t0] for _ in slots]
    for j in range(d):
        res = eng.spec_decode_multi(slots, [c + [0] * (d + 1 - len(c)) for c in cs], [pos0] * len(slots))
        for c, (_, out) in zip(cs, res):
            c.append(int(out[j]))
    return cs


def main_multi(a):
    import numpy as np

    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset(a.model)
    keys = [int(k) for k in a.keys.split(",")]
    eng = random_engine(cfg, a.recipe, seed=1234, max_ctx=max(keys) + 128, max_slots=4, max_batch=32)
    V = cfg.vocab_size
    rng = np.random.default_rng(0)
    for K in keys:
        prompt = [cfg.bos_id] + [int(t) for t in rng.integers(3, V, K - 1)]
        t0 = int(np.asarray(eng.prefill(0, prompt, 0, True)).argmax())
        for s in (1, 2, 3):
            eng.copy_slot(0, s, K)
        calls, chains = {}, {}
        for S in (2, 3, 4):
            slots = list(range(S))
            calls[(S, -1)] = (lambda slots=slots: eng.decode(slots, [t0] * len(slots), [K] * len(slots)))
            for d in (0, 3, 7):
                chains[(S, d)] = multi_chains(eng, slots, t0, K, d)
                calls[(S, d)] = (lambda slots=slots, c=chains[(S, d)]: eng.spec_decode_multi(slots, c, [K] * len(slots)))
        for f in calls.values():  # graphs captured, caches warm
            for _ in range(5):
                f()
        means = {k: [] for k in calls}
        for _ in range(a.rounds):  # interleaved: every call in every round
            for k, f in calls.items():
                t = time.perf_counter()
                for _ in range(a.iters):
                    f()
                means[k].append((time.perf_counter() - t) / a.iters)
        ms = {k: statistics.median(v) * 1e3 for k, v in means.items()}
        for S in (2, 3, 4):
            plain = ms[(S, -1)]
            row = dict(model=a.model, recipe=a.recipe, keys=K, seqs=S, plain_ms=round(plain, 4),
                       plain_ms_min_max=[round(x * 1e3, 4) for x in (min(means[(S, -1)]), max(means[(S, -1)]))],
                       plain_tok_s=round(S * 1e3 / plain, 1), multi_ms={}, multi_ms_min_max={},
                       break_even_accepted_per_seq={}, tok_s={})
            slots = list(range(S))
            for d in (0, 3, 7):
                t = ms[(S, d)]
                row["multi_ms"][d] = round(t, 4)
                row["multi_ms_min_max"][d] = [round(x * 1e3, 4) for x in (min(means[(S, d)]), max(means[(S, d)]))]
                row["break_even_accepted_per_seq"][d] = round(t / plain - 1, 3)
                for acc in (0.0, 0.25, 0.5, 1.0):
                    k = int(round(acc * d))
                    bad = [list(c) for c in chains[(S, d)]]
                    if k < d:
                        for c in bad:
                            c[k + 1] = (c[k + 1] + 1) % V
                    for n, out in eng.spec_decode_multi(slots, bad, [K] * S):
                        assert n == k and len(out) == k + 1, (S, d, k, n)
                    row["tok_s"].setdefault(str(acc), {})[d] = round(S * (k + 1) * 1e3 / t, 1)
            print(json.dumps(row), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--recipe", default="Q4_K_M")
    ap.add_argument("--keys", default="128,4096")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--multi", action="store_true", help="Engine.spec_decode_multi beside S-row plain steps")
    a = ap.parse_args(argv)
    if a.multi:
        return main_multi(a)
    import numpy as np

    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset(a.model)
    keys = [int(k) for k in a.keys.split(",")]
    eng = random_engine(cfg, a.recipe, seed=1234, max_ctx=max(keys) + 128, max_slots=1, max_batch=8)
    V = cfg.vocab_size
    rng = np.random.default_rng(0)
    for K in keys:
        prompt = [cfg.bos_id] + [int(t) for t in rng.integers(3, V, K - 1)]
        t0 = int(np.asarray(eng.prefill(0, prompt, 0, True)).argmax())
        drafts = {R: chain(eng, t0, K, R, 0) for R in range(2, 9)}

        def plain():
            eng.decode([0], [t0], [K])

        calls = {1: plain}
        for R, c in drafts.items():
            calls[R] = (lambda c=c: eng.spec_decode(0, c, K))
        for f in calls.values():  # graphs captured, caches warm
            for _ in range(5):
                f()
        means = {R: [] for R in calls}
        for _ in range(a.rounds):  # interleaved: every R in every round
            for R, f in calls.items():
                t = time.perf_counter()
                for _ in range(a.iters):
                    f()
                means[R].append((time.perf_counter() - t) / a.iters)
        ms = {R: statistics.median(v) * 1e3 for R, v in means.items()}
        spread = {R: (min(v) * 1e3, max(v) * 1e3) for R, v in means.items()}
        row = dict(model=a.model, recipe=a.recipe, keys=K, step_ms={R: round(ms[R], 4) for R in ms},
                   step_ms_min_max={R: [round(x, 4) for x in spread[R]] for R in spread},
                   plain_tok_s=round(1e3 / ms[1], 1),
                   break_even_accepted={R: round(ms[R] / ms[1] - 1, 3) for R in ms if R > 1}, tok_s={})
        for acc in (0.0, 0.25, 0.5, 1.0):
            for R, c in drafts.items():
                k = int(round(acc * (R - 1)))
                bad = list(c)
                if k < R - 1:
                    bad[k + 1] = (c[k + 1] + 1) % V
                n, out = eng.spec_decode(0, bad, K)
                assert n == k and len(out) == k + 1, (R, k, n)
                row["tok_s"].setdefault(str(acc), {})[R] = round((k + 1) * 1e3 / ms[R], 1)
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
