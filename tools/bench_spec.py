#!/usr/bin/env python3
"""Speculative decoding's step cost and pay-off (Engine.spec_decode beside the B = 1 step of the same build).

Per model and context (keys already in the slot): the host-synchronous time of one spec_decode call for
R = 2..8 rows and of one plain decode() call, measured interleaved (round-robin over R, several rounds, the
median of the rounds' means); from those the break-even number of accepted drafts per step, t_R / t_1 - 1,
and tokens per second at forced acceptance of 0 / 25 / 50 / 100 % -- a fully accepted chain of drafts,
corrupted at row round(a * (R - 1)), so a step emits that many drafts plus one token.  The models are
random-init: their text does not repeat, so real acceptance rates are not measured here.

  python tools/bench_spec.py --model mistral-7b --keys 128,4096
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--recipe", default="Q4_K_M")
    ap.add_argument("--keys", default="128,4096")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
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
