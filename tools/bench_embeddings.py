#!/usr/bin/env python3
"""Time Engine.embed_prefill (mean pooling) against prefill(..., want_logits=False) of the same tokens
(profiles/embeddings.txt): Mistral-7B Q4_K_M synthetic, prompts of 128 / 512 / 2048 tokens.

  python tools/bench_embeddings.py                 # both calls, alternating, three repetitions each
  python tools/bench_embeddings.py --prefill-only  # on a build without embed_prefill (the parent commit)

Each repetition is the median of --iters calls after one warm-up call.  For the pool kernel's own time run it
under the profiler and read embed_pool_kernel's row:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_embeddings.py --reps 1
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--recipe", default="Q4_K_M")
    ap.add_argument("--lengths", default="128,512,2048")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--prefill-only", action="store_true")
    a = ap.parse_args()

    import numpy as np

    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset(a.model)
    lengths = [int(x) for x in a.lengths.split(",")]
    eng = random_engine(cfg, a.recipe, seed=1234, max_ctx=max(lengths), max_slots=1, max_batch=1)
    rng = np.random.default_rng(0)

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    out = {"model": a.model, "recipe": a.recipe, "lengths": {}}
    for T in lengths:
        ids = [cfg.bos_id] + [int(t) for t in rng.integers(3, cfg.vocab_size, T - 1)]
        calls = {"prefill": lambda: eng.prefill(0, ids, 0, False)}
        if not a.prefill_only:
            calls["embed_prefill"] = lambda: eng.embed_prefill(0, ids, 0, 1, True)
        res = {k: [] for k in calls}
        for _ in range(a.reps):  # alternating
            for k, fn in calls.items():
                res[k].append(round(timed(fn), 4))
        out["lengths"][T] = res
        print(f"T={T}: " + ", ".join(f"{k} {v} ms" for k, v in res.items()), flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
