#!/usr/bin/env python3
"""Workload for timing per-token logprobs in a serving-style decode (profiles/logprobs.txt).

A short decode of a random-init model at T = 0.8, top-k 40, top-p 0.95 through the pipelined engine calls
(submit, sample, collect: one synchronous step), in three phases of `--steps` steps each: nothing staged,
then Engine.set_logprobs with top_n = 0, then with top_n = 20.  Prints the wall time per step of each phase
(host clock around steps that end in the collect's event wait; take it with the profiler off).  Under the
profiler the logprob kernel's launches come in phase order, top_n = 0 first:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/logprobs_profile.py --batch 8
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--model", default="tinyllama-1.1b")
    a = ap.parse_args(argv)

    import numpy as np

    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset(a.model)
    B = a.batch
    eng = random_engine(cfg, "Q4_K_M", seed=1, max_ctx=512, max_slots=B, max_batch=B)
    rng = np.random.default_rng(0)
    temps, topk, topp = [0.8] * B, [40] * B, [0.95] * B
    for top_n in (None, 0, 20):
        seqs = [[cfg.bos_id] + [int(t) for t in rng.integers(3, cfg.vocab_size, 80)] for _ in range(B)]
        last = [int(np.argmax(np.asarray(eng.prefill(s, p, 0, True)))) for s, p in enumerate(seqs)]
        pos = [len(p) for p in seqs]
        lp = 0.0
        for i in range(a.warmup + a.steps):
            if i == a.warmup:
                eng.synchronize()
                t0 = time.perf_counter()
            eng.decode_submit(list(range(B)), last if i == 0 else [], pos, temps, topk, 0, topp, [7 + b for b in range(B)])
            if top_n is not None:
                eng.set_logprobs([top_n] * B)
            eng.decode_sample(b"")
            last = eng.decode_collect()
            if top_n is not None:
                lp = float(eng.last_logprobs()[0][0])
            pos = [x + 1 for x in pos]
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        print(f"{a.model} V={cfg.vocab_size} B={B} logprobs={'off' if top_n is None else f'top_n={top_n}'}: "
              f"{ms:.4f} ms/step over {a.steps} steps (last token {int(last[0])}, logprob {lp:.4f})", flush=True)
    eng.synchronize()


if __name__ == "__main__":
    main()
