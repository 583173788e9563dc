#!/usr/bin/env python3
"""Workload for timing the device sampler with and without logit processors (profiles/sampler_processors.txt).

A short serving-style decode of a random-init TinyLlama (V = 32000) at T = 0.8, top-k 40, top-p 0.95
through the pipelined engine calls: `--steps` steps with no processors (the `sample_kernel<false>`
instantiation), then the same with min_p = 0.05 and repeat / presence / frequency penalties over a
64-token window (`sample_kernel<true>`).  Run it under the profiler, one batch size per run; the two
instantiations are separate rows of the kernel statistics:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/sampler_processors_profile.py --batch 8
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
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
    for processors in (False, True):
        seqs = [[cfg.bos_id] + [int(t) for t in rng.integers(3, cfg.vocab_size, 80)] for _ in range(B)]
        last = []
        for s, p in enumerate(seqs):
            last.append(int(np.argmax(np.asarray(eng.prefill(s, p, 0, True)))))
            p.append(last[-1])
        pos = [len(p) - 1 for p in seqs]
        for i in range(a.steps):
            eng.decode_submit(list(range(B)), last if i == 0 else [], pos, temps, topk, 0, topp, [7 + b for b in range(B)])
            if processors:
                eng.set_sample_processors([0.05] * B, [1.1] * B, [0.1] * B, [0.1] * B, [p[-64:] for p in seqs])
            eng.decode_sample(b"")
            out = eng.decode_collect()
            for b in range(B):
                seqs[b].append(int(out[b]))
            pos = [x + 1 for x in pos]
        print(f"B={B} processors={'on' if processors else 'off'}: {a.steps} steps, last tokens {[p[-1] for p in seqs]}")
    eng.synchronize()


if __name__ == "__main__":
    main()
