#!/usr/bin/env python3
"""Profile of the context shift (Engine.shift_context, csrc/kernels/kv_shift.hip) -> profiles/context_shift.txt.

  1. one shift_context call on Mistral-7B Q4_K_M synthetic weights at a full 4k and a full 32k window, bf16 and fp8
     caches: milliseconds (host clock around the call, which ends in a stream synchronise) and achieved bytes per
     second, bytes = moved rows x layers x (K + V) x kv heads x head_dim x element size x (read + write);
  2. the kernel's VGPR / SGPR / LDS / scratch figures from tools/kernel_resources.py;
  3. the headline decode (bench.py) of this tree and, with --parent DIR (a built checkout of the parent commit), of
     the parent, three alternating runs each.

  python tools/context_shift_profile.py [--parent DIR] [--out profiles/context_shift.txt] [--windows 4096,32768]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shift_times(window: int, kv: str, reps: int = 5):
    """[(label, n, n_keep, n_discard, ms, bytes)] on a slot prefilled to the whole window"""
    import numpy as np

    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import random_engine

    cfg = get_preset("mistral-7b")
    eng = random_engine(cfg, "Q4_K_M", seed=0, max_ctx=window, max_slots=1, max_batch=1, kv_dtype=kv)
    rng = np.random.default_rng(0)
    for start in range(0, window, 2048):
        n = min(2048, window - start)
        eng.prefill(0, [int(t) for t in rng.integers(3, cfg.vocab_size, n)], start, False)
    eng.synchronize()
    es = 1 if kv != "bf16" else 2
    row = cfg.n_layers * 2 * cfg.n_kv_heads * cfg.head_dim * es * 2   # bytes read + written per moved position
    out = []

    def one(label, n, keep, d):
        t0 = time.perf_counter()
        n_new = eng.shift_context(0, n, keep, d)
        ms = (time.perf_counter() - t0) * 1e3
        out.append((label, n, keep, d, ms, (n - keep - d) * row))
        return n_new

    # the whole window moves by one position (the most bytes a shift can move); the first call loads the code object
    n = window
    n = one("warm-up, whole window by 1", n, 0, 1)
    for _ in range(reps):
        n = one("whole window by 1", n, 0, 1)
    # llama.cpp's numbers with n_keep 256: half of what is behind the kept prefix goes
    one("n_keep 256, n_discard (n - 256) // 2", n, 256, (n - 256) // 2)
    return out


def bench(tree: str, steps: int, warmup: int) -> dict:
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=tree, capture_output=True, text=True, timeout=900)
    for line in reversed(r.stdout.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError(f"bench.py in {tree} printed no result line:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit (for the alternating bench runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_shift.txt"))
    ap.add_argument("--windows", default="4096,32768")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-bench", action="store_true")
    a = ap.parse_args()
    L = ["# Context shift (Engine.shift_context, aios::kv_shift_kernel): tools/context_shift_profile.py on one MI355X.", ""]
    L += ["## 1. One shift_context call, Mistral-7B Q4_K_M synthetic weights, a full window (ms: host clock around the",
          "##    call, table uploads and the closing synchronise included; GB/s: bytes read + written by the kernel / that time)", ""]
    L.append(f"{'window':>7} {'cache':>9}  {'n':>6} {'n_keep':>6} {'n_discard':>9} {'ms':>8} {'GB moved':>9} {'GB/s':>8}  what")
    for w in [int(x) for x in a.windows.split(",")]:
        for kv in ("bf16", "fp8_e4m3"):
            rows = shift_times(w, kv)
            for label, n, keep, d, ms, nbytes in rows:
                L.append(f"{w:>7} {kv:>9}  {n:>6} {keep:>6} {d:>9} {ms:>8.3f} {nbytes / 1e9:>9.3f} {nbytes / 1e6 / ms:>8.1f}  {label}")
            whole = [r for r in rows if r[0] == "whole window by 1"]
            med = statistics.median(r[4] for r in whole)
            L.append(f"{'':>7} {'':>9}  whole window by 1: median {med:.3f} ms = {whole[0][5] / 1e6 / med:.1f} GB/s")
            print("\n".join(L[-len(rows) - 1:]), flush=True)
    L += ["", "## 2. Resources (tools/kernel_resources.py --all --grep kv_shift; read from the built extension)", ""]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--all", "--grep", "kv_shift"],
                       capture_output=True, text=True)
    L += r.stdout.rstrip().splitlines()
    if not a.no_bench:
        L += ["", f"## 3. Headline decode: python bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}, alternating runs", ""]
        trees = ([("parent", a.parent)] if a.parent else []) + [("this", ROOT)]
        if not a.parent:
            L.append("(no --parent checkout given: the parent was not measured in this run)")
        got = {k: [] for k, _ in trees}
        for _ in range(3):
            for k, tree in trees:
                res = bench(tree, a.steps, a.warmup)
                got[k].append(res)
                line = f"{k:<8} " + json.dumps({x: res[x] for x in res if isinstance(res[x], (int, float, str))})[:300]
                L.append(line)
                print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
