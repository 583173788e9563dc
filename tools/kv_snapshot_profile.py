#!/usr/bin/env python3
"""Profile of the KV snapshots (Engine.kv_save / kv_restore, csrc/kernels/kv_snapshot.hip) -> profiles/kv_snapshot.txt.

  1. Mistral-7B Q4_K_M synthetic weights, bf16 and fp8 caches, a slot of 4k and of 32k tokens: one kv_save and one
     kv_restore call on the host clock (the first call of an engine also allocates the staging: shown apart), the
     pack / unpack kernel alone over all layers (device events around one launch through the raw binding, bytes =
     payload read + payload written), and the prefill of the same tokens by the same build -- what a restore replaces;
  2. the kernel's VGPR / SGPR / LDS / scratch figures from tools/kernel_resources.py;
  3. the headline decode (bench.py) of this tree and, with --parent DIR (a built checkout of the parent commit), of
     the parent, three alternating runs each.

  python tools/kv_snapshot_profile.py [--parent DIR] [--out profiles/kv_snapshot.txt] [--tokens 4096,32768]
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


def measure(n: int, kv: str, reps: int = 3) -> dict:
    import numpy as np
    import torch

    from aios_amd.models.config import get_preset
    from aios_amd.runtime import native
    from aios_amd.runtime.loader import random_engine

    E = native.load(build_if_missing=False)
    cfg = get_preset("mistral-7b")
    eng = random_engine(cfg, "Q4_K_M", seed=0, max_ctx=n, max_slots=2, max_batch=1, kv_dtype=kv)
    rng = np.random.default_rng(0)
    toks = [int(t) for t in rng.integers(3, cfg.vocab_size, n)]

    def prefill(slot):
        t0 = time.perf_counter()
        for start in range(0, n, 2048):
            eng.prefill(slot, toks[start:start + 2048], start, False)
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3

    prefill(0)                       # (loads the code objects)
    eng.release_slot(0)
    out = {"n": n, "kv": kv, "prefill_ms": prefill(0), "bytes": eng.kv_snapshot_bytes(n)}
    save, restore = [], []
    data = None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        data = eng.kv_save(0, n)
        save.append((time.perf_counter() - t0) * 1e3)
    for _ in range(reps + 1):
        eng.release_slot(1)
        t0 = time.perf_counter()
        eng.kv_restore(1, data, n)
        restore.append((time.perf_counter() - t0) * 1e3)
    assert eng.kv_read(1, 300) == eng.kv_read(0, 300)
    out.update(save_first_ms=save[0], save_ms=statistics.median(save[1:]), restore_first_ms=restore[0],
               restore_ms=statistics.median(restore[1:]))
    del data

    # the kernel alone: all layers in one launch, into / out of one device buffer
    es = 1 if kv != "bf16" else 2
    nb = eng.kv_blocks_total
    table = torch.tensor([[nb if b < 0 else b for b in eng.block_table(0)]], dtype=torch.int32, device="cuda")
    buf = torch.empty(out["bytes"], dtype=torch.uint8, device="cuda")
    layer_bytes = eng.kv_bytes // 2 // cfg.n_layers
    st = torch.cuda.current_stream().cuda_stream
    for unpack in (False, True):
        ms = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            E.kv_snapshot(eng.k_cache_ptr, eng.v_cache_ptr, layer_bytes, buf.data_ptr(), table.data_ptr(), table.shape[1],
                          nb, 0, n, cfg.n_layers, cfg.n_kv_heads, cfg.head_dim, es, unpack, 0, st)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        out["unpack_kernel_ms" if unpack else "pack_kernel_ms"] = statistics.median(ms[1:])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_snapshot.txt"))
    ap.add_argument("--tokens", default="4096,32768")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--no-snapshots", action="store_true")
    a = ap.parse_args()
    L = ["# KV snapshots (Engine.kv_save / kv_restore, aios::kv_snapshot_kernel): tools/kv_snapshot_profile.py on one MI355X.", ""]
    if not a.no_snapshots:
        L += ["## 1. One slot of Mistral-7B Q4_K_M synthetic weights.  save / restore: one call on the host clock, median of 3",
              "##    (first: the engine's first call, which allocates the staging); GB/s of a call: payload / time.  kernel: one",
              "##    launch over all 32 layers on device events; its GB/s: (payload read + payload written) / time.  prefill:",
              "##    the same tokens through Engine.prefill in chunks of 2048, the cost a restore replaces.", ""]
        L.append(f"{'tokens':>7} {'cache':>9} {'payload GB':>10} | {'save ms':>9} {'GB/s':>6} {'first':>9} | {'restore ms':>10} {'GB/s':>6} {'first':>9} |"
                 f" {'pack ms':>8} {'GB/s':>7} {'unpack ms':>9} {'GB/s':>7} | {'prefill ms':>10} {'restore / prefill':>17}")
        for n in [int(x) for x in a.tokens.split(",")]:
            for kv in ("bf16", "fp8_e4m3"):
                r = measure(n, kv)
                gb = r["bytes"] / 1e9
                L.append(f"{n:>7} {kv:>9} {gb:>10.3f} | {r['save_ms']:>9.1f} {gb / r['save_ms'] * 1e3:>6.1f} {r['save_first_ms']:>9.1f} |"
                         f" {r['restore_ms']:>10.1f} {gb / r['restore_ms'] * 1e3:>6.1f} {r['restore_first_ms']:>9.1f} |"
                         f" {r['pack_kernel_ms']:>8.3f} {2 * gb / r['pack_kernel_ms'] * 1e3:>7.0f}"
                         f" {r['unpack_kernel_ms']:>9.3f} {2 * gb / r['unpack_kernel_ms'] * 1e3:>7.0f} |"
                         f" {r['prefill_ms']:>10.1f} {r['restore_ms'] / r['prefill_ms']:>17.3f}")
                print(L[-1], flush=True)
    L += ["", "## 2. Resources (tools/kernel_resources.py --all --grep kv_snapshot; read from the built extension)", ""]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--all", "--grep", "kv_snapshot"],
                       capture_output=True, text=True)
    L += r.stdout.rstrip().splitlines()
    if not a.no_bench:
        L += ["", f"## 3. Headline decode: python bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}, alternating runs", ""]
        trees = ([("parent", a.parent)] if a.parent else []) + [("this", ROOT)]
        if not a.parent:
            L.append("(no --parent checkout given: the parent was not measured in this run)")
        for _ in range(3):
            for k, tree in trees:
                res = bench(tree, a.steps, a.warmup)
                line = f"{k:<8} " + json.dumps({x: res[x] for x in res if isinstance(res[x], (int, float, str))})[:300]
                L.append(line)
                print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
