#!/usr/bin/env python3
"""Time per launch of the device sampler with a logit bias on (profiles/logit_bias.txt).

The raw op `_engine.sample` on random logits, V = 32000, T = 0.8, top-k 40, top-p 0.95 (the serving defaults), at
B = 1 and B = 8: no processors (`sample_kernel<false>`), penalties over a 64-token window (the processor
instantiation as it was before the bias), a bias list of 1 / 300 / 512 entries, and penalties with a 512-entry
list.  Each figure is device-event time over `--launches` back-to-back launches divided by their number, the
median (and range) of `--repeats` such windows after a warm-up window: launch-to-launch time on one stream, which
is what a decode step pays.  An extension built before the bias existed runs the first two rows only, so the same
script measures the parent commit.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from aios_amd.runtime import native

    E = native.require()
    has_bias = hasattr(E, "SAMPLE_BIAS_MAX")
    V = a.vocab
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    for B in (1, 8):
        logits = (torch.randn(B, V, generator=torch.Generator().manual_seed(B)) * 2).cuda()
        temp = torch.full((B,), 0.8, device="cuda")
        tk = torch.full((B,), 40, dtype=torch.int32, device="cuda")
        tp = torch.full((B,), 0.95, device="cuda")
        pos = torch.arange(B, dtype=torch.int32, device="cuda")
        tok = torch.zeros(B, dtype=torch.int32, device="cuda")
        win = torch.from_numpy(rng.integers(0, V, (B, 64)).astype(np.int32)).cuda()
        rp, pp, fp = (torch.full((B,), x, device="cuda") for x in (1.1, 0.1, 0.1))
        pen = dict(pen_tokens=win.data_ptr(), pen_stride=64, repeat_penalty=rp.data_ptr(),
                   presence_penalty=pp.data_ptr(), frequency_penalty=fp.data_ptr())
        configs = [("no processors", {}), ("penalties (64-token window)", pen)]
        keep = []
        if has_bias:
            for n in (1, 300, 512):
                ids = torch.from_numpy(np.stack([rng.permutation(V)[:n] for _ in range(B)]).astype(np.int32)).cuda()
                vals = torch.from_numpy(rng.uniform(-5, 5, (B, n)).astype(np.float32)).cuda()
                keep += [ids, vals]
                bias = dict(bias_ids=ids.data_ptr(), bias_vals=vals.data_ptr(), bias_stride=n)
                configs.append((f"bias, {n} entries", bias))
            configs.append(("penalties + bias, 512 entries", dict(pen, **bias)))

        def window(kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.launches):
                E.sample(logits.data_ptr(), V, B, V, temp.data_ptr(), tk.data_ptr(), 17 + i, tok.data_ptr(), pos.data_ptr(),
                         0, st, tp.data_ptr(), **kw)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.launches  # us per launch

        for name, kw in configs:
            window(kw)  # warm-up
            us = [window(kw) for _ in range(a.repeats)]
            print(f"{a.label:8s} B={B} V={V} {name:32s} {statistics.median(us):7.2f} us/launch "
                  f"(min {min(us):.2f}, max {max(us):.2f}, {a.repeats} x {a.launches} launches)", flush=True)


if __name__ == "__main__":
    main()
