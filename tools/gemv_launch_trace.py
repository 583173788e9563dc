#!/usr/bin/env python3
"""One GEMV launch per case, nothing checked: the launch record behind tests/data/gemv_plan_golden.json.

Run it under a kernel trace; every case that launches contributes exactly one `gemv_*` kernel to the
trace, in order, and `--reduce` joins the trace with the case list:

  timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d OUT -- \\
      python tools/gemv_launch_trace.py --cases OUT/cases.json
  python tools/gemv_launch_trace.py --reduce OUT --cases OUT/cases.json --out tests/data/gemv_plan_golden.json \\
      --note "parent <commit>, <machine>"

(The run takes a few seconds; the time limit ends it if a launch hangs.)  Two builds launch the same
kernels when their reduced files are equal (`--so` loads another build's extension).  Weight
contents are irrelevant (zeros); buffers are shared by all cases.
"""
import argparse
import csv
import glob
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bytes per block / weights per block of the GGUF layouts QMatrix takes
RAW = {"Q4_K": (144, 256), "Q5_K": (176, 256), "Q6_K": (210, 256), "Q4_0": (18, 32), "Q8_0": (34, 32), "BF16": (2, 1)}
MODELS = {  # d_model, q rows, k / v rows, d_ff, vocab
    "mistral": (4096, 4096, 1024, 14336, 32000),
    "tinyllama": (2048, 2048, 256, 5632, 32000),
}
STORE, RESID, SWIGLU = 0, 1, 2


def projections(model, fmt="Q4_K", fmt_hi="Q6_K"):
    """name -> (segments [(format, rows)], K, epilogue) of a Q4_K_M file (fmt_hi: V, down, lm_head)."""
    d, q, kv, ff, vocab = MODELS[model]
    return {
        "qkv_mixed": ([(fmt, q), (fmt, kv), (fmt_hi, kv)], d, STORE),
        "qkv": ([(fmt, q), (fmt, kv), (fmt, kv)], d, STORE),
        "o": ([(fmt, d)], q, RESID),
        "gate_up": ([(fmt, 2 * ff)], d, SWIGLU),
        "down": ([(fmt_hi, d)], ff, RESID),
        "down_lo": ([(fmt, d)], ff, RESID),
        "lm_head": ([(fmt_hi, vocab)], d, STORE),
    }


def cases():
    out = []

    def add(model, proj, segs, K, epi, B, **kw):
        c = dict(model=model, proj=proj, segs=[[f, r] for f, r in segs], K=K, epi=epi, B=B, act_q8=1, force_v1=0,
                 kernel_sel=0, tune_grid=0, x16=0, y16=0)
        c.update(kw)
        out.append(c)

    for model in MODELS:
        for proj, (segs, K, epi) in projections(model).items():
            for B in (1, 2, 3, 4, 8):
                add(model, proj, segs, K, epi, B)
                add(model, proj, segs, K, epi, B, act_q8=0)
                add(model, proj, segs, K, epi, B, force_v1=1)
                for sel in (1, 2, 3):
                    add(model, proj, segs, K, epi, B, kernel_sel=sel)
                for tg in (3, 37):
                    add(model, proj, segs, K, epi, B, tune_grid=tg)
        # the bf16 hand-off between gate/up (SwiGLU output) and down (input)
        p = projections(model)
        for B in (1, 2, 3, 4):
            add(model, "gate_up", *p["gate_up"], B, y16=1)
            add(model, "down", *p["down"], B, x16=1)
    for fmt, model in (("Q5_K", "mistral"), ("Q4_0", "tinyllama"), ("Q8_0", "tinyllama"), ("BF16", "tinyllama")):
        segs, K, epi = projections(model, fmt, fmt)["gate_up"]
        for B in (1, 2, 3, 4, 8):
            add(model, "gate_up", segs, K, epi, B)
            add(model, "gate_up", segs, K, epi, B, act_q8=0)
    return out


def load_engine(so):
    import torch  # noqa: F401  (first: one HIP runtime per process, aios_amd/runtime/native.py)

    if not so:
        from aios_amd.runtime import native

        return native.require()
    spec = importlib.util.spec_from_file_location("_engine", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(args):
    import numpy as np
    import torch

    E = load_engine(args.so)
    cs = cases()
    mats = {}

    def mat(fmt, rows, K):
        if (fmt, rows, K) not in mats:
            nbytes, per = RAW[fmt]
            mats[(fmt, rows, K)] = E.QMatrix(getattr(E, "QT_" + fmt), rows, K, np.zeros(rows * (K // per) * nbytes, np.uint8))
        return mats[(fmt, rows, K)]

    nmax = 8 * max(sum(r for _, r in c["segs"]) for c in cs)
    kmax = 8 * max(c["K"] for c in cs)
    x = torch.zeros(kmax, dtype=torch.float32, device="cuda")
    x16 = torch.zeros(kmax, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(nmax, dtype=torch.float32, device="cuda")
    y16 = torch.zeros(nmax, dtype=torch.bfloat16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    cus = E.device_cu_count()
    torch.cuda.synchronize()
    for c in cs:
        segs = [mat(f, r, c["K"]) for f, r in c["segs"]]
        N = sum(r for _, r in c["segs"])
        ldy = N // 2 if c["epi"] == SWIGLU else N
        try:
            E.gemv(segs, c["B"], x.data_ptr(), c["K"], 0, 1e-5, y.data_ptr(), ldy, c["epi"], st, force_v1=c["force_v1"],
                   act_q8=c["act_q8"], tune_grid=c["tune_grid"], kernel_sel=c["kernel_sel"],
                   x16=x16.data_ptr() if c["x16"] else 0, y16=y16.data_ptr() if c["y16"] else 0)
            c["launched"] = 1
        except RuntimeError as e:
            c["launched"] = 0
            c["error"] = str(e)
        torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.cases)), exist_ok=True)
    with open(args.cases, "w") as f:
        json.dump({"cus": cus, "device": E.device_name(0), "cases": cs}, f)
    print(f"{len(cs)} cases, {sum(c['launched'] for c in cs)} launched, {cus} CUs")


def reduce(args):
    rec = json.load(open(args.cases))
    rows = []
    for path in sorted(glob.glob(os.path.join(args.reduce, "**", "*kernel_trace.csv"), recursive=True)):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "gemv_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    launched = [c for c in rec["cases"] if c["launched"]]
    if len(rows) != len(launched):
        sys.exit(f"{len(rows)} gemv kernels in the trace, {len(launched)} launched cases")
    for c, r in zip(launched, rows):
        name = r["Kernel_Name"]
        c["kernel"] = name[name.index("gemv_"):name.index(">") + 1] if ">" in name else name
        c["grid_x"] = int(r["Grid_Size_X"])
        c["wg_x"] = int(r["Workgroup_Size_X"])
        c["lds"] = int(r["LDS_Block_Size"])
    out = {"note": args.note, "cus": rec["cus"], "device": rec["device"], "cases": rec["cases"]}
    with open(args.out, "w") as f:
        f.write("{\n")
        for k in ("note", "cus", "device"):
            f.write(f' "{k}": {json.dumps(out[k])},\n')
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in out["cases"]) + "\n ]\n}\n")
    print(f"{args.out}: {len(rows)} launches")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--so", default=None, help="extension file of another build (default: this tree's)")
    ap.add_argument("--cases", required=True, help="JSON of the cases as issued (written by the run, read by --reduce)")
    ap.add_argument("--reduce", metavar="DIR", default=None, help="join the kernel trace under DIR with --cases")
    ap.add_argument("--out", default=None)
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    reduce(a) if a.reduce else run(a)
