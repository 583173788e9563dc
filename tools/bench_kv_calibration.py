#!/usr/bin/env python3
"""Load-time cost of the fp8 KV calibration (`kv_calibrate = "auto"`), beside tools/bench_load.py.

The calibration is one prefill of the built-in prompt (min(256, max_ctx / 2) tokens) with the KV
writers' observer on, a copy of the n_layers x 2 x n_kv_heads table and the scale computation; it
does not depend on how the weights got into HBM, so the synthetic engine (random weights generated
on the device) measures it: the time of the first calibration of a fresh engine (what a load pays,
lazy first-use costs of the prefill path included), a second one (the steady cost), and for scale an
ordinary prefill of the same tokens.

  python tools/bench_kv_calibration.py [--model mistral-7b] [--recipe Q4_K_M] [--ctx 4096] [--json out.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--recipe", default="Q4_K_M")
    ap.add_argument("--ctx", type=int, default=4096)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    from aios_amd.models.config import get_preset
    from aios_amd.models.synthetic import synthetic_vocab
    from aios_amd.runtime import kv_calibration
    from aios_amd.runtime.loader import random_engine
    from aios_amd.runtime.tokenizer import SpmTokenizer

    cfg = get_preset(args.model)
    toks, scores, types = synthetic_vocab(cfg.vocab_size)
    tok = SpmTokenizer(toks, scores, types, cfg.bos_id, cfg.eos_id)
    t = time.time()
    eng = random_engine(cfg, args.recipe, seed=1, max_ctx=args.ctx, max_slots=4, max_batch=8, kv_dtype="fp8_e4m3")
    eng.synchronize()
    build_s = time.time() - t
    t = time.time()
    ids = kv_calibration.auto_tokens(tok, eng.config.max_ctx)
    tokenize_s = time.time() - t
    t = time.time()
    scales = kv_calibration.calibrate(eng, ids)
    first_s = time.time() - t
    t = time.time()
    kv_calibration.calibrate(eng, ids)
    second_s = time.time() - t
    t = time.time()
    eng.prefill(0, ids, 0, False)
    prefill_s = time.time() - t
    eng.release_slot(0)
    row = {"bench": "fp8 kv calibration", "model": args.model, "recipe": args.recipe, "max_ctx": eng.config.max_ctx,
           "tokens": len(ids), "engine_build_s": round(build_s, 3), "tokenize_s": round(tokenize_s, 4),
           "calibrate_first_s": round(first_s, 4), "calibrate_again_s": round(second_s, 4),
           "plain_prefill_s": round(prefill_s, 4),
           "k_scale_min_max": [min(scales[0::2]), max(scales[0::2])],
           "v_scale_min_max": [min(scales[1::2]), max(scales[1::2])]}
    print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
