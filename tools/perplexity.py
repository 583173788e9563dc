#!/usr/bin/env python3
"""Perplexity and configuration deltas through Engine.score_prefill.

Scores non-overlapping windows of --ctx tokens (each window from position 0 of a slot, its last row unscored)
and prints ONE JSON line: perplexity = exp(-mean lp), tokens scored, seconds.  With --compare KEY=VALUE a
second engine is built on the same weights with that one setting changed (kv_dtype, kv_calibrate, act_q8) and
the line also carries, between the two engines over the same positions: mean and max |delta lp|, the share of
positions whose `best` (argmax) agrees, and the perplexity ratio.

    python tools/perplexity.py --model mistral-7b --tokens 2048 --ctx 2048 --compare kv_dtype=fp8_e4m3

--model is a preset (random-init weights generated on the GPU from --seed: the perplexity itself is about V
and means nothing, only the deltas between configurations do) or a .gguf file.  Tokens: --tokens N random
ids (seeded), --ids file.npy, or --text file (a .gguf model's own tokenizer; presets use the synthetic
vocabulary).  --timing adds score_prefill against prefill at 128 / 512 / 2048 tokens and the row-scoring
kernel's time per launch.  Parity with llama-perplexity is not pinned.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COMPARE_KEYS = ("kv_dtype", "kv_calibrate", "act_q8")


def parse_compare(items):
    out = {}
    for it in items or []:
        k, sep, v = it.partition("=")
        if not sep or k not in COMPARE_KEYS:
            raise SystemExit(f"--compare takes KEY=VALUE with KEY in {COMPARE_KEYS}, got {it!r}")
        out[k] = (v.lower() not in ("0", "false", "off", "no")) if k == "act_q8" else v
    return out


def preset_tokenizer(cfg):
    from aios_amd.models.synthetic import synthetic_vocab
    from aios_amd.runtime.tokenizer import SpmTokenizer

    t, s, ty = synthetic_vocab(cfg.vocab_size)
    return SpmTokenizer(t, s, ty, cfg.bos_id, cfg.eos_id)


def build(args, over):
    """(engine, ModelConfig, tokenizer factory) for the base settings with `over` applied"""
    from aios_amd.models.config import get_preset
    from aios_amd.runtime.loader import load_engine, random_engine

    s = dict(kv_dtype=args.kv_dtype, kv_calibrate=args.kv_calibrate, act_q8=not args.fp32_act)
    s.update(over)
    cal = None if s["kv_calibrate"] in (None, "off") else s["kv_calibrate"]
    if args.model.endswith(".gguf"):
        eng, cfg, r = load_engine(args.model, max_ctx=args.ctx, max_slots=1, max_batch=1, act_q8=s["act_q8"],
                                  kv_dtype=s["kv_dtype"], kv_calibrate=cal)

        def tok():
            from aios_amd.runtime.tokenizer import from_gguf

            return from_gguf(r)
    else:
        cfg = get_preset(args.model)
        tok = lambda: preset_tokenizer(cfg)  # noqa: E731
        eng = random_engine(cfg, args.recipe, seed=args.seed, max_ctx=args.ctx, max_slots=1, max_batch=1,
                            act_q8=s["act_q8"], kv_dtype=s["kv_dtype"], kv_calibrate=cal,
                            tokenizer=tok() if cal == "auto" else None)
    return eng, cfg, tok, s


def token_ids(args, cfg, tok):
    if args.ids:
        ids = [int(t) for t in np.load(args.ids).reshape(-1)]
    elif args.text:
        with open(args.text, encoding="utf-8") as f:
            ids = tok().encode(f.read(), add_bos=True, parse_special=False)
    else:
        ids = [int(t) for t in np.random.default_rng(args.seed).integers(3, cfg.vocab_size, args.tokens)]
        ids[0] = cfg.bos_id
    if any(not 0 <= t < cfg.vocab_size for t in ids):
        raise SystemExit(f"token id outside [0, {cfg.vocab_size})")
    if len(ids) < 2:
        raise SystemExit("at least 2 tokens are needed")
    return ids


def score(eng, ids, ctx):
    """(lp [n], best [n], seconds) over the windows' scored positions"""
    lps, bests = [], []
    t0 = time.perf_counter()
    for a in range(0, len(ids), ctx):
        w = ids[a:a + ctx]
        if len(w) < 2:
            break
        sc = eng.score_prefill(0, w, 0, -1, 0, False)
        lps.append(np.asarray(sc["lp"][:-1], np.float64))
        bests.append(np.asarray(sc["best"][:-1]))
    return np.concatenate(lps), np.concatenate(bests), time.perf_counter() - t0


def summary(lp, sec):
    finite = np.isfinite(lp)
    return {"perplexity": float(np.exp(-np.mean(lp[finite]))) if finite.any() else float("nan"),
            "tokens_scored": int(lp.size), "nonfinite": int((~finite).sum()), "seconds": round(sec, 4)}


def timing(eng, cfg, ctx, seed):
    """score_prefill against prefill of the same tokens, and the row-scoring kernel alone"""
    import torch

    from aios_amd.runtime import native

    out = {"score_vs_prefill_ms": {}}
    for T in (128, 512, 2048):
        if T > ctx:
            continue
        ids = [int(t) for t in np.random.default_rng(seed + T).integers(3, cfg.vocab_size, T)]
        row = {}
        for name, fn in (("prefill", lambda: eng.prefill(0, ids, 0, True)),
                         ("score_prefill", lambda: eng.score_prefill(0, ids, 0, -1, 0, True)),
                         ("score_prefill_top5", lambda: eng.score_prefill(0, ids, 0, -1, 5, True))):
            fn()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            row[name] = round(float(np.median(ts)), 3)
        out["score_vs_prefill_ms"][str(T)] = row
    E = native.require()
    R, V = eng.score_group_rows(), cfg.vocab_size
    logits = torch.randn(R, V, device="cuda")
    tg = torch.randint(0, V, (R,), dtype=torch.int32, device="cuda")
    f = torch.zeros(R, 2, device="cuda")
    i = torch.zeros(R, 2, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    run = lambda: E.score_rows(logits.data_ptr(), V, R, V, tg.data_ptr(), f.data_ptr(), i.data_ptr(), st)  # noqa: E731
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / n
    out["score_rows_kernel"] = {"rows": R, "V": V, "us_per_launch": round(us, 2),
                                "GB_per_s": round(R * V * 4 / us / 1e3, 1)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="mistral-7b", help="preset name or file.gguf")
    ap.add_argument("--recipe", default="Q4_K_M")
    ap.add_argument("--kv-dtype", default="bf16", help="bf16 or fp8_e4m3")
    ap.add_argument("--kv-calibrate", default="off", help='fp8 KV scales: "off" (1.0) or "auto"')
    ap.add_argument("--fp32-act", action="store_true", help="fp32 GEMV activations (act_q8 off)")
    ap.add_argument("--ctx", type=int, default=2048, help="window length = the engine's context")
    ap.add_argument("--tokens", type=int, default=2048, help="random token ids to score")
    ap.add_argument("--ids", help=".npy file of token ids")
    ap.add_argument("--text", help="text file, tokenised with the model's tokenizer")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--compare", action="append", metavar="KEY=VALUE",
                    help=f"build a second engine with this setting changed; KEY in {COMPARE_KEYS} (repeatable)")
    ap.add_argument("--timing", action="store_true", help="score_prefill vs prefill and the kernel's time")
    args = ap.parse_args(argv)
    over = parse_compare(args.compare)

    eng, cfg, tok, settings = build(args, {})
    ids = token_ids(args, cfg, tok)
    lp, best, sec = score(eng, ids, args.ctx)
    out = {"model": cfg.name, "recipe": args.recipe, "ctx": args.ctx, "settings": settings, **summary(lp, sec)}
    if args.timing:
        out["timing"] = timing(eng, cfg, args.ctx, args.seed)
    if over:
        del eng  # (one engine at a time on the device)
        eng2, _, _, s2 = build(args, over)
        lp2, best2, sec2 = score(eng2, ids, args.ctx)
        both = np.isfinite(lp) & np.isfinite(lp2)
        d = np.abs(lp - lp2)[both]
        a, b = summary(lp, sec), summary(lp2, sec2)
        out["compare"] = {"settings": s2, **b,
                          "mean_abs_dlp": float(d.mean()) if d.size else float("nan"),
                          "max_abs_dlp": float(d.max()) if d.size else float("nan"),
                          "best_agreement": float(np.mean(best == best2)),
                          "perplexity_ratio": b["perplexity"] / a["perplexity"]}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
