#!/bin/bash
# fp8 long-context attention workgroups per CU; Q5_K_M / Q8_0 prefill (fallback GEMM); the full bench.py
set -o pipefail
OUT=${AIOS_OUT_DIR:-bench_out}
mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
for w in 2 4; do for p in 16000 32000; do
  AIOS_ATTN_WG_PER_CU=$w timeout -k 10 300 python bench.py --steps 128 --warmup 8 --no-secondary --prompt $p --kv-dtype fp8_e4m3 > "$OUT/wpc.json" 2> "$OUT/lc.err" || { tail -20 "$OUT/lc.err"; exit 1; }
  echo "fp8 wg_per_cu $w prompt $p: $(grep -o '"value": [0-9.]*' "$OUT/wpc.json")"
  AIOS_ATTN_WG_PER_CU=$w timeout -k 10 300 python bench.py --steps 128 --warmup 8 --no-secondary --prompt $p > "$OUT/wpc.json" 2> "$OUT/lc.err" || { tail -20 "$OUT/lc.err"; exit 1; }
  echo "bf16 wg_per_cu $w prompt $p: $(grep -o '"value": [0-9.]*' "$OUT/wpc.json")"
done; done
for r in Q5_K_M Q8_0; do
  timeout -k 10 300 python tools/bench_prefill.py --recipe $r --lens 512,2048 > "$OUT/pf_$r.jsonl" 2> "$OUT/pf.err" || { tail -20 "$OUT/pf.err"; exit 1; }
  cat "$OUT/pf_$r.jsonl"
done
timeout -k 10 900 python bench.py --full > "$OUT/bench_full.json" 2> "$OUT/bench_full.err" || { tail -30 "$OUT/bench_full.err"; exit 1; }
cat "$OUT/bench_full.json"
