#!/bin/bash
# round-6 end validation, part 2: the full bench.py line (all secondaries)
set -o pipefail
OUT=${AIOS_OUT_DIR:-bench_out}
mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 1100 python bench.py --full > "$OUT/bench_final.json" 2> "$OUT/bench_final.err" || { tail -30 "$OUT/bench_final.err"; exit 1; }
cat "$OUT/bench_final.json"
