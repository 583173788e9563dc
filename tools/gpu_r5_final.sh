#!/bin/bash
# round-5 validation: every GPU test, smoke(), decode profiles (Mistral, TinyLlama), long-context bench
set -o pipefail
OUT=${AIOS_OUT_DIR:-bench_out}
mkdir -p "$OUT"
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 1500 python -u -m pytest -x -q --timeout 900 --timeout-method thread -m gpu tests > "$OUT/t_final.log" 2>&1 || { tail -40 "$OUT/t_final.log"; exit 1; }
tail -n 1 "$OUT/t_final.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke.log" 2>&1 || { tail -20 "$OUT/smoke.log"; exit 1; }
tail -n 1 "$OUT/smoke.log"
timeout -k 10 1100 python bench.py --full > "$OUT/bench_final.log" 2>&1 || { tail -20 "$OUT/bench_final.log"; exit 1; }
grep '^{"metric"' "$OUT/bench_final.log" | tail -1 | cut -c1-300
