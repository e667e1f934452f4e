#!/bin/bash
# tools/ktab_rate.py of this tree and of a parent build's library in turn, `rounds` times, one JSON
# line per run in <outdir>/{new,parent}_r<k>.json, and the medians over all runs side by side.
# Usage (on the GPU box): bash tools/ab_ktab_rate.sh <parent libntcrypto.so> <outdir> [rounds=3]
set -euo pipefail
PARENT=$(readlink -f "$1")
OUT=$2
ROUNDS=${3:-3}
mkdir -p "$OUT"
unset NT_KTAB_KEYS
for r in $(seq 1 "$ROUNDS"); do
  timeout -k 10 240 python tools/ktab_rate.py > "$OUT/new_r$r.json" 2> "$OUT/new_r$r.err"
  NTCRYPTO_LIB="$PARENT" timeout -k 10 240 python tools/ktab_rate.py > "$OUT/parent_r$r.json" 2> "$OUT/parent_r$r.err"
done
python tools/ktab_rate.py --summarize "$OUT" "$ROUNDS" | tee "$OUT/summary.txt"
