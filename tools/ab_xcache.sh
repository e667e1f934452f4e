#!/bin/bash
# Interleaved A/B of the x cache on one box: the plain benchmark
# (config 2, `--steps 20 --warmup 5 --dump-outputs`) of this tree, of a parent
# build's library, and of this tree with NT_XCACHE_SLOTS=1 (one slot: essentially
# every probe misses -- the price of a cold key), `rounds` times each in turn.
# Every run's JSON line is kept; summary.txt lists host, the rates (M verifies/s)
# and whether the dumped verdicts of the last pair are byte-equal.
# Usage (on the GPU box): bash tools/ab_xcache.sh <parent libntcrypto.so> <outdir> [rounds=3]
set -euo pipefail
PARENT=$(readlink -f "$1")
OUT=$2
ROUNDS=${3:-3}
mkdir -p "$OUT"
unset NT_XCACHE_SLOTS
run() {  # run <name> [VAR=value ...]: one bench run with the given environment, stops the script on failure
  local name=$1
  shift
  env "$@" timeout -k 10 240 python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs "$OUT/$name" \
    > "$OUT/$name.json" 2> "$OUT/$name.err"
}
for r in $(seq 1 "$ROUNDS"); do
  run "new_r$r"
  run "parent_r$r" NTCRYPTO_LIB="$PARENT"
  run "miss_r$r" NT_XCACHE_SLOTS=1
done
{
  echo "host $(hostname) gpu $( (rocm-smi --showuniqueid 2>/dev/null | grep -m1 -o '0x[0-9a-f]*') || echo unknown)"
  for k in new parent miss; do
    printf "%s" "$k"
    for r in $(seq 1 "$ROUNDS"); do
      python -c "import json,sys; d=json.load(open(sys.argv[1])); print(' %.2f' % (d['value'] / 1e6), end=''); assert d['parity']['mismatches_vs_expected'] == 0" "$OUT/${k}_r$r.json"
    done
    echo
  done
  cmp "$OUT/new_r$ROUNDS/verdicts.npy" "$OUT/parent_r$ROUNDS/verdicts.npy" && echo "verdicts new == parent: byte-equal"
  cmp "$OUT/miss_r$ROUNDS/verdicts.npy" "$OUT/parent_r$ROUNDS/verdicts.npy" && echo "verdicts miss == parent: byte-equal"
} | tee "$OUT/summary.txt"
