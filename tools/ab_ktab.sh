#!/bin/bash
# Interleaved A/B of the key-table cache on one box: the plain benchmark
# (config 2, `--steps 20 --warmup 5 --dump-outputs`) of this tree, of a parent build's
# library, and of this tree with NT_KTAB_KEYS=0 (the cache off: what the probe-free
# balanced path costs now), `rounds` times each in turn.  Every run's JSON line is kept;
# summary.txt lists host, the rates (M verifies/s), whether the slowest run of this tree
# beats the fastest of the parent by the 2 % adoption bar, and whether the dumped
# verdicts of the last runs are byte-equal.
# Usage (on the GPU box): bash tools/ab_ktab.sh <parent libntcrypto.so> <outdir> [rounds=3] [box label=1]
set -euo pipefail
PARENT=$(readlink -f "$1")
OUT=$2
ROUNDS=${3:-3}
mkdir -p "$OUT"
unset NT_KTAB_KEYS
run() {  # run <name> [VAR=value ...]: one bench run with the given environment, stops the script on failure
  local name=$1
  shift
  env "$@" timeout -k 10 240 python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs "$OUT/$name" \
    > "$OUT/$name.json" 2> "$OUT/$name.err"
}
for r in $(seq 1 "$ROUNDS"); do
  run "new_r$r"
  run "parent_r$r" NTCRYPTO_LIB="$PARENT"
  run "off_r$r" NT_KTAB_KEYS=0
done
{
  echo "box ${4:-1}"
  for k in new parent off; do
    printf "%s" "$k"
    for r in $(seq 1 "$ROUNDS"); do
      python -c "import json,sys; d=json.load(open(sys.argv[1])); print(' %.2f' % (d['value'] / 1e6), end=''); assert d['parity']['mismatches_vs_expected'] == 0" "$OUT/${k}_r$r.json"
    done
    echo
  done
  python - "$OUT" "$ROUNDS" <<'EOF'
import json, sys
out, rounds = sys.argv[1], int(sys.argv[2])
v = lambda k: [json.load(open("%s/%s_r%d.json" % (out, k, r)))["value"] for r in range(1, rounds + 1)]
new, parent = v("new"), v("parent")
print("slowest new / fastest parent: %.4f (adoption bar 1.02: %s)" % (min(new) / max(parent), "met" if min(new) >= 1.02 * max(parent) else "MISSED"))
EOF
  cmp "$OUT/new_r$ROUNDS/verdicts.npy" "$OUT/parent_r$ROUNDS/verdicts.npy" && echo "verdicts new == parent: byte-equal"
  cmp "$OUT/off_r$ROUNDS/verdicts.npy" "$OUT/parent_r$ROUNDS/verdicts.npy" && echo "verdicts off == parent: byte-equal"
} | tee "$OUT/summary.txt"
