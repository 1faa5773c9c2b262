#!/bin/bash
# A/B of two builds of libts2d.so on ONE box: bench.py's per-stage HIP-event averages, alternating.  usage: ab_bench.sh [-n ROUNDS] <other.so> [bench args]
# Stops at the first run that fails or hits its timeout (exit status = that run's): nothing more is started on a card that may just have faulted.
R=$(cd "$(dirname "$0")/.." && pwd)
N=2
if [ "$1" = "-n" ]; then N=$2; shift 2; fi
OTHER=$1; shift
ERR=$(mktemp)  # a run's stderr: shown only when the run fails
trap 'rm -f "$ERR"' EXIT
for i in $(seq "$N"); do
  for L in "" "$OTHER"; do
    out=$(TS2D_LIBRARY_PATH=$L timeout -k 10 200 python "$R/bench.py" --no-cpu-baseline "$@" 2>"$ERR")
    rc=$?
    if [ $rc -ne 0 ]; then cat "$ERR" >&2; echo "ab_bench: the run of ${L:-product} failed with exit status $rc" >&2; exit $rc; fi
    printf '%s\n' "$out" | python -c "
import json,sys
j=json.loads(sys.stdin.read().strip().splitlines()[-1]); k=j['kernels_avg_ms']
print('${L:-product}'.split('/')[-1], j['ms_per_step'], ' '.join(f'{a}={b:.4f}' for a,b in k.items()))" || exit $?
  done
done
