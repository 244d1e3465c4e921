#!/bin/bash
# A/B of engine variant libraries on the C5 step (per-kernel times), on the GPU box:
#   VARS="head tc11 tc10" bash tools/nh_ab.sh
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}   # logs of this script
mkdir -p "$OUT"
for v in ${VARS:-}; do
  timeout -k 10 300 env RCMDYN_LIB=varlib/var_$v.so python tools/ktimes.py --config ${CFG:-C5} --steps ${STEPS:-6} --prof-steps ${PSTEPS:-3} > $OUT/nhab_$v.log 2>&1 || { echo "run $v failed"; tail -3 $OUT/nhab_$v.log; exit 3; }
  echo "== $v"; head -${TOP:-6} $OUT/nhab_$v.log; tail -1 $OUT/nhab_$v.log
done
