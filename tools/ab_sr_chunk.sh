#!/bin/bash
# Same-box sweep of the estimator's pass size (MOF_SR_CHUNK pairs per pass, the run-time knob):
# does an intermediate that fits the 256 MB Infinity Cache (64 pairs: Zt 118 MB + Dt 59 MB) beat the 512-pair default?
#   usage (GPU box): tools/ab_sr_chunk.sh
set -e
R=${GRAFT_REPO_ROOT:-/root/repo}
for wl in ${WLS:-c5 c5seq}; do
  for chunk in ${CHUNKS:-32 64 128 256 512}; do
    echo "$wl chunk $chunk $(MOF_SR_CHUNK=$chunk python3 $R/bench.py --workload $wl --no-cpu-baseline --no-others --sustain-s 0 --steps 60 --warmup 15 | python3 -c 'import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(round(d["value"]), round(d["ms_per_step"],4))')"
  done
done
