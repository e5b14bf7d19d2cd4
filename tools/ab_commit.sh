#!/bin/bash
# Same-box A/B of the current tree against an older commit -- the older commit's WHOLE tree (its library, its Python binding, its
# bench.py), so that a change of the C ABI between the two does not matter.
#   where hipcc is (no GPU needed): tools/ab_commit.sh prepare <commit>   exports that commit to tmp_ab/parent/ and builds its library there
#   on the GPU box:                 tools/ab_commit.sh run [bench args...]  alternates old / new, three times (AB_REPS), one line per run:
#                                                                           "<old|new> <pairs/s> <kernel_ms>"
#                                   tools/ab_commit.sh bits                 tools/tail_bits.py's corpus through the old and the new tree (each
#                                                                           library under its own binding), one process each, compared on the CPU
# Nothing is built by `run` or `bits`, and the product library is never overwritten.
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
if [ "$1" == "prepare" ]; then
  rm -rf $R/tmp_ab && mkdir -p $R/tmp_ab/parent
  git -C $R archive $2 | tar -x -C $R/tmp_ab/parent
  make -C $R/tmp_ab/parent/mrs_optic_flow_amd/csrc -s -j${AB_JOBS:-8}
  make -C $R/tmp_ab/parent/oracle -s all
  echo "prepared tmp_ab/parent from $2"; exit 0
fi
if [ "$1" == "bits" ]; then
  [ -f $R/tmp_ab/parent/mrs_optic_flow_amd/libmof_hip.so ] || { echo "run 'tools/ab_commit.sh prepare <commit>' first"; exit 2; }
  O=$(cd ${AB_BITS_DIR:-$R/tmp_ab} && pwd)
  timeout -k 10 ${AB_STEP_LIMIT:-240} python3 $R/tmp_ab/parent/tools/tail_bits.py run $O/bits_old.npz &&
    timeout -k 10 ${AB_STEP_LIMIT:-240} python3 $R/tools/tail_bits.py run $O/bits_new.npz && python3 $R/tools/tail_bits.py compare $O/bits_old.npz $O/bits_new.npz
  exit $?
fi
shift
[ -f $R/tmp_ab/parent/mrs_optic_flow_amd/libmof_hip.so ] || { echo "run 'tools/ab_commit.sh prepare <commit>' first"; exit 2; }
for rep in $(seq 1 ${AB_REPS:-3}); do
  for v in old new; do
    D=$R; [ $v == old ] && D=$R/tmp_ab/parent
    out=$(cd $D && timeout -k 10 ${AB_STEP_LIMIT:-240} python3 bench.py --no-cpu-baseline --no-others --sustain-s 0 --steps 30 "$@" | python3 -c 'import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(round(d["value"]), d["roofline"]["kernel_ms"])') || { echo "$v run failed: stopping"; exit 1; }
    echo "$v $out"
  done
done
