#!/bin/bash
# A/B of two whole trees (Python and library): bench.py's headline, `--full` and the zinc_subset workload, run from a checkout of
# the parent commit with its own library built (profiles/tools/ab_build.sh builds one from a git ref) and from this tree, fresh
# processes, alternating (the parent first in odd rounds, the branch first in even ones), N rounds or as many as fit SECONDS of
# wall time (a round is two processes per leg).
#   [LEGS="headline full subset"] profiles/tools/ab_trees.sh PARENT_TREE OUT_DIR [N] [SECONDS]      then: python profiles/tools/ab_trees_table.py OUT_DIR
# Every process runs under its own time limit; the first failure ends the script.
set -o pipefail
parent=$(cd "$1" && pwd); out=$(mkdir -p "$2" && cd "$2" && pwd); n=${3:-3}; budget=${4:-100000}
here=$(cd "$(dirname "$0")/../.." && pwd)
start=$SECONDS; round_s=0
for i in $(seq 1 "$n"); do
  if [ $((SECONDS - start + round_s)) -gt "$budget" ]; then echo "stopping before round $i: no time for it"; break; fi
  t0=$SECONDS
  if [ $((i % 2)) = 1 ]; then order="parent branch"; else order="branch parent"; fi
  for name in ${LEGS:-headline full subset}; do
    case $name in headline) set -- ;; full) set -- --full ;; subset) set -- --workload zinc_subset ;; *) echo "unknown leg $name"; exit 1 ;; esac
    for tree in $order; do
      if [ $tree = parent ]; then dir=$parent; else dir=$here; fi
      (cd "$dir" && timeout -k 10 420 python bench.py --gpus 1 --steps 50 --warmup 5 "$@" 2> "$out/${name}_${tree}_$i.err" | tail -1 > "$out/${name}_${tree}_$i.json") \
        || { echo "FAILED $name $tree $i"; tail -5 "$out/${name}_${tree}_$i.err"; exit 1; }
      echo "$name $tree $i: $((SECONDS - start)) s"
    done
  done
  round_s=$((SECONDS - t0))
done
echo "A/B done"
