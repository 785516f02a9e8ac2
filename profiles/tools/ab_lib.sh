#!/bin/bash
# A/B of two libraries under the same Python, in one job: the IBTT / text / slab legs with GTOK_LIB=<the parent's libgtok.so> and with
# this tree's library, fresh processes, alternating (the parent first in odd rounds, this tree first in even ones).  Per round and side:
# profiles/tools/time_ibtt_host.py, bench.py --full, bench.py --full --workload synth_er.  Every process runs under its own time limit;
# the first failure ends the script.  (profiles/tools/ab_build.sh builds a library from a git ref.)
#   profiles/tools/ab_lib.sh PARENT_LIB OUT_DIR [ROUNDS]      then: python profiles/tools/ab_lib_table.py OUT_DIR
set -o pipefail
P=$(cd "$(dirname "$1")" && pwd)/$(basename "$1"); out=$2; n=${3:-3}
mkdir -p "$out"
# importing the package rebuilds the library it is pointed at when a source is newer than it: both must count as up to date
touch -d 2030-01-01 "$P" glearning-benchmark_amd/csrc/libgtok.so oracle/*.so
run() {   # name, library or "", command ...
  name=$1; lib=$2; shift 2
  if [ -n "$lib" ]; then GTOK_LIB=$lib timeout -k 10 420 "$@" 2> "$out/$name.err" | tail -1 > "$out/$name.json"
  else timeout -k 10 420 "$@" 2> "$out/$name.err" | tail -1 > "$out/$name.json"; fi
  rc=$?; echo "$name rc=$rc $SECONDS s"; [ $rc = 0 ] || { tail -5 "$out/$name.err"; exit $rc; }
}
for i in $(seq 1 "$n"); do
  if [ $((i % 2)) = 1 ]; then order="parent branch"; else order="branch parent"; fi
  for leg in host full er; do
    case $leg in host) set -- python profiles/tools/time_ibtt_host.py ;; full) set -- python bench.py --gpus 1 --steps 50 --warmup 5 --full ;;
                 er) set -- python bench.py --gpus 1 --steps 50 --warmup 5 --full --workload synth_er ;; esac
    for tree in $order; do
      if [ $tree = parent ]; then run ${leg}_parent_$i "$P" "$@"; else run ${leg}_branch_$i "" "$@"; fi
    done
  done
done
echo "A/B done"
