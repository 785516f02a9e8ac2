#!/bin/bash
# A/B on the config-5 shaped workloads - bench.py's headline / epoch loop and the packed legs (time_blane_pack.py): the parent commit's library against this tree's, fresh
# processes, alternating, N processes each (two processes of ONE library differ by up to 6 %: single pairs decide nothing).
#   [WORKLOADS="synth_er synth_mix"] profiles/tools/blane_pack_ab.sh PARENT_LIB OUT_DIR [N]      then: python profiles/tools/blane_pack_ab_table.py OUT_DIR
# PARENT_LIB: libgtok.so built from the parent commit (profiles/tools/ab_build.sh builds one from a git ref).
# Every process runs under its own time limit; the first failure ends the script.
set -o pipefail
parent=$1; out=$2; n=${3:-5}
mkdir -p "$out"
for wl in ${WORKLOADS:-synth_er synth_mix}; do
  for K in 1 14; do
    for i in $(seq 1 "$n"); do
      for lib in parent branch; do
        if [ $lib = parent ]; then export GTOK_LIB=$parent; else unset GTOK_LIB; fi
        timeout -k 10 300 python bench.py --workload $wl --full --no-cpu-baseline --no-ibtt --no-boundary --epochs-per-launch $K --steps $((4 * K)) \
          2> "$out/${wl}_K${K}_${lib}_$i.err" | tail -1 > "$out/${wl}_K${K}_${lib}_$i.json" || { echo "FAILED $wl K=$K $lib $i"; tail -5 "$out/${wl}_K${K}_${lib}_$i.err"; exit 1; }
        timeout -k 10 300 python profiles/tools/time_blane_pack.py ${wl#synth_} $K 2>> "$out/${wl}_K${K}_${lib}_$i.err" | tail -1 > "$out/legs_${wl}_K${K}_${lib}_$i.json" \
          || { echo "FAILED legs $wl K=$K $lib $i"; tail -5 "$out/${wl}_K${K}_${lib}_$i.err"; exit 1; }
      done
    done
  done
done
echo "A/B done"
