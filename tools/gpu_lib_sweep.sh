#!/bin/bash
# Alternating same-box A/B of several builds of libpupil_pt.so on the default config-4 bench.
# usage: LIBS="default build/ab_base/libpupil_pt.so build/ab_x/libpupil_pt.so,PUPIL_NODE_MIN=16 ..." bash tools/gpu_lib_sweep.sh
# (the last run's log is kept in $SWEEP_OUT, default build/sweep)
set -u
LOG=${SWEEP_OUT:-build/sweep}/run.log
mkdir -p $(dirname $LOG)
ROUNDS=${ROUNDS:-2}
for r in $(seq 1 $ROUNDS); do
  for l in $LIBS; do
    # token: <lib path or "default">[,VAR=value...]
    IFS=',' read -r path extra <<< "$l"
    if [ "$path" = "default" ]; then lib=""; else lib="PUPIL_LIB=$path"; fi
    env $lib ${extra//,/ } timeout -k 10 200 python bench.py --full --cpu-baseline 0 --dropin 0 --steps 10 ${BENCH_ARGS:-} > $LOG 2>&1 || { echo "$l failed"; tail -5 $LOG; exit 1; }
    line=$(grep '^{' $LOG | tail -1)
    echo "$r $l $(echo "$line" | grep -o '"ms_per_step": [0-9.]*') $(echo "$line" | grep -o '"ms_per_launch": [0-9.]*') $(echo "$line" | grep -o '"avg_node_visits_per_ray": [0-9.]*') $(echo "$line" | grep -o '"bvh_build_ms": [0-9.]*') $(echo "$line" | grep -o '"instance_update_ms": [^}]*}')"
  done
done
