#!/bin/bash
# Alternating same-box A/B of environment settings on the default config-4 bench.
# usage: SETS="PUPIL_NODE_MIN=8 PUPIL_NODE_MIN=12 ..." bash tools/gpu_env_sweep.sh   ("base" = no setting;
# several variables in one set are joined with '+'; the last run's log is kept in $SWEEP_OUT, default build/sweep)
set -u
LOG=${SWEEP_OUT:-build/sweep}/run.log
mkdir -p $(dirname $LOG)
ROUNDS=${ROUNDS:-2}
for r in $(seq 1 $ROUNDS); do
  for s in $SETS; do
    envs=""; [ "$s" != "base" ] && envs="${s//+/ }"
    env $envs timeout -k 10 200 python bench.py --full --cpu-baseline 0 --dropin 0 --steps 10 ${BENCH_ARGS:-} > $LOG 2>&1 || { echo "$s failed"; tail -5 $LOG; exit 1; }
    echo "$r $s $(grep '^{' $LOG | tail -1 | grep -o '"ms_per_step": [0-9.]*') $(grep '^{' $LOG | tail -1 | grep -o '"ms_per_launch": [0-9.]*')"
  done
done
