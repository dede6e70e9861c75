#!/bin/bash
# A/B harness: bench.py against the in-tree libuavx.so and every alternative build in tools/ab/*.so (UAVX_LIB), alternating
# per repetition.  REPS repetitions (default 2); every bench run has its own time limit (STEP_TIMEOUT seconds, default 300)
# and the first one that fails, faults or runs out of time ends the script: nothing else is started on that GPU.
# usage: [REPS=3] tools/ab_run.sh [bench.py args]
set -o pipefail
cd "$(dirname "$0")/.."
shopt -s nullglob
for rep in $(seq 1 "${REPS:-2}"); do
for so in gym_uav_collision_avoidance_amd/csrc/libuavx.so tools/ab/*.so; do
  UAVX_LIB=$PWD/$so timeout -k 10 "${STEP_TIMEOUT:-300}" python bench.py --steps 2000 --warmup 200 --no-cpu-baseline --no-large "$@" 2>/dev/null \
    | python tools/benchline.py "$so rep $rep" || { echo "ab_run: $so rep $rep failed (exit $?)"; exit 1; }
done
done
