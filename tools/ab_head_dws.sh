#!/bin/bash
# On the GPU box: MobileNet-V1 at batch 128 with and without fuse_head_dws (environment seeds of a new handle), as two pairs — over the default plan
# and over the fuse_dws plan: bench value, unpipelined value and summed kernel time, interleaved REPS times (boxes drift), then the per-launch times
# of the first launches of every setting (the head position).  Every run has its own time limit and the first one that fails ends the script.
#   tools/ab_head_dws.sh   (REPS default 3, STEPS default 150)
set -o pipefail
REPS=${REPS:-3}; STEPS=${STEPS:-150}
SETS=("F8_FUSE_DWS=0 F8_FUSE_DWS7=0 F8_FUSE_HEAD_DWS=0" "F8_FUSE_DWS=0 F8_FUSE_DWS7=0 F8_FUSE_HEAD_DWS=1"
      "F8_FUSE_DWS=1 F8_FUSE_DWS7=0 F8_FUSE_HEAD_DWS=0" "F8_FUSE_DWS=1 F8_FUSE_DWS7=0 F8_FUSE_HEAD_DWS=1")
for r in $(seq 1 $REPS); do
  for e in "${SETS[@]}"; do
    env $e timeout -k 10 300 python bench.py --arch mobilenet_v1 --bs 128 --steps $STEPS --warmup 20 --no-cpu-baseline 2>/dev/null |
      python -c "import json,sys; d=json.loads(sys.stdin.read()); print('rep $r  $e  img/s', d['value'], 'unpipelined', d['value_unpipelined'], 'sum_kernel_ms', d['whole_net']['sum_kernel_ms'])" || exit 1
  done
done
for e in "${SETS[@]}"; do
  echo "== per launch (us), $e"
  env $e F8_BENCH_LEAN=1 timeout -k 10 300 python bench.py --arch mobilenet_v1 --bs 128 --steps $STEPS --warmup 20 --per-layer --no-cpu-baseline 2>&1 >/dev/null |
    grep -E "^ +[0-9]+ .*(${PAT:-input|head|stage_0_layer_0|stage_1_layer_0})" | cut -c1-150 || exit 1
done
