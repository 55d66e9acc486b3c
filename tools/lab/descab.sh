#!/bin/bash
# GPU box: describe-stage time for library variants x workloads
for wl in euroc mono640; do
for n in "$@"; do
  lib=okvis2_amd/libokvfe_$n.so; [ "$n" = "-" ] && lib=okvis2_amd/libokvfe.so
  OKVFE_LIB=$PWD/$lib python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-extras --workload $wl 2>/dev/null | grep '^{"metric"' | python -c "
import json,sys; r=json.loads(sys.stdin.read()); s=r['stage_ms_per_launch']; print('$wl', '$n', 'ms/step %.3f describe %.3f select %.3f kp/img %s'%(r['ms_per_step'], s['describe'], s['select'], r.get('mean_keypoints_per_image')))"
done
done
