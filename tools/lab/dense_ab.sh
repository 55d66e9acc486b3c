#!/bin/bash
# GPU box: default and dense-content (checker) step of library variants (names as for k1ab_env.sh)
for a in "$@"; do
  lib=okvis2_amd/libokvfe_$a.so; [ "$a" = "-" ] && lib=okvis2_amd/libokvfe.so
  for c in corners checker; do
    OKVFE_LIB=$PWD/$lib python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-extras --content $c 2>/dev/null | grep '^{"metric"' | python -c "
import json,sys; r=json.loads(sys.stdin.read()); s=r['stage_ms_per_launch']; print('$a', '$c', 'fps %.0f ms/step %.3f match %.4f'%(r['value'], r['ms_per_step'], s['match']))"
  done
done
