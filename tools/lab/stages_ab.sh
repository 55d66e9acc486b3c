#!/bin/bash
# GPU box: per-stage times of library variants (arguments as for k1ab_env.sh)
for a in "$@"; do
  n=${a%%:*}; envs=""; [ "$a" != "$n" ] && envs=$(echo "${a#*:}" | tr ',' ' ')
  lib=okvis2_amd/libokvfe_$n.so; [ "$n" = "-" ] && lib=okvis2_amd/libokvfe.so
  env $envs OKVFE_LIB=$PWD/$lib python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline ${BENCH_ARGS:-} 2>/dev/null | grep '^{"metric"' | python -c "
import json,sys; r=json.loads(sys.stdin.read()); print('$a', 'fps %.0f ms/step %.3f'%(r['value'], r['ms_per_step']), {k: round(v,4) for k,v in r['stage_ms_per_launch'].items() if v is not None})"
done
