#!/bin/bash
# GPU box: describe-stage time of the default library under environment variants
# (arguments: ENV=VAL[,ENV=VAL] or "-"; WLS = workloads, default "euroc mono640")
for wl in ${WLS:-euroc mono640}; do
for a in "$@"; do
  envs=""; [ "$a" != "-" ] && envs=$(echo "$a" | tr ',' ' ')
  env $envs python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-extras --workload $wl 2>/dev/null | grep '^{"metric"' | python -c "
import json,sys; r=json.loads(sys.stdin.read()); s=r['stage_ms_per_launch']; print('$wl', '$a', 'ms/step %.3f describe %.3f fps %.0f'%(r['ms_per_step'], s['describe'], r['value']))"
done
done
