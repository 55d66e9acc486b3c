#!/bin/bash
# GPU box: bench line summary for each variant library given (names as for k1variants.sh; "-" = default)
for n in "$@"; do
  lib=okvis2_amd/libokvfe_$n.so; [ "$n" = "-" ] && lib=okvis2_amd/libokvfe.so
  OKVFE_LIB=$PWD/$lib python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline 2>/dev/null | grep '^{"metric"' | python -c "
import json,sys; r=json.loads(sys.stdin.read()); print('$n', 'fps %.0f ms/step %.3f frac %.3f k1_ms %.4f copyGBps %.0f'%(r['value'], r['ms_per_step'], r['roofline']['frac'], r['roofline']['avg_launch_ms'], r['roofline']['copy_kernel_GBps']))"
done
