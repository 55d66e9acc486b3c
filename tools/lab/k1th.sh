#!/bin/bash
# GPU box: bench summary of the default library for several OKVFE_K1_TH settings
for th in "$@"; do
  OKVFE_LIB=$PWD/okvis2_amd/libokvfe_lab.so OKVFE_K1_TH=$th python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline 2>/dev/null | grep '^{"metric"' | python -c "
import json,sys; r=json.loads(sys.stdin.read()); print('TH', '$th', 'fps %.0f ms/step %.3f frac %.3f k1_ms %.4f'%(r['value'], r['ms_per_step'], r['roofline']['frac'], r['roofline']['avg_launch_ms']))"
done
