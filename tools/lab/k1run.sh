python -m pytest tests/test_gpu_parity.py tests/test_gpu_detector_paths.py tests/test_gpu_golden_and_gather.py -x -q 2>&1 | tail -8
for v in "" "OKVFE_K1_TH=31"; do
env $v python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline 2>/dev/null | grep '^{"metric"' | python -c "
import json,sys; r=json.loads(sys.stdin.read()); print(r['value'], r['ms_per_step'], r['roofline']['frac'], r['roofline']['avg_launch_ms'], r['stage_ms_per_launch'])"
done
