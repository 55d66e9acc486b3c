#!/bin/bash
# GPU box: parity suite + default bench line summary (+ optional select stats)
python -m pytest tests -m gpu -x -q 2>&1 | grep -E "passed|failed|Error|error|assert" | tail -8
python bench.py --full --steps 20 --no-cpu-baseline ${BENCH_ARGS:-} 2>/dev/null | grep '^{"metric"' | python -c "
import json,sys; r=json.loads(sys.stdin.read()); print(r['value'], r['ms_per_step'], r['roofline']['frac']); print(r['stage_ms_per_launch']); print(r['dense_content'])"
