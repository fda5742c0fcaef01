#!/bin/bash
# bench.py at several --prefill-batches (packed prefill launches of 32 x pb prompts), driver form; one line per run
set -o pipefail
for pb in "$@"; do
    python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-overlap-probe --prefill-batches $pb | python -c "
import json, sys
r=json.loads(sys.stdin.read().strip().splitlines()[-1])
print($pb, round(r['value'],1), round(r['roofline']['frac'],4), round(r['phases']['prefill_ms_per_step'],2), round(r['phases']['decode_ms_per_step'],2))" || exit 1
done
