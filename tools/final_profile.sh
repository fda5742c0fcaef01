#!/bin/bash
# End-of-session records (GPU box): the driver-form bench line, the same command under rocprofv3 --kernel-trace --stats, smoke().
# Records are written to $OUT (default build/profile).
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT="${OUT:-build/profile}"
mkdir -p "$OUT"
python bench.py --gpus 1 --steps 20 --warmup 5 --full > "$OUT/final_bench.json" 2> "$OUT/final_bench.err"
rm -rf "$OUT/final_prof"
rocprofv3 --kernel-trace --stats -d "$OUT/final_prof" -o bench640 --output-format csv -- python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline --no-overlap-probe > "$OUT/final_bench_rocprof.json" 2> "$OUT/final_bench_rocprof.err"
find "$OUT/final_prof" -name "*kernel_stats.csv" -exec cp {} "$OUT/final_kernel_stats.csv" \;
find "$OUT/final_prof" -type f ! -name "*kernel_stats.csv" -delete
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/final_smoke.txt" 2>&1
tail -1 "$OUT/final_smoke.txt"
