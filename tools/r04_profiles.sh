#!/bin/bash
# Round-4 records in ONE gpurun call: driver-form bench + the same command under rocprofv3 --kernel-trace --stats + smoke (final_profile.sh),
# the two --pmc passes over the layer's four prefill GEMM launches (separate runs: FETCH_SIZE and WRITE_SIZE do not fit one pass), the side lines.
# Records are written to $OUT (default build/profile).
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export OUT="${OUT:-build/profile}"
mkdir -p "$OUT"
bash tools/final_profile.sh
rm -rf "$OUT/pmcF" "$OUT/pmcW"
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d "$OUT/pmcF" -o f -- python3 tools/pmc_gemm.py > "$OUT/pmcF.log" 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d "$OUT/pmcW" -o w -- python3 tools/pmc_gemm.py > "$OUT/pmcW.log" 2>&1
python tools/pmc_summary.py $(find "$OUT/pmcF" -name "*.db") $(find "$OUT/pmcW" -name "*.db") "$OUT/r04_pmc_gemm.json" > "$OUT/r04_pmc_gemm.txt" 2>&1 || true
rm -rf "$OUT/pmcF" "$OUT/pmcW"
echo "pmc done"; cat "$OUT/r04_pmc_gemm.txt"
python bench.py --ragged --steps 20 --warmup 5 --full --no-overlap-probe > "$OUT/r04_bench_ragged.json" 2> "$OUT/r04_side.err"
python bench.py --full --no-overlap-probe > "$OUT/r04_bench_default64.json" 2>> "$OUT/r04_side.err"
python bench.py --config llama3-8b-fp8 --steps 8 --warmup 2 --full > "$OUT/r04_bench_llama3_fp8.json" 2>> "$OUT/r04_side.err"
python bench.py --config llama3-8b-bf16 --steps 8 --warmup 2 --full > "$OUT/r04_bench_llama3_bf16.json" 2>> "$OUT/r04_side.err"
python bench.py --config finetune-tinyllama --steps 16 --warmup 2 > "$OUT/r04_bench_finetune.json" 2>> "$OUT/r04_side.err"
echo "side lines done"
