#!/bin/bash
# r05y: the round's final tree. The whole GPU suite, 600 seeded random solves (new seed), bench.py with the driver's
# flags twice, its rocprofv3 kernel-trace summary, one 512^3 Newton solve's per-iteration kernel split, the level-0
# PMC of the LINEAR and NEWTON_B kernels (separate counter passes), and a 1023^3 Newton iteration (config #5's grid).
set -o pipefail
OUT=gpurun_out/${1:-r05y}
mkdir -p "$OUT"
export TMPDIR=/tmp
step() { echo "[$(date +%T)] $*"; }
fatal() { [ "$1" -ge 124 ] && { echo "fatal rc=$1"; exit 1; }; return 0; }
step pytest-gpu-full
timeout -k 10 900 python -u -m pytest tests -m gpu -q --timeout 300 --timeout-method thread --maxfail 20 > "$OUT/pytest.log" 2>&1; rc=$?
tail -3 "$OUT/pytest.log"; fatal $rc
step fuzz
GS_FUZZ_N=600 GS_FUZZ_SEED=20261024 timeout -k 10 900 python -u -m pytest tests/test_gpu_fuzz.py -m gpu -q --timeout 900 --timeout-method thread > "$OUT/fuzz.log" 2>&1; rc=$?
tail -2 "$OUT/fuzz.log"; fatal $rc
step bench-driver-flags
for r in 1 2; do
  timeout -k 10 400 python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$OUT/bench_r$r.json" 2> "$OUT/bench_r$r.err" || { tail -20 "$OUT/bench_r$r.err"; exit 1; }
  python tools/bench_brief.py "$OUT/bench_r$r.json" || true
done
step bench-rocprof-stats
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof_bench" -o run --output-format csv -- \
    python bench.py --full --steps 20 --warmup 5 --cpu-sweeps 0 > "$OUT/prof_bench.json" 2> "$OUT/prof_bench.err" || { tail -20 "$OUT/prof_bench.err"; exit 1; }
python tools/kernel_agg.py "$(find $OUT/prof_bench -name '*kernel_trace.csv' -print -quit)" > "$OUT/prof_bench_agg.txt" && head -12 "$OUT/prof_bench_agg.txt"
step newton-seq
timeout -k 10 400 rocprofv3 --kernel-trace -d "$OUT/prof_n" -o run --output-format csv -- \
    python bench.py --full --steps 2 --warmup 2 --ramp-ms 0 --cpu-sweeps 0 --vcycles 0 --config5 0 --newton-iters 2 > "$OUT/n512.json" 2> "$OUT/n512.err" || { tail -20 "$OUT/n512.err"; exit 1; }
python tools/trace_seq.py "$(find $OUT/prof_n -name '*kernel_trace.csv' -print -quit)" -4 --agg > "$OUT/n512_seq.txt" && head -22 "$OUT/n512_seq.txt"
step pmc-level0
bash tools/pmc_run.sh r05y/kprobe tools/newton_kprobe.py 1 3 512 > "$OUT/pmc_kprobe.log" 2>&1 || { tail -30 "$OUT/pmc_kprobe.log"; exit 1; }
python tools/pmc_level0.py "$OUT/kprobe/pmc" 134217728 "k_rr2<0=17" "k_rr2<2=25" "k_rr2<3=25" "k_tb2y<2, 2, 4, true, false, false, true, 1=33" "k_tb2y<3, 2, 4, true, false, false, true, 1=33" "k_tb2y<2, 2, 4, true, false, false, true, 0=32" "k_tb2y<3, 2, 4, true, false, false, true, 0=32" "k_tb2y<0, 2, 4, true, false, false, true, 0, 2=24" > "$OUT/pmc_level0.txt" 2>&1 || true
cat "$OUT/pmc_level0.txt" || true
step newton1023
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/prof_n1023" -o run --output-format csv -- \
    python bench.py --full --size 1023 --steps 2 --warmup 2 --ramp-ms 0 --cpu-sweeps 0 --vcycles 0 --config5 0 --newton-iters 1 > "$OUT/n1023.json" 2> "$OUT/n1023.err" || { tail -20 "$OUT/n1023.err"; exit 1; }
python tools/trace_seq.py "$(find $OUT/prof_n1023 -name '*kernel_trace.csv' -print -quit)" -4 --agg > "$OUT/n1023_seq.txt" && head -24 "$OUT/n1023_seq.txt"
python -c "import json; d=json.load(open('$OUT/n1023.json')); print('1023^3 newton', {k: v for k, v in d['newton'].items() if k != 'residuals'})"
step done
