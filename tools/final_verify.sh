#!/bin/bash
# Round-end verification on the GPU box: full GPU suite, smoke, the bench line, and the rocprofv3 passes profiles/ is built from.
# Run from the repo root on the GPU machine; outputs land in $SVT_VERIFY_OUT (default verify_out/; then: python3 tools/refresh_profiles.py).
R=${SVT_ROUND:-r03}
OUT=${SVT_VERIFY_OUT:-verify_out}
export SVT_VERIFY_OUT=$OUT
set -e -o pipefail
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/gpu_tests.log 2>&1 || { tail -30 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
timeout -k 10 300 python __graft_entry__.py smoke 2>&1 | tail -1
timeout -k 10 600 python bench.py --full > $OUT/bench_final.log 2> $OUT/bench_final.err || { tail -20 $OUT/bench_final.err; exit 1; }
tail -1 $OUT/bench_final.log | cut -c1-400
rm -rf $OUT/${R}s $OUT/${R}f $OUT/${R}w $OUT/${R}q
BENCH="bench.py --full --steps 6 --warmup 3 --no-cpu-baseline --no-extras"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${R}s -o bench --output-format csv -- python3 $BENCH > $OUT/${R}s.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/${R}f -o bench --output-format csv -- python3 $BENCH > $OUT/${R}f.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/${R}w -o bench --output-format csv -- python3 $BENCH > $OUT/${R}w.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_INSTS_VMEM_RD -d $OUT/${R}q -o bench --output-format csv -- python3 $BENCH > $OUT/${R}q.log 2>&1
rm -rf $OUT/${R}m
timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU_MFMA_F16 SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU SQ_BUSY_CYCLES -d $OUT/${R}m -o bench --output-format csv -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > $OUT/${R}m.log 2>&1
if [ -x tools/ubench/hadamard_mfma ]; then ./tools/ubench/hadamard_mfma > $OUT/hadamard_mfma.txt 2>&1 || true; fi
if [ -f tools/_libprof7.so ]; then timeout -k 10 300 python tools/me_phase_profile.py 1 2 5 7 > $OUT/me_phase.log 2>&1 || tail -5 $OUT/me_phase.log; fi
find $OUT/${R}s $OUT/${R}f $OUT/${R}w $OUT/${R}q -name "*.csv" | head -20
echo verify-done
