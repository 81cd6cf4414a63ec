#!/bin/bash
# GPU validation of a build (one gpurun call): the test files named on the command line (default: all), smoke(), the
# full bench line (modes, stages, parity, cpu baseline) and the rocprofv3 kernel stats of the bench command
OUT=${OUT:-out}                  # logs and JSON lines, relative to the repository root
mkdir -p $OUT
export TMPDIR=/tmp
R=$(pwd)
TESTS=${@:-tests}
timeout ${PYTEST_TIMEOUT:-2400} python -m pytest $TESTS -m gpu -q --durations=8 < /dev/null > $OUT/pytest_gpu.log 2>&1
echo "pytest exit: $?" >> $OUT/pytest_gpu.log; tail -14 $OUT/pytest_gpu.log | cut -c1-220
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" < /dev/null > $OUT/smoke.log 2>&1; echo "smoke exit $?" >> $OUT/smoke.log; tail -2 $OUT/smoke.log
if [ -z "$SKIP_BENCH" ]; then
timeout 900 python bench.py --full --steps ${STEPS:-20} --warmup 3 < /dev/null > $OUT/final_bench.json 2> $OUT/final_bench.err; echo "bench exit $?"
python tools/bench_brief.py $OUT/final_bench.json bench | cut -c1-700
cd /tmp && timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/final_prof -o bench -- python $R/bench.py --full --steps 4 --warmup 1 --no-cpu-baseline --no-modes --no-stages < /dev/null > $R/$OUT/final_prof_bench.json 2> $R/$OUT/final_prof_bench.err
cd $R; f=$(find $OUT/final_prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp "$f" $OUT/final_kernel_stats.csv && head -9 $OUT/final_kernel_stats.csv | cut -c1-200
python tools/bench_brief.py $OUT/final_prof_bench.json profiled | head -1 | cut -c1-400
fi
