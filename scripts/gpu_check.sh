#!/bin/bash
# One GPU session: parity tests, a short bench, a rocprofv3 kernel-trace of
# the bench.  Stops at the first crash / timeout (exit codes other than 0/1).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
export OUT=${OUT:-out}  # where logs, bench lines and profiles go
mkdir -p "$OUT"
TAG=${1:-r01}
STEPS=${STEPS:-100}
echo "[gpu_check] $(date) host=$(hostname) nproc=$(nproc)"
lscpu | grep -E 'Model name|^CPU\(s\)' > $OUT/host_cpu.txt 2>&1
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread \
    > $OUT/pytest_gpu_${TAG}.log 2>&1
rc=$?
tail -5 $OUT/pytest_gpu_${TAG}.log
echo "[gpu_check] pytest rc=$rc"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 600 python -u bench.py --full --steps $STEPS --warmup 5 > $OUT/bench_${TAG}.json 2> $OUT/bench_${TAG}.err
rc=$?
cat $OUT/bench_${TAG}.json; tail -3 $OUT/bench_${TAG}.err
echo "[gpu_check] bench rc=$rc"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -o run --output-format csv -- \
    python -u bench.py --steps 20 --warmup 2 --no-cpu-baseline > $OUT/bench_prof_${TAG}.json 2> $OUT/prof_${TAG}.err
rc=$?
echo "[gpu_check] rocprof rc=$rc"
find $OUT/prof_${TAG} -name '*stats*' | head
[ $rc -eq 0 ] || exit $rc
# HBM traffic of the sweep (both advection kernels): FETCH_SIZE and
# WRITE_SIZE in separate --pmc runs
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 120 rocprofv3 --pmc $c --kernel-include-regex 'advection_(regular|tiles)' -d $OUT/pmc_${TAG}_$c -o run \
      --output-format csv -- python -u bench.py --steps 10 --warmup 1 --no-cpu-baseline > $OUT/pmc_${TAG}_$c.json 2> $OUT/pmc_${TAG}_$c.err
  rc=$?
  echo "[gpu_check] pmc $c rc=$rc"
  [ $rc -eq 0 ] || exit $rc
done
python scripts/traffic.py 'advection_(regular|tiles)' $OUT/pmc_${TAG}_FETCH_SIZE $OUT/pmc_${TAG}_WRITE_SIZE \
    --bench-json $OUT/pmc_${TAG}_FETCH_SIZE.json > $OUT/traffic_${TAG}.json && cat $OUT/traffic_${TAG}.json
