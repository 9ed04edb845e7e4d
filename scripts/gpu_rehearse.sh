#!/bin/bash
# Rehearsal of bench.py's N > 1 path on one GPU: `bench.py --gpus N` launches
# its N ranks itself, all on cuda:0 over the library's host exchange (gloo),
# every workload.  Usage: scripts/gpu_rehearse.sh TAG [N]
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
export OUT=${OUT:-out}  # where the bench lines go
mkdir -p "$OUT"
TAG=${1:-reh}
N=${2:-2}
for w in ${WORKLOADS:-advection gol gol_amr poisson scalability advection_adapt}; do
  DCCRG_BENCH_TRANSPORT=host timeout -k 10 400 python -u bench.py --full --gpus $N --steps ${STEPS:-5} --warmup 1 --workload $w \
      > $OUT/${TAG}_$w.json 2> $OUT/${TAG}_$w.err
  rc=$?
  echo "[rehearse] $w rc=$rc"; tail -c 600 $OUT/${TAG}_$w.json; echo
  [ $rc -eq 0 ] || { tail -20 $OUT/${TAG}_$w.err; exit $rc; }
done
