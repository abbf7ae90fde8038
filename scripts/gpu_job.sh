#!/bin/bash
# GPU-box job runner (the library is built in-tree on the CPU side beforehand).
#   scripts/gpu_job.sh tests "<pytest -k expr or file list>"   GPU tests
#   scripts/gpu_job.sh bench "<bench.py args>"                   one bench line
#   scripts/gpu_job.sh prof  "<bench.py args>"                   rocprofv3 kernel stats of a bench run
#   scripts/gpu_job.sh pmc   "<counters>|<script args>"           one rocprofv3 counter pass over a script
# Every GPU step has its own time limit; the chain stops at the first failure.
set -o pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
cd "$ROOT"
OUT="${CASIM_JOB_OUT:-$ROOT/job_out}"          # logs and results of the job
mkdir -p "$OUT"
: > "$OUT/script.log"
export TMPDIR=/tmp
rc=0
while [[ $# -gt 0 ]]; do
  step="$1"; arg="$2"; shift 2
  case "$step" in
    tests)
      eval timeout -k 10 900 python -u -m pytest $arg -m gpu -x -q --timeout 300 --timeout-method thread \
        > "$OUT/pytest_gpu.log" 2>&1; rc=$?
      tail -4 "$OUT/pytest_gpu.log"
      [[ $rc -eq 0 ]] || { echo "GPU TESTS FAILED rc=$rc"; tail -60 "$OUT/pytest_gpu.log"; exit $rc; } ;;
    bench)
      timeout -k 10 600 python -u bench.py $arg > "$OUT/bench.json" 2> "$OUT/bench.err"; rc=$?
      [[ $rc -eq 0 ]] || { echo "BENCH FAILED rc=$rc"; tail -30 "$OUT/bench.err"; exit $rc; }
      cat "$OUT/bench.json" ;;
    prof)
      cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run \
        --output-format csv -- python3 "$ROOT/bench.py" $arg > "$OUT/prof.log" 2>&1; rc=$?
      cd "$ROOT"
      [[ $rc -eq 0 ]] || { echo "PROF FAILED rc=$rc"; tail -30 "$OUT/prof.log"; exit $rc; }
      echo PROF_OK ;;
    pmc)
      ctrs="${arg%%|*}"; sargs="${arg#*|}"; tag=$(echo "$ctrs" | tr ' ' '_' | cut -c1-60)
      cd /tmp && timeout -s KILL 120 rocprofv3 --pmc $ctrs -d "$OUT/pmc_$tag" -o run \
        --output-format csv -- python3 $ROOT/$sargs > "$OUT/pmc_$tag.log" 2>&1; rc=$?
      cd "$ROOT"
      [[ $rc -eq 0 ]] || { echo "PMC FAILED rc=$rc"; tail -30 "$OUT/pmc_$tag.log"; exit $rc; }
      echo "PMC_OK $tag" ;;
    script)
      echo "== $arg" >> "$OUT/script.log"
      timeout -k 10 600 python -u $arg >> "$OUT/script.log" 2>&1; rc=$?
      tail -40 "$OUT/script.log"
      [[ $rc -eq 0 ]] || { echo "SCRIPT FAILED rc=$rc"; exit $rc; } ;;
    *) echo "unknown step $step"; exit 2 ;;
  esac
done
echo JOB_OK
