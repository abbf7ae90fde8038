#!/bin/bash
# GPU-box job: build, GPU tests, smoke, bench, rocprof kernel stats.  Every GPU step has
# its own time limit; the chain stops at the first failure.
set -o pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
cd "$ROOT"
OUT="${CASIM_JOB_OUT:-$ROOT/job_out}"          # logs and results of the job
mkdir -p "$OUT"
export TMPDIR=/tmp
STEP="${1:-all}"
python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { echo BUILD FAILED; tail "$OUT/build.log"; exit 1; }
if [[ "$STEP" == all || "$STEP" == tests ]]; then
  timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$OUT/pytest_gpu.log" 2>&1; rc=$?
  tail -5 "$OUT/pytest_gpu.log"
  [[ $rc -eq 0 ]] || { echo "GPU TESTS FAILED rc=$rc"; tail -40 "$OUT/pytest_gpu.log"; exit $rc; }
fi
if [[ "$STEP" == all || "$STEP" == smoke ]]; then
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { echo SMOKE FAILED; tail -20 "$OUT/smoke.log"; exit 1; }
  tail -1 "$OUT/smoke.log"
fi
if [[ "$STEP" == all || "$STEP" == bench ]]; then
  timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || { echo BENCH FAILED; tail -20 "$OUT/bench.err"; exit 1; }
  cat "$OUT/bench.json"
fi
if [[ "$STEP" == all || "$STEP" == prof ]]; then
  # the headline alone (the bench line's kernel averages come from these launches only),
  # then the other legs in a profile of their own
  cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run \
     --output-format csv -- python3 "$ROOT/bench.py" --steps 5 --warmup 2 --no-cpu-baseline --no-sweep --no-c4 \
     --no-expansion --no-util --no-filter --no-unlimited --no-runonce --no-planner \
     > "$OUT/prof.log" 2>&1 || { echo PROF FAILED; tail -20 "$OUT/prof.log"; exit 1; }
  cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_legs" -o run \
     --output-format csv -- python3 "$ROOT/bench.py" --full --steps 3 --warmup 1 --no-cpu-baseline \
     > "$OUT/prof_legs.log" 2>&1 || { echo PROF LEGS FAILED; tail -20 "$OUT/prof_legs.log"; exit 1; }
  cd "$ROOT"
  echo PROF_OK
fi
if [[ "$STEP" == pmc ]]; then
  # HBM traffic: one counter per pass (FETCH_SIZE and WRITE_SIZE cannot share a pass on gfx950)
  for c in FETCH_SIZE WRITE_SIZE; do
    cd /tmp && PMC_STEPS=3 timeout -k 10 300 rocprofv3 --pmc $c --kernel-trace -d "$OUT/pmc_$c" -o run \
       --output-format csv -- python3 "$ROOT/scripts/pmc_step.py" \
       > "$OUT/pmc_$c.log" 2>&1 || { echo "PMC $c FAILED"; tail -20 "$OUT/pmc_$c.log"; exit 1; }
  done
  cd "$ROOT"
  python3 scripts/pmc_traffic.py "$OUT" 3 > "$OUT/pmc_traffic.json" && cat "$OUT/pmc_traffic.json"
fi
echo ROUND_OK
