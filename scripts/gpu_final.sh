#!/bin/bash
# Round-end GPU job: all GPU tests, the bench line, its rocprofv3 kernel stats, the
# timing scripts, and a 2-rank rehearsal of the multi-GPU bench on one device.
set -o pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
cd "$ROOT"
export CASIM_JOB_OUT="${CASIM_JOB_OUT:-$ROOT/job_out}"   # gpu_job.sh writes there too
OUT="$CASIM_JOB_OUT"
bash scripts/gpu_job.sh tests "tests" bench "--full --steps 20 --warmup 5" prof "--full --steps 20 --warmup 5" \
    script "scripts/filter_timing.py" script "scripts/util_diag.py" script "scripts/plan_prof.py" || exit $?
CASIM_BENCH_BACKEND=gloo timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
    --master-port 29517 bench.py --gpus 2 --steps 10 --warmup 3 --full > "$OUT/multi2.json" 2> "$OUT/multi2.err" || {
    echo "MULTI FAILED"; tail -20 "$OUT/multi2.err"; exit 1; }
cat "$OUT/multi2.json"
echo FINAL_OK
