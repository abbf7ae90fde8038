"""scripts/ab_lib.py with run-time switches: A/B of (library, environment) variants on the
bench's headline step (C2, results on the host as 16-bit podset indices, phase events off),
alternating processes, each timing 40 steps after 5 warm-up steps.  AB_IDS=i32 among a
variant's variables times the 32-bit-id step (ca_estimate_plan_run) instead.
Usage: python scripts/ab_knobs.py LABEL=LIB[,VAR=VALUE...] [LABEL=LIB[,VAR=VALUE...] ...] [rounds]

(Records A and B of profiles/publish_hold_ab.txt were taken with an earlier form of this
script on a tree that still had the publisher's hold list: the CASIM_PUB_HOLD and
CASIM_PUB_EXACT switches and the "held" column printed there left with it.)"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r"""
import os, sys, time
sys.path.insert(0, %r)
from autoscaler_amd import native, workloads as W
w = W.c2()
m = native.Mirror(0)
W.load_estimate(m, w)
with native.EstimatePlan(m, w.table, w.group_off, w.pod_idx, w.templates) as plan:
    plan.set_phase_timing(False)
    if os.environ.get("AB_IDS") == "i32":
        step = lambda: plan.run(w.max_nodes, 0, want_nodes=False, copy=False)
    else:
        step = lambda: plan.run_u16(w.max_nodes, 0, copy=False)
    for _ in range(5):
        step()
    ts = []
    for _ in range(40):
        t = time.perf_counter()
        step()
        ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    print(ts[len(ts) // 2], ts[0])
""" % ROOT

args = sys.argv[1:]
rounds = int(args.pop()) if args and args[-1].isdigit() else 4
variants = []
for a in args:
    label, rest = a.split("=", 1)
    lib, *kv = rest.split(",")
    variants.append((label, os.path.abspath(lib), dict(x.split("=", 1) for x in kv)))
res = {label: [] for label, _, _ in variants}
for r in range(rounds):
    for label, lib, kv in variants:
        env = dict(os.environ, CASIM_LIB_PATH=lib, CASIM_KNOBS="1", **kv)
        out = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=300)
        if out.returncode != 0:
            print(out.stderr[-2000:])
            sys.exit(1)
        med, mn = map(float, out.stdout.split())
        res[label].append(med)
        print(f"round {r} {label}: median {med:.4f} min {mn:.4f}", flush=True)
for label, v in res.items():
    print(f"{label}: median of medians {np.median(v):.4f} ms ({', '.join(f'{x:.4f}' for x in v)})  range {max(v) - min(v):.4f}")
