"""A/B of two or more builds of the library on the cold path of the headline batch (C2):
alternating processes, each building a new plan and running it once, 9 times after 2 warm
builds, as bench.py's extra.cold does (no resident podset: the host item walk, tie check and
list upload are inside plan creation; first run with 16-bit ids on the host), then the
one-shot Mirror.estimate, then the option form on a resident podset (scripts/cold_options.py).
Prints the median of each process in ms.
Usage: python scripts/cold_ab.py LABEL=LIB [LABEL=LIB ...] [rounds]"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r"""
import os, sys, time
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "scripts"))
from autoscaler_amd import native, workloads as W
import cold_options
w = W.c2()
m = native.Mirror(0)
W.load_estimate(m, w)
ps = m.podset(w.table)
eg_off, eg_pod, ok = cold_options.controllers(w)
clock = time.perf_counter
cp, cr, cb, oc, orun = [], [], [], [], []
for it in range(11):
    t0 = clock()
    with native.EstimatePlan(m, w.table, w.group_off, w.pod_idx, w.templates) as p:
        t1 = clock()
        p.run_u16(w.max_nodes, 0, copy=False)
        t2 = clock()
    t3 = clock()
    m.estimate(w.table, w.group_off, w.pod_idx, w.templates, w.max_nodes, 0, want_nodes=False)
    t4 = clock()
    with native.EstimatePlan.from_options(m, ps, eg_off, eg_pod, ok, w.templates) as p:
        t5 = clock()
        p.run_u16(w.max_nodes, 0, copy=False)
        t6 = clock()
    if it >= 2:
        cp.append(t1 - t0); cr.append(t2 - t1); cb.append(t4 - t3); oc.append(t5 - t4); orun.append(t6 - t5)
med = lambda v: float(np.median(v)) * 1e3
print(med(cp), med(cr), med(np.add(cp, cr)), med(cb), med(oc), med(np.add(oc, orun)))
""" % (ROOT, ROOT)

NAMES = ("plan_create", "first_run", "create+first_run", "one_shot_estimate", "options_create", "options_create+first_run")
args = sys.argv[1:]
rounds = int(args.pop()) if args and args[-1].isdigit() else 4
variants = [(a.split("=", 1)[0], os.path.abspath(a.split("=", 1)[1])) for a in args]
res = {label: [] for label, _ in variants}
for r in range(rounds):
    for label, lib in variants:
        env = dict(os.environ, CASIM_LIB_PATH=lib)
        out = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            print(out.stderr[-2000:])
            sys.exit(1)
        v = list(map(float, out.stdout.split()))
        res[label].append(v)
        print(f"round {r} {label}: " + "  ".join(f"{n} {x:.3f}" for n, x in zip(NAMES, v)), flush=True)
for label, rows in res.items():
    a = np.array(rows)
    print(f"{label}: " + "  ".join(f"{n} {np.median(a[:, i]):.3f} ({a[:, i].min():.3f}-{a[:, i].max():.3f})" for i, n in enumerate(NAMES)))
