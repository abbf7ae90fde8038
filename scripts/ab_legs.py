"""A/B of two or more builds of the library on two of bench.py --full's Estimate legs, timed as
bench.py times them: extra.c4 (C4 batch, results left in device memory, 20 steps after 2) and
extra.c2_unlimited (C2 with max_nodes = 0, 32-bit ids to the host, 5 steps after 1).
Alternating processes; prints each process's medians in ms and which chain kernel ran.
Usage: python scripts/ab_legs.py LABEL=LIB [LABEL=LIB ...] [rounds]"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r"""
import sys, time
import numpy as np
sys.path.insert(0, %r)
from autoscaler_amd import native, workloads as W
def leg(w, step, warm, n):
    m = native.Mirror(0)
    W.load_estimate(m, w)
    with native.EstimatePlan(m, w.table, w.group_off, w.pod_idx, w.templates) as plan:
        for _ in range(warm):
            step(plan, w)
        ts = []
        for _ in range(n):
            t = time.perf_counter()
            r = step(plan, w)
            ts.append(time.perf_counter() - t)
            r = None
        st = plan.stats()
    m.close()
    return float(np.median(ts) * 1e3), int(st["table_chain"]) + int(st["lean_chain"])
c4 = leg(W.c4(n_pods=50_000, n_groups=100, n_existing=1000, max_nodes=1000),
         lambda p, w: p.run(w.max_nodes, 0, copy=False, device_results=True), 2, 20)
un = leg(W.c2(), lambda p, w: p.run(0, 0, want_nodes=False, copy=False), 1, 5)
print(c4[0], c4[1], un[0], un[1])
""" % ROOT

KERNEL = ("stream", "table", "lean")
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
        a, ka, b, kb = out.stdout.split()
        res[label].append((float(a), float(b)))
        print(f"round {r} {label}: c4 {float(a):.4f} ({KERNEL[int(ka)]})  c2_unlimited {float(b):.4f} ({KERNEL[int(kb)]})", flush=True)
for label, rows in res.items():
    v = np.array(rows)
    print(f"{label}: c4 median {np.median(v[:, 0]):.4f} ({v[:, 0].min():.4f}-{v[:, 0].max():.4f})  "
          f"c2_unlimited median {np.median(v[:, 1]):.4f} ({v[:, 1].min():.4f}-{v[:, 1].max():.4f})")
