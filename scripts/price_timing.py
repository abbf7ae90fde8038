"""Price-expander pick after a device-results Estimate run on C2 (maxNodes 1000), two forms
alternating in one process (python scripts/price_timing.py [reps]):

  (a) fetch: the run, ca_estimate_plan_fetch of every list, the in-order float64 sum of the
      pods' prices per option on the host (np.add.accumulate, which adds left to right; np.sum
      is pairwise), the pick — what a caller had to do without the device sums;
  (b) resident: the run, ca_estimate_plan_option_price_sums, the pick,
      ca_estimate_plan_fetch_group of the winner.

Per-pod prices come from a linear model of the requests; node prices from one of the
templates' allocatable.  The pick is PriceBased.option_score per option and the loop of
price.go:178-184.  The pick is Python here (a Go shim's is a few floating-point operations per option) and
is the same code in both forms; its time is printed apart.
Prints the median wall time of each form and of its part after the run, the
kernel's device time (HIP events), the longest list's n_scheduled and their quotient — the
cost of one dependent add of the chain — and checks that both forms give the same totals, bit
for bit, and pick the same option."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from autoscaler_amd import k8s, native, workloads as W  # noqa: E402
from autoscaler_amd.expander import PriceBased, SimpleNodeUnfitness  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
w = W.c2()
g = native.Mirror(0)
W.load_estimate(g, w)
plan = native.EstimatePlan(g, w.table, w.group_off, w.pod_idx, w.templates)
G = plan.G
off = plan.group_off.astype(np.int64)
every = np.arange(G, dtype=np.int32)
GI = float(1 << 30)
pods = w.table.pods
price = (pods["score_milli_cpu"].astype(np.float64) * 0.0317e-3 + pods["score_memory"].astype(np.float64) / GI * 0.00425)
node_price = (w.templates["node"]["alloc_milli_cpu"].astype(np.float64) * 0.031e-3 +
              w.templates["node"]["alloc_memory"].astype(np.float64) / GI * 0.0042)
nodes = [k8s.build_test_node(f"t{i}", int(t["node"]["alloc_milli_cpu"]), int(t["node"]["alloc_memory"]))
         for i, t in enumerate(w.templates)]
preferred = k8s.build_test_node("preferred", 4000, 16 << 30)
flt = PriceBased(None, None, SimpleNodeUnfitness)
stabilization = 500 * 0.0317e-3 + 500.0 / 1024 * 0.00425


def pick(results, totals):
    scored = []
    for o in every[(results["n_scheduled"] > 0) & (results["node_count"] > 0)].tolist():
        if np.isnan(totals[o]):
            continue
        scored.append((o, flt.option_score(node_price[o], int(results[o]["node_count"]), totals[o], stabilization,
                                           preferred, nodes[o], True)))
    return flt._pick(scored)


def form_fetch():
    t0 = time.perf_counter()
    out = plan.run(w.max_nodes, 0, device_results=True, copy=False)
    t1 = time.perf_counter()
    lists = plan.fetch()
    n = out.results["n_scheduled"].astype(np.int64)
    totals = np.zeros(G, np.float64)
    for o in range(G):
        if n[o] > 0:
            a = int(off[o])
            totals[o] = np.add.accumulate(price[lists[a:a + int(n[o])]])[-1]
    tp = time.perf_counter()
    best = pick(out.results, totals)
    tp = time.perf_counter() - tp
    a = int(off[best[0]])
    winner = lists[a:a + int(n[best[0]])]
    t2 = time.perf_counter()
    return ((t2 - t0) * 1e3, (t2 - t1) * 1e3, tp * 1e3), best, winner, totals


def form_resident():
    t0 = time.perf_counter()
    out = plan.run(w.max_nodes, 0, device_results=True, copy=False)
    t1 = time.perf_counter()
    totals = plan.option_price_sums(price)
    tp = time.perf_counter()
    best = pick(out.results, totals)
    tp = time.perf_counter() - tp
    winner = plan.fetch_group(int(best[0]))
    t2 = time.perf_counter()
    return ((t2 - t0) * 1e3, (t2 - t1) * 1e3, tp * 1e3), best, winner, totals


for _ in range(3):
    form_fetch()
    form_resident()
A, B, K = [], [], []
for _ in range(reps):
    a = form_fetch()
    b = form_resident()
    K.append(plan.option_price_sums_ms())
    A.append(a[0])
    B.append(b[0])
    assert a[1] == b[1] and np.array_equal(a[2], b[2])
    assert a[3].tobytes() == b[3].tobytes()
A, B = np.median(np.array(A), axis=0), np.median(np.array(B), axis=0)
ns = plan.results["n_scheduled"].astype(np.int64)
n_sched, longest = int(ns.sum()), int(ns.max())
k_ms = float(np.median(K))
print(f"C2 max_nodes={w.max_nodes}: G={G} list positions={plan.total} scheduled={n_sched} pods={len(price)}")
print(f"(a) fetch all + in-order host sums + pick : total {A[0]:.3f} ms, after the run {A[1]:.3f} ms "
      f"of which the pick {A[2]:.3f} ms ({4 * plan.total / 1e6:.1f} MB D2H)")
print(f"(b) device price sums + pick + one list   : total {B[0]:.3f} ms, after the run {B[1]:.3f} ms "
      f"of which the pick {B[2]:.3f} ms ({8 * len(price) / 1e3:.1f} KB H2D, {(8 * G + 4 * len(b[2])) / 1e3:.1f} KB D2H)")
print(f"price sums kernel: {k_ms * 1e3:.1f} us (HIP events), longest list {longest} pods, "
      f"{k_ms * 1e6 / longest if longest else 0:.2f} ns per add of its chain", flush=True)
plan.close()
g.close()
