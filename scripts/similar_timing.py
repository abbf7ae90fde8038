"""filterNodeGroupsByPods after the least-waste pick on C2 (maxNodes 1000, device results), two
forms alternating in one process (python scripts/similar_timing.py [reps]):

  (a) fetch: ca_estimate_plan_fetch_group of the winner and of every similar group, numpy set
      membership (np.isin) of the winner's ids in each list — what a caller could do without
      the device filter;
  (b) resident: ca_estimate_plan_groups_missing_pods over the similar groups, then
      ca_estimate_plan_fetch_group of the winner.

Both follow the same run, ca_estimate_plan_option_sums and ca_expander_best_options; the times
are of the part after the pick.  Similar groups are those whose template has the winner's
allocatable (what workloads.c2 gives the groups of one instance shape).  Prints the median wall
time of each form, the kernels' device time (HIP events: two row memsets' worth of zeroing, the
mark and the test kernel), the bytes each form moves to the host and the number of similar
groups, and checks that both forms keep the same groups."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from autoscaler_amd import abi, native, workloads as W  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
w = W.c2()
g = native.Mirror(0)
W.load_estimate(g, w)
plan = native.EstimatePlan(g, w.table, w.group_off, w.pod_idx, w.templates)
G = plan.G
node = w.templates["node"]
cap_cpu = np.ascontiguousarray(node["alloc_milli_cpu"], dtype=np.int64)
cap_mem = np.ascontiguousarray(node["alloc_memory"], dtype=np.int64)
cap_pods = np.ascontiguousarray(node["alloc_pods"], dtype=np.int64)
every = np.arange(G, dtype=np.int32)
LW = abi.CA_EXPANDER_LEAST_WASTE


def run_and_pick():
    out = plan.run(w.max_nodes, 0, device_results=True, copy=False)
    req_cpu, req_mem = plan.option_sums()
    valid = every[(out.results["n_scheduled"] > 0) & (out.results["node_count"] > 0)]
    best = int(native.expander_best_options(LW, out.results, req_cpu, req_mem, cap_cpu, cap_mem, valid)[0][0])
    same = (cap_cpu == cap_cpu[best]) & (cap_mem == cap_mem[best]) & (cap_pods == cap_pods[best])
    similar = [int(k) for k in valid if k != best and same[k]]         # the similar groups that have an option
    return best, similar


def form_fetch(best, similar):
    t0 = time.perf_counter()
    winner = plan.fetch_group(best)
    moved = 4 * len(winner)
    n_missing, first = np.zeros(len(similar), np.int32), np.full(len(similar), -1, np.int32)
    for i, k in enumerate(similar):
        ids = plan.fetch_group(k)
        moved += 4 * len(ids)
        miss = ~np.isin(winner, ids)
        n_missing[i] = int(miss.sum())
        if n_missing[i]:
            first[i] = int(np.argmax(miss))
    return (time.perf_counter() - t0) * 1e3, n_missing, first, winner, moved


def form_resident(best, similar):
    t0 = time.perf_counter()
    n_missing, first = plan.groups_missing_pods(best, similar)
    winner = plan.fetch_group(best)
    return (time.perf_counter() - t0) * 1e3, n_missing, first, winner, 8 * len(similar) + 4 * len(winner)


for _ in range(3):
    b, s = run_and_pick()
    form_fetch(b, s)
    form_resident(b, s)
A, B, K = [], [], []
for _ in range(reps):
    best, similar = run_and_pick()
    a = form_fetch(best, similar)
    bb = form_resident(best, similar)
    K.append(plan.groups_missing_pods_ms())
    A.append(a[0])
    B.append(bb[0])
    assert a[1].tolist() == bb[1].tolist() and a[2].tolist() == bb[2].tolist() and np.array_equal(a[3], bb[3])
n_sched = plan.results["n_scheduled"]
print(f"C2 max_nodes={w.max_nodes}: G={G} pods={len(w.table)} winner group {best} ({int(n_sched[best])} scheduled pods), "
      f"{len(similar)} similar groups with an option ({int(n_sched[similar].sum())} scheduled pods), "
      f"{int((bb[1] == 0).sum())} kept")
print(f"(a) fetch winner + similar lists, np.isin : {np.median(A):.3f} ms after the pick ({a[4] / 1e6:.2f} MB D2H)")
print(f"(b) device filter + the winner's list      : {np.median(B):.3f} ms after the pick ({bb[4] / 1e3:.1f} KB D2H)")
print(f"kernels (row zeroing, mark, test): {np.median(K) * 1e3:.1f} us (HIP events); "
      f"bitmap rows {len(similar)} x {4 * ((len(w.table) + 31) // 32)} B", flush=True)
plan.close()
g.close()
