"""Least-waste pick after a device-results Estimate run on C2 (maxNodes 1000), two forms
alternating in one process (python scripts/expander_timing.py [reps]):

  (a) fetch: the run, ca_estimate_plan_fetch of every list, numpy sums of the containers-only
      fields per option, ca_expander_best_options — what a caller could do without the device sums;
  (b) resident: the run, ca_estimate_plan_option_sums, ca_expander_best_options,
      ca_estimate_plan_fetch_group of the winner.

Prints the median wall time of each form and of its part after the run, the sums kernel's
device time (HIP events) against its byte floor of 8 B per scheduled pod (4 B id + 4 B class)
at 6.3 TB/s, and checks that both forms pick the same option from the same sums."""
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
cap_cpu = np.ascontiguousarray(w.templates["node"]["alloc_milli_cpu"], dtype=np.int64)
cap_mem = np.ascontiguousarray(w.templates["node"]["alloc_memory"], dtype=np.int64)
sc_cpu = np.ascontiguousarray(w.table.pods["score_milli_cpu"])
sc_mem = np.ascontiguousarray(w.table.pods["score_memory"])
off = plan.group_off.astype(np.int64)
every = np.arange(G, dtype=np.int32)
LW = abi.CA_EXPANDER_LEAST_WASTE


def pick(results, req_cpu, req_mem):
    valid = every[(results["n_scheduled"] > 0) & (results["node_count"] > 0)]
    return native.expander_best_options(LW, results, req_cpu, req_mem, cap_cpu, cap_mem, valid)[0]


def form_fetch():
    t0 = time.perf_counter()
    out = plan.run(w.max_nodes, 0, device_results=True, copy=False)
    t1 = time.perf_counter()
    lists = plan.fetch()
    n = out.results["n_scheduled"].astype(np.int64)
    # positions below n_scheduled of every group's slice, then segment sums
    keep = np.arange(len(lists)) - np.repeat(off[:-1], np.diff(off)) < np.repeat(n, np.diff(off))
    ids = lists[keep]
    some = np.nonzero(n > 0)[0]                       # (reduceat wants non-empty segments)
    seg = (np.cumsum(n) - n)[some]
    req_cpu, req_mem = np.zeros(G, np.int64), np.zeros(G, np.int64)
    if len(some):
        req_cpu[some] = np.add.reduceat(sc_cpu[ids], seg)
        req_mem[some] = np.add.reduceat(sc_mem[ids], seg)
    best = pick(out.results, req_cpu, req_mem)
    a = int(off[best[0]])
    winner = lists[a:a + int(n[best[0]])]
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t2 - t1) * 1e3, best, winner, (req_cpu, req_mem)


def form_resident():
    t0 = time.perf_counter()
    out = plan.run(w.max_nodes, 0, device_results=True, copy=False)
    t1 = time.perf_counter()
    req_cpu, req_mem = plan.option_sums()
    best = pick(out.results, req_cpu, req_mem)
    winner = plan.fetch_group(int(best[0]))
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t2 - t1) * 1e3, best, winner, (req_cpu, req_mem)


for _ in range(3):
    form_fetch()
    form_resident()
A, B, K = [], [], []
for _ in range(reps):
    a = form_fetch()
    b = form_resident()
    K.append(plan.option_sums_ms())
    A.append(a[:2])
    B.append(b[:2])
    assert a[2].tolist() == b[2].tolist() and np.array_equal(a[3], b[3])
    assert np.array_equal(a[4][0], b[4][0]) and np.array_equal(a[4][1], b[4][1])
A, B = np.median(np.array(A), axis=0), np.median(np.array(B), axis=0)
n_sched = int(plan.results["n_scheduled"].sum())
k_ms = float(np.median(K))
floor_us = 8.0 * n_sched / 6.3e12 * 1e6
print(f"C2 max_nodes={w.max_nodes}: G={G} list positions={plan.total} scheduled={n_sched} "
      f"classes<=LDS bound: {len(np.unique(w.table.pods[['score_milli_cpu', 'score_memory']])) <= native.OPTION_SUMS_LDS_CLASSES}")
print(f"(a) fetch all + numpy sums + pick : total {A[0]:.3f} ms, after the run {A[1]:.3f} ms ({4 * plan.total / 1e6:.1f} MB D2H)")
print(f"(b) device sums + pick + one list : total {B[0]:.3f} ms, after the run {B[1]:.3f} ms "
      f"({(16 * G + 4 * len(b[3])) / 1e3:.1f} KB D2H)")
print(f"sums kernel: {k_ms * 1e3:.1f} us (HIP events), byte floor {floor_us:.2f} us at 8 B per scheduled pod, "
      f"{8.0 * n_sched / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0:.0f} GB/s", flush=True)
plan.close()
g.close()
