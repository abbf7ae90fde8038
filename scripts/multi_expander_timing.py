"""ScaleUp after a sharded Estimate run on C2 (50k pods x 100 node groups, maxNodes 1000) over 4
replicas, four legs alternating in one process (python scripts/multi_expander_timing.py [reps]):

  (a) host lists: ca_multi_estimate_plan_run into page-locked host lists, numpy sums of the
      containers-only fields per option, ca_expander_best_options, the winner's list a slice of
      the host lists — all a sharded caller could do before the readers existed (this leg runs
      on a library without them as well: the other legs are then skipped);
  (b) resident: the run with sched_pod == NULL, ca_multi_estimate_plan_option_sums,
      ca_expander_best_options, ca_multi_estimate_plan_fetch_group of the winner;
  (c) leg (b) plus ca_multi_estimate_plan_groups_missing_pods of the winner against all groups;
  (d) the price expander's reader alone after a resident run: ca_multi_estimate_plan_option_price_sums,
      which uploads the price table (8 B per pod) to every block on each call.

Prints the median wall time of each leg and of its part after the run, the readers' kernel time
per block (HIP events, ca_multi_estimate_plan_reader_ms) and the bytes of the winner's list that
left its device, and checks that the legs pick the same option from the same sums.

The replicas are mirrors on ONE device: the blocks' kernels share its CUs and its copy engines, so
the figures are the cost of the protocol (threads, state, the exchange through host memory), not
scaling over devices."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from autoscaler_amd import abi, native, workloads as W  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
REPLICAS = 4
w = W.c2()
mirrors = [native.Mirror(0) for _ in range(REPLICAS)]
for m in mirrors:
    W.load_estimate(m, w)
mm = native.Multi(mirrors)
plan = native.MultiEstimatePlan(mm, w.table, w.group_off, w.pod_idx, w.templates)
readers = hasattr(plan, "option_sums")
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


def leg_host():
    t0 = time.perf_counter()
    out = plan.run(w.max_nodes, 0, want_nodes=False, copy=False)
    t1 = time.perf_counter()
    lists = out.sched_pod
    n = np.where(out.results["status"] == abi.CA_OK, out.results["n_scheduled"], 0).astype(np.int64)
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
    winner = lists[a:a + int(n[best[0]])].copy()
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t2 - t1) * 1e3, best, winner, (req_cpu, req_mem)


def leg_resident(similar: bool):
    t0 = time.perf_counter()
    out = plan.run(w.max_nodes, 0, device_results=True, copy=False)
    t1 = time.perf_counter()
    req_cpu, req_mem = plan.option_sums()
    best = pick(out.results, req_cpu, req_mem)
    winner = plan.fetch_group(int(best[0]))
    missing = plan.groups_missing_pods(int(best[0]), every) if similar else None
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t2 - t1) * 1e3, best, winner, (req_cpu, req_mem), missing


price = np.random.default_rng(1).uniform(0.001, 2.0, len(w.table))


def leg_price():
    plan.run(w.max_nodes, 0, device_results=True, copy=False)
    t1 = time.perf_counter()
    total = plan.option_price_sums(price)
    return (time.perf_counter() - t1) * 1e3, total


for _ in range(3):
    leg_host()
    if readers:
        leg_resident(False)
        leg_resident(True)
        leg_price()
A, B, Cc, KS, KM, Dd, KP = [], [], [], [], [], [], []
for _ in range(reps):
    a = leg_host()
    A.append(a[:2])
    if not readers:
        continue
    b = leg_resident(False)
    KS.append(plan.reader_ms("sums"))
    c = leg_resident(True)
    KM.append(plan.reader_ms("missing"))
    d = leg_price()
    Dd.append(d[0])
    KP.append(plan.reader_ms("price"))
    B.append(b[:2])
    Cc.append(c[:2])
    for x in (b, c):
        assert a[2].tolist() == x[2].tolist() and np.array_equal(a[3], x[3])
        assert np.array_equal(a[4][0], x[4][0]) and np.array_equal(a[4][1], x[4][1])
st = plan.stats()
n_sched = int(np.where(plan.results["status"] == abi.CA_OK, plan.results["n_scheduled"], 0).sum())
print(f"C2 max_nodes={w.max_nodes}: G={G} list positions={plan.total} scheduled={n_sched} replicas={REPLICAS} "
      f"(one device) blocks={st['blocks']} first groups={st['block_first_group']} re-run blocks={st['reruns']}")
A = np.median(np.array(A), axis=0)
print(f"(a) host lists + numpy sums + pick         : total {A[0]:.3f} ms, after the run {A[1]:.3f} ms "
      f"({4 * plan.total / 1e6:.1f} MB of lists to the host in the run)")
if readers:
    B, Cc = np.median(np.array(B), axis=0), np.median(np.array(Cc), axis=0)
    ex = plan.export_stats()
    win = int(c[2][0])
    kept = int((c[5][0] == 0).sum())
    print(f"(b) resident run + device sums + pick + one list: total {B[0]:.3f} ms, after the run {B[1]:.3f} ms "
          f"({(16 * G + 4 * len(b[3])) / 1e3:.1f} KB D2H)")
    print(f"(c) (b) + groups_missing_pods(winner, all) : total {Cc[0]:.3f} ms, after the run {Cc[1]:.3f} ms")
    print("    option_sums kernel ms per block        : " + " ".join(f"{x:.4f}" for x in np.median(np.array(KS), axis=0)))
    print("    groups_missing_pods kernels ms per block: " + " ".join(f"{x:.4f}" for x in np.median(np.array(KM), axis=0)))
    print(f"    winner group {win} in block {int(np.searchsorted(st['block_first_group'], win, side='right')) - 1}: "
          f"{len(c[3])} pods, {ex['exported_bytes']} bytes exported once, uploaded by {ex['importing_blocks']} blocks; "
          f"{kept} of {G} groups hold every pod of the winner's")
    print(f"(d) option_price_sums after a resident run : {float(np.median(Dd)):.3f} ms "
          f"({8 * len(price) * st['blocks'] / 1e3:.0f} KB of prices uploaded: {len(price)} pods x 8 B x {st['blocks']} blocks)")
    print("    option_price_sums kernel ms per block  : " + " ".join(f"{x:.4f}" for x in np.median(np.array(KP), axis=0)))
else:
    print("(b), (c), (d): this library has no readers on sharded plans")
print("replicas share one device: these are the protocol's costs, not scaling over devices", flush=True)
plan.close()
mm.close()
for m in mirrors:
    m.close()
