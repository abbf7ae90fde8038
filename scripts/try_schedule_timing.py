"""TrySchedulePods timing on c5_filter(n_nodes=2000, n_pending=6000): one ca_try_schedule_pods
call with a half-on node mask and the break, against the per-pod path it replaces (the
reference loop over ca_check_predicates / ca_fits_any_node / ca_mirror_add_pods, two or three
device calls per pod) and against the ALL call (python scripts/try_schedule_timing.py)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

from autoscaler_amd import abi, native, workloads as W  # noqa: E402
from tspgen import try_schedule_ref  # noqa: E402

w = W.c5_filter(n_nodes=2000, pods_per_node=20, n_pending=6000)
n = len(w.nodes)
half = (abi.CA_MATCH_MASK, 0, 0, -1, (np.arange(n) & 1).astype(np.uint8))
g = native.Mirror(0)
W.load_filter(g, w)


def timed(f, reps):
    ts, ks, r = [], [], None
    for _ in range(reps):
        g.fork()
        t = time.perf_counter()
        r = f()
        ts.append((time.perf_counter() - t) * 1e3)
        ks.append(g.filter_stats()["kernel_ms"])
        g.revert()
    return r, float(np.median(ts)), float(np.median(ks))


for brk in (True, False):
    one, one_ms, one_k = timed(lambda: g.try_schedule_pods(w.pending, w.order, half, brk, w.class_owner, w.hints, 0), 5)
    path = g.filter_stats()["path"]
    per, per_ms, _ = timed(lambda: try_schedule_ref(g, w.pending, w.order, half, brk, w.class_owner, w.hints, 0), 1)
    every, all_ms, all_k = timed(lambda: g.try_schedule_pods(w.pending, w.order, None, brk, w.class_owner, w.hints, 0), 5)
    ok = np.array_equal(one.node, per.node) and (one.evals, one.last_index, one.tried) == \
        (per.evals, per.last_index, per.tried)
    print(f"break={int(brk)} path={path} parity={ok} half-mask: tried={one.tried} placed={one.placed} "
          f"call_ms={one_ms:.2f} kernel_ms={one_k:.2f} | per-pod call_ms={per_ms:.1f} (x{per_ms / one_ms:.0f}) | "
          f"ALL: tried={every.tried} placed={every.placed} call_ms={all_ms:.2f} kernel_ms={all_k:.2f}", flush=True)
fo, fo_ms, fo_k = timed(lambda: g.filter_out_schedulable(w.pending, w.order, w.class_owner, w.hints, 0), 5)
print(f"filter_out_schedulable: placed={fo.placed} call_ms={fo_ms:.2f} kernel_ms={fo_k:.2f}", flush=True)
g.close()
