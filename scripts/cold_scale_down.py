"""Steps 4-5 of the loop up to the sweep's own run, four ways
(python scripts/cold_scale_down.py [--runs N] [--nodes N --pending N]).

Full C5 after FilterOutSchedulable, one mirror, the four forms alternating in one process:

1. host, cold: what a caller pays every loop on a new snapshot: the utilization rows of every
   node and pod (UtilInput with nothing cached), a new ca_util_table and its calculate
   (DeviceUtil), the numpy split into empty nodes and candidates, the argsort and the Python
   loop for the pods to move, and RemovalPlan(...) on those lists.
2. host, cached: the same with the loop's starting rows cached on the workload and the table
   resident, only FilterOutSchedulable's placements sent again (ca_util_table_set_added).
3. device: ScaleDownCandidates on the mirror's own state and its removal_plan().  The host's
   drain verdicts go in as override rows; finding the pods whose verdict is not the default (a
   scan of every record's flags here; the host forms assume "all movable" and pay nothing) is
   timed on its own as device_overrides.
4. resident: the same handle from the mirror's resident pod columns (resident=True).  The running
   pods' verdicts are resident rows set once before the rounds; a steady-state round sets only
   the rows of this loop's DaemonSet placements, and no override is sent.

Host clock around each form, medians with quartiles; form 3's device times, its pod -> node
staging time and the bytes each form moves across PCIe (form 4: its column sync and the device
time of its move-list kernels).  The lists of the four forms are compared at the end."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoscaler_amd import abi, native, runonce, workloads as W  # noqa: E402


def host_lists(w, fo, util):
    """runonce.run's host glue between the utilization rows and the sweep."""
    f = w.filt
    low = np.nonzero((util["status"] == 0) & (util["utilization"] < runonce.UTIL_THRESHOLD))[0].astype(np.int32)
    empty = low[util["empty"][low] != 0]
    cand = low[util["empty"][low] == 0]
    P = len(f.table)
    placed = np.nonzero(fo.node >= 0)[0]
    pod_node = np.concatenate([f.pod_node, fo.node[placed]]).astype(np.int64)
    pod_id = np.concatenate([np.arange(P, dtype=np.int32), fo.pod_id[placed]])
    order = np.argsort(pod_node, kind="stable")
    node_first = np.zeros(len(f.nodes) + 1, np.int64)
    np.cumsum(np.bincount(pod_node, minlength=len(f.nodes)), out=node_first[1:])
    move_off, moves = [0], []
    for c in cand.tolist():
        ids = pod_id[order[node_first[c]:node_first[c + 1]]]
        moves.append(ids)
        move_off.append(move_off[-1] + len(ids))
    move_pods = np.concatenate(moves).astype(np.int32) if moves else np.zeros(0, np.int32)
    return empty, cand, np.array(move_off, np.int32), move_pods


def host_form(m, w, fo, du):
    ui = runonce.UtilInput(w, fo.node, "added", du.zeros)
    util = du(ui, w.now_ns)
    empty, cand, off, moves = host_lists(w, fo, util)
    plan = native.RemovalPlan(m, cand, np.ones(len(w.filt.nodes), np.uint8), np.zeros(len(cand), np.int32), off, moves)
    return plan, (empty, cand, off, moves), ui


def quart(v):
    q = np.percentile(np.asarray(v) * 1e3, [25, 50, 75])
    return {"q1": round(float(q[0]), 3), "median": round(float(q[1]), 3), "q3": round(float(q[2]), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--nodes", type=int, default=15_000)
    ap.add_argument("--pending", type=int, default=20_000)
    a = ap.parse_args()
    w = runonce.c5_runonce(n_nodes=a.nodes, n_pending=a.pending)
    f = w.filt
    m = native.Mirror(0)
    W.load_filter(m, f)
    fo = m.filter_out_schedulable(f.pending, f.order, f.class_owner, f.hints, 0)
    n, n_pods, n_placed = len(f.nodes), len(f.table), int((fo.node >= 0).sum())
    clock = time.perf_counter
    cached, cold = runonce.DeviceUtil(0), runonce.DeviceUtil(0)
    w_cold = dataclasses.replace(w)                     # its own row cache, dropped before every round
    t = {"host_cold": [], "host_cached": [], "device": [], "device_overrides": [], "resident": []}
    dev_t, res_t, res_up, lists = [], [], [], {}
    placed = np.nonzero(fo.node >= 0)[0]
    # what a shim does as pods enter the snapshot, outside the loop: the running pods' verdicts
    running = np.arange(n_pods, dtype=np.int32)
    m.set_pod_util_rows(*runonce._movable_rows(f.table.pods, running, running))
    for k in range(a.runs + 2):                         # two warm rounds: allocation cache, code objects, page-locked rows
        w_cold._ubase = None                            # a new snapshot: new rows, so a new table
        t0 = clock()
        plan, lists["host_cold"], _ = host_form(m, w_cold, fo, cold)
        t1 = clock()
        plan.close()
        t2 = clock()
        plan, lists["host_cached"], ui = host_form(m, w, fo, cached)
        t3 = clock()
        plan.close()
        t_over = clock()
        over = runonce.scale_down_overrides(w, fo)          # the host's drain verdicts that differ from the default
        t4 = clock()
        sd = m.scale_down_candidates(False, False, w.now_ns, runonce.UTIL_THRESHOLD, runonce.UTIL_THRESHOLD,
                                     pod_over=over)
        plan = sd.removal_plan()
        t5 = clock()
        ls = sd.fetch()
        lists["device"] = (ls.empty, ls.cand, ls.move_off, ls.move_pods)
        tm = sd.timings()
        plan.close()
        sd.close()
        new_ids, new_rows = runonce._movable_rows(f.pending.pods, f.order[placed], fo.pod_id[placed])
        m.set_pod_util_rows(new_ids, None)              # (untimed: a row set again unchanged is not sent; every
        up0 = m.pod_column_stats()["bytes_uploaded"]    # round's placements are new to the mirror, as in a real loop)
        t6 = clock()
        m.set_pod_util_rows(*runonce._movable_rows(f.pending.pods, f.order[placed], fo.pod_id[placed]))
        sd = m.scale_down_candidates(False, False, w.now_ns, runonce.UTIL_THRESHOLD, runonce.UTIL_THRESHOLD,
                                     resident=True)
        plan = sd.removal_plan()
        t7 = clock()
        ls = sd.fetch()
        lists["resident"] = (ls.empty, ls.cand, ls.move_off, ls.move_pods)
        tr = sd.timings()
        plan.close()
        sd.close()
        if k >= 2:
            t["resident"].append(t7 - t6)
            res_t.append(tr)
            res_up.append(m.pod_column_stats()["bytes_uploaded"] - up0)
            t["host_cold"].append(t1 - t0)
            t["host_cached"].append(t3 - t2)
            t["device"].append(t5 - t4)
            t["device_overrides"].append(t4 - t_over)
            dev_t.append(tm)
    m_stats = m.pod_column_stats()
    cached.close()
    cold.close()
    m.close()
    C, M = len(lists["device"][1]), len(lists["device"][3])
    plan_up = 4 * (3 * C + 1 + 2 * M) + n
    up_added = (4 + abi.UTIL_POD_DTYPE.itemsize) * n_placed
    up_base = abi.UTIL_NODE_DTYPE.itemsize * n + 4 * (n + 1) + abi.UTIL_POD_DTYPE.itemsize * n_pods
    info = abi.UTIL_INFO_DTYPE.itemsize * n
    med = lambda key, rows=dev_t: float(np.median([d[key] for d in rows]))         # noqa: E731
    out = {
        "workload": "C5 after FilterOutSchedulable", "nodes": n, "mirror_pods": n_pods + n_placed, "placed": n_placed,
        "candidates": C, "empty": len(lists["device"][0]), "pods_to_move": M, "runs": a.runs,
        "ms": {k: quart(v) for k, v in t.items()},
        "device_parts_ms": {k: round(med(k), 4) for k in ("util_kernel_ms", "classify_kernel_ms", "stage_ms",
                                                          "move_lists_ms", "create_ms")},
        # resident: stage_ms is the host time of the column sync, move_lists_ms the device time of the move-list kernels
        "resident_parts_ms": {k: round(med(k, res_t), 4) for k in ("util_kernel_ms", "classify_kernel_ms", "stage_ms",
                                                                   "move_lists_ms", "create_ms")},
        "column_stats": m_stats,
        "pcie_bytes": {"host_cold": {"h2d": up_base + up_added + plan_up, "d2h": info},
                       "host_cached": {"h2d": up_added + plan_up, "d2h": info},
                       "device": {"h2d": int(med("h2d_bytes")) + plan_up, "d2h": int(med("d2h_bytes"))},
                       "resident": {"h2d": int(med("h2d_bytes", res_t)) + int(np.median(res_up)) + plan_up,
                                    "d2h": int(med("d2h_bytes", res_t))}},
        "lists_equal": all(np.array_equal(x, y) for form in ("host_cold", "host_cached", "resident")
                           for x, y in zip(lists[form], lists["device"])),
    }
    dev = out["ms"]["device"]["median"] + out["ms"]["device_overrides"]["median"]
    out["device_beats_cached"] = dev < out["ms"]["host_cached"]["q1"]
    out["device_beats_cold"] = dev < out["ms"]["host_cold"]["q1"]
    out["resident_q3_below_cached_q1"] = out["ms"]["resident"]["q3"] < out["ms"]["host_cached"]["q1"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
