"""Cold Estimate plan creation, host lists against the option matrix
(python scripts/cold_options.py [--runs N] [--skip-c5]).

Full C2: EstimatePlan(...) on the workload's lists against EstimatePlan.from_options(...) on
optgen-style options (the controllers as equivalence groups and the matrix of the lists), on
one resident podset, alternating in one process with the buffers coming from the allocation
cache; the host clock around the constructor, and around the first run after it.  The same
with the caller's side included: the append loop (numpy) for the host form, the CSR for the
option form.  Then runonce's Estimate leg at C5 in both forms.  Medians with quartiles; the
two plans' first-run results are compared at the end.  k_option_lists' device time (HIP
events) and the bytes it moves are printed against the 8 TB/s HBM bound."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoscaler_amd import native, runonce, workloads as W  # noqa: E402


def controllers(w):
    """(eg_off, eg_pod, ok): the pods of one similar_class in pod order, and ok[g][e] = the
    group's first pod is in list g (C2's lists are whole controllers)."""
    sc = np.asarray(w.table.pods["similar_class"])
    order = np.argsort(sc, kind="stable").astype(np.int32)
    _, first, counts = np.unique(sc[order], return_index=True, return_counts=True)
    eg_off = np.zeros(len(first) + 1, np.int32)
    np.cumsum(counts, out=eg_off[1:])
    sample = order[first]
    G = len(w.templates)
    ok = np.zeros((G, len(first)), np.uint8)
    member = np.zeros(len(w.table), bool)
    for g in range(G):
        member[:] = False
        member[w.pod_idx[w.group_off[g]:w.group_off[g + 1]]] = True
        ok[g] = member[sample]
    return eg_off, order, ok


def append_loop(eg_off, eg_pod, ok):
    off, parts = [0], []
    for g in range(ok.shape[0]):
        segs = [eg_pod[eg_off[e]:eg_off[e + 1]] for e in np.nonzero(ok[g])[0]]
        parts.extend(segs)
        off.append(off[-1] + sum(len(s) for s in segs))
    return np.array(off, np.int32), (np.concatenate(parts) if parts else np.zeros(0, np.int32))


def quart(v):
    q = np.percentile(np.asarray(v) * 1e3, [25, 50, 75])
    return {"q1": round(float(q[0]), 3), "median": round(float(q[1]), 3), "q3": round(float(q[2]), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--skip-c5", action="store_true")
    a = ap.parse_args()
    w = W.c2()
    eg_off, eg_pod, ok = controllers(w)
    off, idx = append_loop(eg_off, eg_pod, ok)
    assert np.array_equal(off, w.group_off) and np.array_equal(idx, w.pod_idx)
    m = native.Mirror(0)
    W.load_estimate(m, w)
    ps = m.podset(w.table)
    clock = time.perf_counter
    for _ in range(2):                                  # warm: allocation cache, streams, code objects
        with native.EstimatePlan(m, w.table, off, idx, w.templates, podset=ps) as p:
            p.run_u16(w.max_nodes, 0, copy=False)
        with native.EstimatePlan.from_options(m, ps, eg_off, eg_pod, ok, w.templates) as p:
            p.run_u16(w.max_nodes, 0, copy=False)
    t = {k: [] for k in ("host_create", "host_first_run", "host_with_caller", "options_create", "options_first_run",
                         "options_with_caller")}
    kernel_ms, first = [], {}
    for _ in range(a.runs):
        t0 = clock()
        o2, i2 = append_loop(eg_off, eg_pod, ok)        # the caller's side of the host form
        t1 = clock()
        with native.EstimatePlan(m, w.table, o2, i2, w.templates, podset=ps) as p:
            t2 = clock()
            r = p.run_u16(w.max_nodes, 0)
            t3 = clock()
        t["host_create"].append(t2 - t1)
        t["host_with_caller"].append(t2 - t0)
        t["host_first_run"].append(t3 - t2)
        first["host"] = (r.results.tobytes(), r.sched_pod.tobytes(), r.last_index)
        t0 = clock()
        sc = np.asarray(w.table.pods["similar_class"])          # the caller's side of the option form: the CSR
        q2 = np.argsort(sc, kind="stable").astype(np.int32)
        e2 = np.zeros(len(eg_off), np.int32)
        np.cumsum(np.bincount(sc, minlength=len(eg_off) - 1), out=e2[1:])
        t1 = clock()
        with native.EstimatePlan.from_options(m, ps, e2, q2, ok, w.templates) as p:
            t2 = clock()
            r = p.run_u16(w.max_nodes, 0)
            t3 = clock()
            kernel_ms.append(p.stats()["option_lists_ms"])
        t["options_create"].append(t2 - t1)
        t["options_with_caller"].append(t2 - t0)
        t["options_first_run"].append(t3 - t2)
        first["options"] = (r.results.tobytes(), r.sched_pod.tobytes(), r.last_index)
    out = {"workload": "C2", "items": int(off[-1]), "pods": len(w.table), "n_eg": len(eg_off) - 1,
           "groups": len(w.templates), "runs": a.runs, "ms": {k: quart(v) for k, v in t.items()},
           "first_run_results_equal": first["host"] == first["options"]}
    k = float(np.median(kernel_ms))
    moved = 3 * 4 * int(off[-1])                        # eg_pod read, pod_idx and item_cls written (+ the class gather)
    out["k_option_lists"] = {"ms": round(k, 4), "bytes": moved,
                             "tb_per_s": round(moved / (k * 1e-3) / 1e12, 3) if k > 0 else None,
                             "share_of_8_tb_per_s": round(moved / (k * 1e-3) / 8e12, 3) if k > 0 else None}
    out["uploads"] = {"host_lists_bytes": 4 * int(off[-1]), "options_bytes": 4 * len(eg_off) + 4 * len(eg_pod) + ok.size}
    out["device_default_rule"] = out["ms"]["options_create"]["median"] < out["ms"]["host_create"]["q1"]
    ps.close()
    m.close()
    print(json.dumps(out), flush=True)
    if a.skip_c5:
        return
    w5 = runonce.c5_runonce()
    leg = {"device": [], "host": []}
    res = {}
    for _ in range(max(3, a.runs // 2)):
        for form in ("host", "device"):
            m = native.Mirror(0)
            W.load_filter(m, w5.filt)
            util = runonce.DeviceUtil(0)
            r = runonce.run(m, util, w5, expand_fn=runonce.DeviceExpansion(), option_lists=form)
            util.close()
            m.close()
            leg[form].append(r.ms["estimate"] * 1e-3)
            res[form] = (r.est_results.tobytes(), r.est_sched.tobytes(), r.last_index)
    print(json.dumps({"workload": "C5 runonce, Estimate leg", "ms": {k: quart(v) for k, v in leg.items()},
                      "results_equal": res["host"] == res["device"], "sizes": r.sizes}), flush=True)


if __name__ == "__main__":
    main()
