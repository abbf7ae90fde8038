"""BuildPodGroups on the device against the host loop at C5
(python scripts/pod_groups_timing.py [--runs N] [--small] [--host-only]).

One FilterOutSchedulable run on the full C5 loop workload gives the verdicts; then, on the one
resident pod set, the span of runonce.run between the filter's return and the start of the
Estimate run is repeated, alternating the two forms in one process: the grouping, the expansion
check (one resident ExpansionPlan for both) and, on the host form, the CSR the option form of
the plan takes.  The same with every pending pod unschedulable (node = -1 everywhere).  Medians
with quartiles of the host clock; the device time of the build from ca_pod_groups_timings; the
groups of both forms are compared.  --host-only runs what a tree without the device form has
(the parent commit), for the comparison in one job."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autoscaler_amd import abi, native, runonce, workloads as W  # noqa: E402


def quart(v):
    q = np.percentile(np.asarray(v) * 1e3, [25, 50, 75])
    return {"q1": round(float(q[0]), 3), "median": round(float(q[1]), 3), "q3": round(float(q[2]), 3)}


def host_span(f, node, ps, expand, templates):
    """runonce.run's host form between the filter and the Estimate run."""
    t0 = time.perf_counter()
    unsched = f.order[node < 0]
    groups = runonce._equivalence_groups(f.pending.pods, unsched)
    samples = np.array([g[0] for g in groups], np.int32)
    t1 = time.perf_counter()
    expand(None, ps, samples, templates)
    t2 = time.perf_counter()
    eg_off = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=eg_off[1:])
    eg_pod = np.fromiter((i for g in groups for i in g), np.int32, int(eg_off[-1]))
    t3 = time.perf_counter()
    return t3 - t0, (t1 - t0) + (t3 - t2), (eg_off, eg_pod)


def device_span(m, f, node, ps, expand, templates):
    t0 = time.perf_counter()
    pg = m.build_pod_groups(ps, order=f.order, node=node, class_owner=None)
    t1 = time.perf_counter()
    expand(None, ps, None, templates, groups=pg)
    t2 = time.perf_counter()
    return t2 - t0, t1 - t0, pg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--small", action="store_true", help="a reduced C5 (rehearsal)")
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    if native.device_count() < 1:
        raise SystemExit("no HIP device visible")
    w = runonce.c5_runonce(n_nodes=800, n_pending=2000, n_groups=16) if a.small else runonce.c5_runonce()
    f = w.filt
    m = native.Mirror(0)
    W.load_filter(m, f)
    ps = m.podset(f.pending)
    fo = m.filter_out_schedulable(f.pending, f.order, f.class_owner, f.hints, 0, podset=ps)
    plan = native.ExpansionPlan(m, w.templates)

    def expand(_, podset, samples, templates, groups=None):
        return plan.run(podset, samples, verdict_only=True, **({"groups": groups} if groups is not None else {}))

    out = {"device_form": not a.host_only, "runs": a.runs}
    for label, node in (("c5", fo.node.copy()), ("all_unschedulable", np.full(len(f.order), -1, np.int32))):
        span = {"host": [], "device": []}
        part = {"host": [], "device": []}
        dev_ms, launches, same, same_ds, n_dev = [], 0, None, None, 0
        for rep in range(a.runs + 2):                       # (two warm-up rounds dropped)
            s, p, csr = host_span(f, node, ps, expand, w.templates)
            if rep >= 2:
                span["host"].append(s)
                part["host"].append(p)
            if a.host_only:
                continue
            s, p, pg = device_span(m, f, node, ps, expand, w.templates)
            t = pg.timings()
            if rep >= 2:
                span["device"].append(s)
                part["device"].append(p)
                dev_ms.append(t["build_ms"] * 1e-3)
            launches = t["launches"]
            if same is None:
                eg_off, eg_pod = pg.fetch()
                same = bool(np.array_equal(eg_off, csr[0]) and np.array_equal(eg_pod, csr[1]))
                # the host helper with groups.go:68-72 applied (a DaemonSet pod alone), which it leaves out
                pods = f.pending.pods.copy()
                pods["similar_class"][(pods["flags"] & abi.CA_POD_DAEMONSET) != 0] = -1
                ds_groups = runonce._equivalence_groups(pods, f.order[node < 0])
                n_dev = pg.n_groups
                same_ds = [eg_pod[eg_off[e]:eg_off[e + 1]].tolist() for e in range(n_dev)] == ds_groups
            pg.close()
        r = {"pods": int((node < 0).sum()), "groups_host": int(len(csr[0]) - 1),
             "host_span_ms": quart(span["host"]), "host_grouping_and_csr_ms": quart(part["host"])}
        if not a.host_only:
            r.update({"device_span_ms": quart(span["device"]), "build_pod_groups_wall_ms": quart(part["device"]),
                      "build_device_ms": quart(dev_ms), "launches": launches, "groups_device": n_dev, "groups_equal_host": same,
                      "groups_equal_host_with_daemonset_rule": same_ds,
                      "daemonset_pods_listed": int(((f.pending.pods["flags"][f.order[node < 0]]
                                                     & abi.CA_POD_DAEMONSET) != 0).sum())})
        out[label] = r
    plan.close()
    ps.close()
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
