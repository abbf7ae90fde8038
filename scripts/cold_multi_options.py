"""Cold creation of the sharded Estimate plan: host lists against the option matrix against a
pod-groups handle (python scripts/cold_multi_options.py [--runs N] [--inner K] [--replicas D]).

Full C2 (50 000 pods, 100 node groups) over D replicas, which here are D mirrors on one device:
the numbers show the host work and the upload volume of each form, not scaling over devices.
Every sample is one plan creation plus the first resident run after it, the host clock around
each.  A form is measured in a fresh process (two warm creations, then K samples), and the
processes of the three forms alternate, N rounds; medians with quartiles over all samples of a
form.  Beside the times: the bytes each form uploads per block, and the device time of the
blocks' list kernels.  The first-run results of the three forms are compared.

Then the row-total pass alone (the one pass over `ok` ahead of the split) at 500 node groups x
50 000 singleton pod groups, read from the library's CASIM_DEBUG_TIMING line."""
import argparse
import json
import os
import re
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from autoscaler_amd import abi, native, workloads as W  # noqa: E402
from cold_options import append_loop, controllers, quart  # noqa: E402

FORMS = ("list", "options", "groups")


def child(form: str, replicas: int, inner: int) -> dict:
    w = W.c2()
    eg_off, eg_pod, ok = controllers(w)
    off, idx = append_loop(eg_off, eg_pod, ok)
    assert np.array_equal(off, w.group_off) and np.array_equal(idx, w.pod_idx)
    ms = [native.Mirror(0) for _ in range(replicas)]
    for m in ms:
        W.load_estimate(m, w)
    mm = native.Multi(ms)
    ps = pg = None
    if form == "groups":
        # the handle on replica 0, built from the pods in controller order: its CSR is (eg_off, eg_pod)
        ps = ms[0].podset(w.table)
        pg = ms[0].build_pod_groups(ps, order=eg_pod)
        g_off, g_pod = pg.fetch()
        assert np.array_equal(g_off, eg_off) and np.array_equal(g_pod, eg_pod)

    def make():
        if form == "list":
            return native.MultiEstimatePlan(mm, w.table, off, idx, w.templates)
        if form == "options":
            return native.MultiEstimatePlan.from_options(mm, w.table, eg_off, eg_pod, ok, w.templates)
        return native.MultiEstimatePlan.from_groups(mm, w.table, pg, ok, w.templates)

    clock = time.perf_counter
    for _ in range(2):                                  # warm: allocation cache, streams, code objects
        with make() as p:
            p.run(w.max_nodes, 0, device_results=True)
    create, first_run, lists_ms = [], [], []
    for _ in range(inner):
        t0 = clock()
        p = make()
        t1 = clock()
        r = p.run(w.max_nodes, 0, device_results=True)
        t2 = clock()
        create.append(t1 - t0)
        first_run.append(t2 - t1)
        lists_ms.append(p.lists_ms().tolist())
        bounds = p.stats()["block_first_group"]
        sched = p.fetch()
        p.close()
    rows = np.diff(bounds)
    items = np.diff(off[bounds])
    csr = 4 * len(eg_off) + 4 * len(eg_pod)
    up = (4 * items) if form == "list" else (csr + rows * ok.shape[1])
    out = {"form": form, "create": create, "first_run": first_run, "lists_ms": np.median(lists_ms, axis=0).tolist(),
           "blocks": bounds, "upload_bytes_per_block": [int(v) for v in up],
           "digest": zlib.crc32(r.results.tobytes() + sched.tobytes() + str(r.last_index).encode())}
    if pg is not None:
        pg.close()
        ps.close()
    mm.close()
    for m in ms:
        m.close()
    return out


def row_pass(replicas: int) -> None:
    """One creation at 500 x 50 000 singleton groups (a tenth of the pairs pass); the library
    prints the time of its row-total pass to stderr under CASIM_DEBUG_TIMING."""
    w = W.c2()
    n, G = len(w.table), 500
    rng = np.random.default_rng(1)
    ok = (rng.random((G, n)) < 0.1).astype(np.uint8)
    tm = np.ascontiguousarray(w.templates[np.arange(G) % len(w.templates)], dtype=abi.TEMPLATE_DTYPE)
    ms = [native.Mirror(0) for _ in range(replicas)]
    for m in ms:
        W.load_estimate(m, w)
    with native.Multi(ms) as mm:
        for _ in range(5):
            native.MultiEstimatePlan.from_options(mm, w.table, np.arange(n + 1, dtype=np.int32),
                                                  np.arange(n, dtype=np.int32), ok, tm).close()
    for m in ms:
        m.close()


def spawn(args: list, env=None) -> subprocess.CompletedProcess:
    return subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                          env=env, timeout=600, check=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--replicas", type=int, default=2)
    ap.add_argument("--child", choices=FORMS + ("rowpass",))
    a = ap.parse_args()
    if a.child == "rowpass":
        row_pass(a.replicas)
        return
    if a.child:
        print(json.dumps(child(a.child, a.replicas, a.inner)), flush=True)
        return
    got = {f: [] for f in FORMS}
    for _ in range(a.runs):
        for f in FORMS:                                 # a fresh process per form, the forms in turn
            line = spawn(["--child", f, "--replicas", str(a.replicas), "--inner", str(a.inner)]).stdout.splitlines()[-1]
            got[f].append(json.loads(line))
    out = {"workload": "C2: 50000 pods, 100 node groups", "replicas": a.replicas,
           "devices": "every replica on device 0: host work and upload volume, not scaling",
           "samples_per_form": a.runs * a.inner, "forms": {}}
    for f in FORMS:
        create = [v for r in got[f] for v in r["create"]]
        first = [v for r in got[f] for v in r["first_run"]]
        out["forms"][f] = {"create_ms": quart(create), "first_resident_run_ms": quart(first),
                           "create_plus_first_run_ms": quart(np.add(create, first)),
                           "blocks": got[f][0]["blocks"], "upload_bytes_per_block": got[f][0]["upload_bytes_per_block"],
                           "lists_kernel_ms_per_block": np.median([r["lists_ms"] for r in got[f]], axis=0).round(4).tolist()}
    out["first_run_results_equal"] = len({r["digest"] for f in FORMS for r in got[f][:1]}) == 1
    print(json.dumps(out), flush=True)
    env = dict(os.environ, CASIM_KNOBS="1", CASIM_DEBUG_TIMING="1")    # (the library reads knobs under CASIM_KNOBS)
    err = spawn(["--child", "rowpass", "--replicas", str(a.replicas)], env=env).stderr
    ms = [float(x) for x in re.findall(r"\[multi options\] row totals\s+([0-9.]+) ms", err)]
    if not ms:
        raise SystemExit("no row-total line on the child's stderr:\n" + err[-2000:])
    print(json.dumps({"row_total_pass": "500 node groups x 50000 singleton pod groups", "threads": a.replicas,
                      "ms": quart(np.asarray(ms) * 1e-3), "calls": len(ms)}), flush=True)


if __name__ == "__main__":
    main()
