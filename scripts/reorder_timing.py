"""A new node order on the C5 filter cluster (15 000 nodes, 300 000 pods, loaded once), two
forms alternating in one process (python scripts/reorder_timing.py [reps] [out file]):

  (a) reorder: ca_mirror_reorder_nodes with a seeded random permutation, then one FitsAnyNode;
  (b) reload: ca_mirror_clear, the nodes and the pods added again in that order, then one
      FitsAnyNode — the only way before the call existed.

The host clock runs around each form; both end in the FitsAnyNode's synchronise.  The
permuted node records and pod positions of (b) are built before its clock starts (a caller
has them from its own lists).  Writes the medians, the quartiles and the device time of the
reorder (ca_mirror_reorder_stats [2]) to the out file (default profiles/reorder_c5.txt)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from autoscaler_amd import native, workloads as W  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reorder_c5.txt")
w = W.c5_filter()
g = native.Mirror(0)
W.load_filter(g, w)
n, n_pods = len(w.nodes), len(w.table)
every = np.arange(n_pods, dtype=np.int32)
rng = np.random.default_rng(5)
nodes, pod_node = w.nodes.copy(), np.ascontiguousarray(w.pod_node, dtype=np.int32)
L = 0


def scan():
    global L
    node, L, _, _ = g.fits_any_node(w.pending, 0, None, L)
    return node


def step(order):
    """The host's own copy of the lists in the new order."""
    global nodes, pod_node
    inv = np.zeros(n, np.int32)
    inv[order] = np.arange(n, dtype=np.int32)
    nodes, pod_node = np.ascontiguousarray(nodes[order]), np.ascontiguousarray(inv[pod_node])


def form_reorder():
    order = rng.permutation(n).astype(np.int32)
    t0 = time.perf_counter()
    g.reorder_nodes(order)
    got = scan()
    t1 = time.perf_counter()
    step(order)
    return (t1 - t0) * 1e3, got, g.reorder_stats()


def form_reload():
    order = rng.permutation(n).astype(np.int32)
    step(order)
    t0 = time.perf_counter()
    g.clear()
    g.add_nodes(nodes)
    g.add_pods(w.table, every, pod_node)
    got = scan()
    t1 = time.perf_counter()
    return (t1 - t0) * 1e3, got


scan()
for _ in range(3):
    form_reorder()
    form_reload()
A, B, K = [], [], []
for _ in range(reps):
    before = g.reorder_stats()
    a = form_reorder()
    assert (a[2][0], a[2][1]) == (before[0] + 1, before[1] + 1), "the reorder did not run on the device"
    # the scan after the reorder answers for the node the host's own list has there
    there = np.nonzero(pod_node == a[1])[0]
    assert there.size == 0 or g.pod_node(int(there[0])) == a[1]
    K.append(a[2][2])
    A.append(a[0])
    B.append(form_reload()[0])
qa, qb = np.percentile(A, [25, 50, 75]), np.percentile(B, [25, 50, 75])
lines = [
    f"C5 filter cluster: {n} nodes, {n_pods} pods, {reps} alternating repeats after 3 warm-up rounds (host clock, ms)",
    f"(a) reorder_nodes + FitsAnyNode        : median {qa[1]:.3f}  quartiles {qa[0]:.3f} .. {qa[2]:.3f}",
    f"(b) clear + reload + FitsAnyNode       : median {qb[1]:.3f}  quartiles {qb[0]:.3f} .. {qb[2]:.3f}",
    f"device time of the reorder (HIP events): median {np.median(K):.0f} us  quartiles "
    f"{np.percentile(K, 25):.0f} .. {np.percentile(K, 75):.0f} us "
    f"({n * 208 / 1e6:.1f} MB of rows gathered into scratch and copied back)",
    f"(a) upper quartile {'below' if qa[2] < qb[0] else 'NOT below'} (b) lower quartile: "
    f"{qa[2]:.3f} vs {qb[0]:.3f} ms ({qb[1] / qa[1]:.1f}x at the medians)",
]
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
g.close()
