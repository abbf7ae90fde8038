"""FilterOutSchedulable / TrySchedulePods cases planted at the widths the two kernels of
csrc/filter.hip are built around (64-bit words, 64 pods per batch, the 64-position window of
a mixed run, 64 live shapes, 1 024 collected shapes, the row-by-row limit of 24, the 160 KiB
of LDS, the 512-row window, 64 staged slots, 8 192 ring positions per pass, 10 classes per
controller), from raw ABI records: every free value, slot count, flag and hint is chosen.

A `Ring` holds the rows as the kernels see them (free cpu / memory / ephemeral storage / pod
slots per node); `build` turns them into node records whose allocatable is free + the
residents' requests (every third node runs one resident pod).  A row is closed unless opened:
a closed row misses the standard pod `A` by one unit in one dimension, and the dimension
rotates with the node (cpu, memory, ephemeral storage, pod slots), so each of the four binds
somewhere in every case.  Every other shape requests at least `A` in every dimension, or
nothing at all (the all-zero shape, which fits every row with a free slot).

Every case has a name ("family/..."), the kernels it can run on (`paths`), and `claims`: what
it is placed at, in terms tests/test_filter_cases.py checks from numpy and the oracle's
output alone:

  placed k                  last_index L                wraps (a scan placement behind the ring's end)
  keeps_last_index          nothing is placed by a scan: lastIndex comes back as it went in
  nodes {position: node}    evals k                     overflowing k
  on_node (x, m, k)         m pods are hinted to node x, exactly k of them land there
  hint_in_window {position: bool}   the pod's hinted node lies in [L, L + 64) when its turn comes
  shapes (live, dead)       distinct request shapes of the walk that fit some / no node
  tried k                   (with the case's own match and break) pods processed
  lds                       a dict checked against fb_lds (see test_filter_cases.check_lds)
  route                     what Mirror.filter_stats() must report for FilterOutSchedulable:
                            steps (block_steps, ring_scans, windows) on the bitmap walk,
                            window "resident" | "moves" on the window kernel; path, shapes,
                            static_classes and static_in_lds come from `route()` below."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from autoscaler_amd import abi

MI, GI = 1 << 20, 1 << 30
A = (100, 100 * MI, GI)                      # the standard pod
B = (150, 120 * MI, GI + MI)
ZERO = (0, 0, 0)                             # the all-zero request shape
BIG = (10 ** 7, 1 << 45, 1 << 45, 1000)      # a dimension that never binds
DEAD = (10 ** 8, 100 * MI, GI)               # a request no node has
RESIDENT = (70, 64 * MI, GI // 2)

# the widths of csrc/filter.hip
FB_T = 64
FB_MAX_SHAPES = 64
FB_COLLECT_SHAPES = 1024
FB_ROWWISE_MAX = 24
FB_LDS_MAX = 160 * 1024
SQ_WIN, SQ_SLOTS, SQ_PASS = 512, 64, 512 * 16
FO_MAX_PER_OWNER = 10
SIZEOF_FBSHAPE, SIZEOF_FBROW, SIZEOF_FBTHR = 32, 32, 3120

PF = abi.CA_POD_PREFILTER_FAIL
DS = abi.CA_POD_DAEMONSET
TOL = abi.CA_POD_TOLERATES_UNSCHED


def fb_lds(S: int, NW: int, K: int, stat_in_lds: bool, n_classes: int, n_owners: int, masked: bool) -> int:
    """The LDS bytes of k_fb_walk (fb_lds of filter.hip, struct sizes written out)."""
    a16 = lambda x: (x + 15) & ~15                                              # noqa: E731
    t = SIZEOF_FBSHAPE * max(S, 1)             # shapes
    t += 8 * S * NW                            # dyn words
    t += 8 * NW if masked else 0               # vis, when the scans read vis & acc
    t += 8 * NW                                # svis
    t += 8 * K * NW if stat_in_lds else 0      # static words
    t += a16(4 * (NW + 1))                     # prefix counts
    t += 4 * FB_T                              # a run's nodes
    t += SIZEOF_FBROW * FB_T                   # the batch's rows
    t += 4 * FB_T                              # their nodes
    t += 8 * NW                                # dirty bits
    t += a16(4 * max(n_owners, 1))             # classes per controller
    t += a16(max(n_classes, 1))                # marks
    t += a16(max(n_owners, 1))                 # overflowing controllers
    return t + SIZEOF_FBTHR


def words(n: int) -> int:
    return (n + 63) // 64


@dataclass
class FiltCase:
    name: str
    nodes: np.ndarray
    resident: abi.PodTable
    resident_node: np.ndarray
    pending: abi.PodTable
    order: np.ndarray
    class_owner: np.ndarray | None
    hints: np.ndarray
    L0: int
    paths: tuple = ("bitmap", "window")
    claims: dict = field(default_factory=dict)
    match: tuple | None = None               # the case's own TrySchedulePods call
    brk: bool = False

    @property
    def family(self) -> str:
        return self.name.split("/")[0]

    def load(self, b) -> None:
        b.clear()
        b.add_nodes(self.nodes)
        if len(self.resident):
            b.add_pods(self.resident, np.arange(len(self.resident), dtype=np.int32), self.resident_node)

    def filter(self, b, hints=None, L=None):
        return b.filter_out_schedulable(self.pending, self.order, self.class_owner,
                                        self.hints if hints is None else hints, self.L0 if L is None else L)

    def free_rows(self) -> np.ndarray:
        """[n][4] free cpu, memory, ephemeral storage, slots from the records alone."""
        f = np.stack([self.nodes[k].astype(np.int64) for k in
                      ("alloc_milli_cpu", "alloc_memory", "alloc_ephemeral", "alloc_pods")], axis=1)
        r = self.resident.pods
        for i, x in enumerate(self.resident_node.tolist()):
            f[x] -= [int(r[i]["req_milli_cpu"]), int(r[i]["req_memory"]), int(r[i]["req_ephemeral"]), 1]
        return f


class Ring:
    def __init__(self, n: int, loose: int = 0, shape=A):
        """n closed rows; loose > 0: every row has room for `loose` pods of `shape` instead."""
        self.n = n
        self.free = np.zeros((n, 4), np.int64)
        self.unsched = np.zeros(n, bool)
        self.taints = np.zeros(n, np.uint64)
        self.scalar = np.zeros(n, np.int64)
        self.pods: list = []
        self.res_ports: dict = {}                      # node -> port bit of its resident pod
        for i in range(n):
            if loose:
                self.open(i, loose, shape)
            else:
                self.close(i)

    def close(self, i: int, kind: int | None = None) -> None:
        kind = i % 4 if kind is None else kind
        self.free[i] = BIG
        self.free[i][kind] = 0 if kind == 3 else A[kind] - 1

    def open(self, i: int, k: int = 1, shape=A, bind: int | None = None) -> None:
        """Room for exactly k pods of `shape`; `bind`: the dimension that runs out."""
        bind = i % 4 if bind is None else bind
        self.free[i] = BIG
        self.free[i][bind] = k if bind == 3 else k * shape[bind]

    def raw(self, i: int, cpu: int, mem: int, eph: int, slots: int) -> None:
        self.free[i] = (cpu, mem, eph, slots)

    def pod(self, shape=A, hint: int = -1, cls: int = -1, flags: int = 0, tol: int = 0, port: int | None = None,
            scalar: int = 0, names=None) -> int:
        self.pods.append(dict(shape=shape, hint=hint, cls=cls, flags=flags, tol=tol, port=port, scalar=scalar,
                              names=names))
        return len(self.pods) - 1

    def fill(self, k: int) -> None:
        """k pods that no node passes PreFilter for (no class): they only take positions."""
        for _ in range(k):
            self.pod(A, flags=PF)

    def build(self, name: str, claims: dict, L0: int = 0, paths=("bitmap", "window"), class_owner="own",
              match=None, brk=False) -> FiltCase:
        n, P = self.n, len(self.pods)
        has_res = [i % 3 == 1 or i in self.res_ports for i in range(n)]
        nodes = abi.empty_nodes(n)
        rn = [i for i in range(n) if has_res[i]]
        res = abi.empty_pods(len(rn))
        for k, i in enumerate(rn):
            res[k]["req_milli_cpu"], res[k]["req_memory"], res[k]["req_ephemeral"] = RESIDENT
            res[k]["score_milli_cpu"], res[k]["score_memory"] = RESIDENT[:2]
            if i in self.res_ports:
                b = self.res_ports[i]
                res[k]["port_use"][b >> 6] = res[k]["port_conflict"][b >> 6] = np.uint64(1 << (b & 63))
        for i in range(n):
            used = RESIDENT if has_res[i] else (0, 0, 0)
            nodes[i]["alloc_milli_cpu"] = self.free[i][0] + used[0]
            nodes[i]["alloc_memory"] = self.free[i][1] + used[1]
            nodes[i]["alloc_ephemeral"] = self.free[i][2] + used[2]
            nodes[i]["alloc_pods"] = self.free[i][3] + (1 if has_res[i] else 0)
            nodes["alloc_scalar"][i, 0] = self.scalar[i]
            nodes[i]["taints"] = self.taints[i]
            nodes[i]["flags"] = abi.CA_NODE_UNSCHEDULABLE if self.unsched[i] else 0
            nodes[i]["name_id"] = 1000 + i
        rec = abi.empty_pods(P)
        names: list = []
        for k, p in enumerate(self.pods):
            c, m, e = p["shape"]
            rec[k]["req_milli_cpu"], rec[k]["req_memory"], rec[k]["req_ephemeral"] = c, m, e
            rec[k]["score_milli_cpu"], rec[k]["score_memory"] = c, m
            rec[k]["similar_class"] = p["cls"]
            rec[k]["tolerated_taints"] = np.uint64(p["tol"])
            fl = p["flags"]
            if p["port"] is not None:
                b = p["port"]
                rec[k]["port_use"][b >> 6] = rec[k]["port_conflict"][b >> 6] = np.uint64(1 << (b & 63))
            if p["scalar"]:
                rec[k]["req_scalar"][0] = p["scalar"]
                fl |= abi.CA_POD_HAS_SCALAR_KEYS | abi.CA_POD_HAS_NONTPU_SCALAR_KEYS
            if p["names"] is not None:
                rec[k]["prefilter_first"], rec[k]["prefilter_count"] = len(names), len(p["names"])
                names.extend(1000 + x for x in p["names"])
                fl |= abi.CA_POD_PREFILTER_NAMES
            rec[k]["flags"] = fl
        n_cls = max([p["cls"] for p in self.pods], default=-1) + 1
        owner = np.arange(n_cls, dtype=np.int32) if isinstance(class_owner, str) else class_owner
        table = abi.PodTable(rec, names=np.array(names, np.int32)) if names else abi.PodTable(rec)
        return FiltCase(name, nodes, abi.PodTable(res), np.array(rn, np.int32), table, np.arange(P, dtype=np.int32),
                        None if owner is None else np.asarray(owner, np.int32),
                        np.array([p["hint"] for p in self.pods], np.int32).reshape(P), L0, tuple(paths), dict(claims),
                        match, brk)


# ---------------------------------------------------------------------------
# the route a call must take (the host side of try_schedule_core, restated)
# ---------------------------------------------------------------------------
def shapes_of(case: FiltCase):
    """(live, dead) distinct request shapes of the walk, or None when the walk meets a host
    port, a scalar request, PreFilter node names or a 1 025th distinct shape first."""
    p = case.pending.pods[case.order]
    free = case.free_rows()
    open_rows = free[free[:, 3] >= 1]
    seen: dict = {}
    for r in p:
        if r["port_use"].any() or r["port_conflict"].any() or r["req_scalar"].any() or \
                (int(r["flags"]) & abi.CA_POD_PREFILTER_NAMES):
            return None
        key = (int(r["req_milli_cpu"]), int(r["req_memory"]), int(r["req_ephemeral"]),
               bool(int(r["flags"]) & abi.CA_POD_HAS_SCALAR_KEYS))
        if key not in seen:
            if len(seen) >= FB_COLLECT_SHAPES:
                return None
            c, m, e, keys = key
            zero = (c, m, e) == (0, 0, 0) and not keys
            seen[key] = bool(len(open_rows)) and (zero or bool(
                ((open_rows[:, 0] >= c) & (open_rows[:, 1] >= m) & (open_rows[:, 2] >= e)).any()))
    live = sum(seen.values())
    return live, len(seen) - live


def route(case: FiltCase, masked: bool = False, forced_window: bool = False) -> dict:
    """path, shapes, static_classes and static_in_lds of a call on `case`."""
    window = dict(path="window", shapes=0, static_classes=0, static_in_lds=False)
    n = len(case.nodes)
    sh = None if forced_window or n == 0 else shapes_of(case)
    if sh is None or sh[0] > FB_MAX_SHAPES:
        return window
    S = sh[0] + (1 if sh[1] else 0)
    p = case.pending.pods[case.order]
    union = int(np.bitwise_or.reduce(case.nodes["taints"])) if n else 0
    K = len({int(t) for t in p["tolerated_taints"] if int(t) & union != union})
    cls = case.pending.pods["similar_class"]
    n_classes = max(int(cls.max()) + 1, 0) if len(cls) else 0
    n_owners = 0
    if case.class_owner is not None and n_classes:
        n_owners = max(int(np.asarray(case.class_owner)[:n_classes].max()) + 1, 0)
    NW = words(n)
    stat_in = K > 0 and fb_lds(S, NW, K, True, n_classes, n_owners, masked) <= FB_LDS_MAX
    if fb_lds(S, NW, K, stat_in, n_classes, n_owners, masked) > FB_LDS_MAX:
        return window
    return dict(path="bitmap", shapes=S, static_classes=K, static_in_lds=bool(stat_in))


def lds_edge_words(S: int, K: int = 0, n_classes: int = 0, n_owners: int = 0) -> int:
    """NW*: the largest word count for which S shapes (and no static words) fit FB_LDS_MAX."""
    nw = 1
    while fb_lds(S, nw + 1, K, False, n_classes, n_owners, False) <= FB_LDS_MAX:
        nw += 1
    return nw


# ---------------------------------------------------------------------------
# the masks of the TrySchedulePods runs
# ---------------------------------------------------------------------------
MASKS = ("half", "edges", "range")


def hot_node(case: FiltCase) -> int:
    """The node most pods are hinted to (-1: no pod is hinted to a node)."""
    h = case.hints[(case.hints >= 0) & (case.hints < len(case.nodes))]
    return int(np.bincount(h).argmax()) if len(h) else -1


def make_match(name: str, case: FiltCase):
    """tspgen's "half" and "edges" masks and a RANGE whose end lies on a word edge, each
    excluding the case's most-hinted node."""
    import tspgen as T
    n = len(case.nodes)
    ex = hot_node(case)
    if name == "range":
        hi = 64 * (n // 64) if n >= 64 else n
        return (abi.CA_MATCH_RANGE, hi // 3, hi, ex, None)
    kind, lo, hi, _, mask = T.make_match(name, case, case.L0)
    return (kind, lo, hi, ex, mask)


# ---------------------------------------------------------------------------
# both kernels: ring geometry and lastIndex
# ---------------------------------------------------------------------------
RING_SIZES = (1, 37, 63, 64, 65, 127, 128, 129, 255, 256, 257)


def ring_L0s(n: int) -> tuple:
    return tuple(dict.fromkeys((0, min(n - 1, 64 * ((n - 1) // 128) + 21), n - 1, n + 3)))   # 0, mid-word, n - 1, n + 3


def ring_wrap(n: int, L0: int) -> FiltCase:
    """Rooms on nodes n - 1, 0 (two) and 1; four pods: whatever L is, a scan placement on a
    lower node follows one on a higher node."""
    r = Ring(n)
    room: dict = {}
    for x in ((n - 1) % n, 0, 0, 1 % n):
        room[x] = room.get(x, 0) + 1
    for x, k in room.items():
        r.open(x, k)
    for _ in range(4):
        r.pod(A)
    claims = dict(placed=4, wraps=n >= 2)
    if n == 1:
        claims["last_index"] = 0
    return r.build(f"ring/wrap-n{n}-L{L0}", claims, L0)


def ring_end(n: int, L0: int) -> FiltCase:
    """The last placement lands on node n - 1: lastIndex becomes 0."""
    r = Ring(n)
    L = L0 % n
    fits = [n - 1] if (n == 1 or L == n - 1) else [n - 2, n - 1]
    for x in fits:
        r.open(x, 1)
    for _ in fits:
        r.pod(A)
    return r.build(f"ring/end-n{n}-L{L0}", dict(placed=len(fits), last_index=0, nodes={len(fits) - 1: n - 1}), L0)


def ring_overfull(n: int, L0: int) -> FiltCase:
    """More classless pods than fitting nodes: the run stops after one ring pass and each pod
    left over scans the whole ring again."""
    r = Ring(n)
    L = L0 % n
    fits = sorted({(L + 5) % n, (L + n // 2) % n})
    for x in fits:
        r.open(x, 1)
    for _ in range(len(fits) + 2):
        r.pod(A)
    vis = n
    last = max(fits, key=lambda x: (x - L) % n)
    return r.build(f"ring/overfull-n{n}-L{L0}",
                   dict(placed=len(fits), last_index=(last + 1) % n, evals=(last - L) % n + 1 + 2 * vis), L0)


def ring_nothing(n: int, L0: int) -> FiltCase:
    """Nothing fits: lastIndex comes back as it went in (n + 3 included)."""
    r = Ring(n)
    r.pod(A)
    r.pod(A, cls=0)
    r.pod(A, cls=0)
    return r.build(f"ring/nothing-n{n}-L{L0}", dict(placed=0, keeps_last_index=True, evals=2 * n), L0)


def ring_unsched(n: int) -> FiltCase:
    """Unschedulable nodes with room at 0, 63, 64 and n - 1; tolerating and non-tolerating
    pods, hinted onto them and not; one visible node with room behind each word edge."""
    r = Ring(n)
    un = sorted({x for x in (0, 63, 64, n - 1) if 0 <= x < n})
    for x in un:
        r.open(x, 8)
        r.unsched[x] = True
    vis = [x for x in (min(n - 1, 2), 66, n - 2) if 0 <= x < n and x not in un]
    for x in vis:
        r.open(x, 2)
    placed = 0
    for x in un:
        r.pod(A, hint=x, flags=TOL)        # takes the unschedulable node
        r.pod(A, hint=x)                   # does not tolerate: one evaluation, then the scan
        r.pod(A, flags=TOL)                # scans never visit unschedulable nodes
        r.pod(A)
        placed += 1
    del vis, placed
    claims = dict(nodes={4 * i: x for i, x in enumerate(un)}, on_node=(un[-1], 2, 1))
    return r.build(f"ring/unsched-n{n}", claims, min(n - 1, 21))


def ring_pods(P: int) -> FiltCase:
    """P pods of two alternating shapes and every eighth hinted, on a loose ring of 70 nodes."""
    r = Ring(70, loose=4, shape=B)
    for k in range(P):
        r.pod(A if k % 2 else B, hint=(k * 7) % 70 if k % 8 == 3 else -1)
    return r.build(f"ring/P{P}", dict(placed=P), 9)


# ---------------------------------------------------------------------------
# bitmap walk: single-shape runs
# ---------------------------------------------------------------------------
def single_run(m: int, n: int) -> FiltCase:
    """m unhinted pods of one record; rooms for three every 67 nodes from node 36 and L0 = 37,
    so the next fit always lies beyond the 64-position window (no mixed run places a pod) and
    a run's nodes span many words; L0 & 63 != 0: the scan's tail step revisits word w0."""
    r = Ring(n)
    fits = list(range(36, n, 67))
    for x in fits:
        r.open(x, 3)
    for _ in range(m):
        r.pod(A, cls=0)
    want = [fits[(1 + k) % len(fits)] for k in range(min(m, len(fits)))]
    claims = dict(placed=m, nodes={k: x for k, x in enumerate(want)}, shapes=(1, 0))
    if m >= 2:
        claims["route"] = dict(ring_scans=0)
    return r.build(f"single/m{m}-n{n}", claims, 37)


# ---------------------------------------------------------------------------
# bitmap walk: mixed runs
# ---------------------------------------------------------------------------
def mixed_run(f: int, n: int, L0: int) -> FiltCase:
    """f pods of alternating shapes on a loose ring: one mixed run places them on the f
    nodes from L (the window crosses the ring's end where L0 + f > n)."""
    r = Ring(n, loose=3, shape=B)
    for k in range(f):
        r.pod(A if k % 2 else B)
    L = L0 % n
    # a mixed run takes the real nodes among the 64 raw positions from L (ids n .. 64 * NW - 1 are phantom bits)
    steps, left, at = 0, f, L
    while left:
        got = min(left, sum((at + k) % (64 * words(n)) < n for k in range(64)))
        steps, left, at = steps + 1, left - got, (at + got) % n
    claims = dict(placed=f, nodes={k: (L + k) % n for k in range(f)}, last_index=(L + f) % n, evals=f,
                  shapes=(2, 0), route=dict(steps=(steps, f, 0)))
    return r.build(f"mixed/f{f}-n{n}-L{L0}", claims, L0)


def mixed_skip() -> FiltCase:
    """Closed rows inside the window (pods skip them), then a pod whose first fit lies beyond
    the window: the run ends there and the pod scans alone."""
    n = 200
    r = Ring(n)
    for x in (10, 11, 13, 17, 18, 40, 72, 73):
        r.open(x, 1)
    r.open(150, 2)
    for k in range(11):
        r.pod(A if k % 2 else B)
    r.open(10, 1, B), r.open(13, 1, B), r.open(18, 1, B), r.open(72, 1, B), r.open(150, 2, B)
    want = {0: 10, 1: 11, 2: 13, 3: 17, 4: 18, 5: 40, 6: 72, 7: 73, 8: 150, 9: 150, 10: -1}
    return r.build("mixed/skip-and-beyond", dict(placed=10, nodes=want, last_index=151), 8)


def threshold_shapes(dims: tuple) -> list:
    """63 shapes with distinct requests in `dims` (one value in the others) and the all-zero
    shape: 64 live shapes."""
    step = (1, MI, MI)
    return [tuple(A[d] + (s * step[d] if d in dims else 0) for d in range(3)) for s in range(63)] + [ZERO]


def mixed_threshold(f: int, dims: tuple, tag: str) -> FiltCase:
    """A mixed run of f pods, then a PreFilter failure: node k of the run is left with exactly
    the request of shape t_k in `dims` (k even) or one unit less (k odd), t_k growing with k,
    and every fourth run node (k % 4 == 2) with its last pod slot taken.  Then, for every
    k % 4 == 0 in turn, an unhinted pod of shape t_k: the nodes before k are left with less, so
    it lands on node k exactly, by the `<=` of the fit, read on the bitmap walk from the bits
    the run's update left.  Then a pod of shape t_k hinted onto every other node k (one unit
    short, or no slot), and one pod of each shape."""
    shapes = threshold_shapes(dims)
    n, L0 = 100, 70
    r = Ring(n)
    t_of = lambda k: min(k, 62)                                                 # noqa: E731
    for k in range(f):
        s, t = (k * 5) % 63, t_of(k)
        x = (L0 + k) % n
        free = list(BIG)
        for d in dims:
            free[d] = shapes[s][d] + shapes[t][d] - (k & 1)
        if k % 4 == 2:
            free[3] = 1                                  # the placement takes the last slot
        r.raw(x, *free)
        r.pod(shapes[s])
    r.pod(A, flags=PF)
    want = {k: (L0 + k) % n for k in range(f)}
    for k in range(0, f, 4):
        want[r.pod(shapes[t_of(k)])] = (L0 + k) % n
    for k in range(f):
        if k % 4:
            r.pod(shapes[t_of(k)], hint=(L0 + k) % n)
    for s in range(64):
        r.pod(shapes[(s * 7) % 64])
    live = len({(k * 5) % 63 for k in range(f)} | set(range(64)))
    return r.build(f"mixed/threshold-{tag}-f{f}", dict(nodes=want, shapes=(live, 0)), L0)


# ---------------------------------------------------------------------------
# bitmap walk: hints
# ---------------------------------------------------------------------------
def hint_clash() -> FiltCase:
    """Pod 5 of a mixed run is hinted to a node inside the run's window."""
    r = Ring(150, loose=3, shape=B)
    for k in range(12):
        r.pod(A if k % 2 else B, hint=30 if k == 5 else (120 if k == 8 else -1))
    claims = dict(placed=12, nodes={5: 30, 8: 120}, hint_in_window={5: True, 8: False})
    return r.build("hints/clash", claims, 20)


def hint_same_node(m: int, k: int) -> FiltCase:
    """m pods of one batch hinted to node 140, which has room for k; the rest scan."""
    r = Ring(150)
    r.open(140, k, bind=0 if m % 2 else 3)
    r.open(30, 70)
    for _ in range(m):
        r.pod(A, hint=140)
    return r.build(f"hints/same-node-m{m}-k{k}", dict(placed=m, on_node=(140, m, k), hint_in_window={0: False}), 10)


def hint_dirty(fillers: int, tag: str) -> FiltCase:
    """Three scanning pods land on 50, 51, 52; `fillers` positions later pods are hinted to
    51 (room left: lands), 50 (full: scans) and 52 (room left).  fillers = 0: the same batch
    (the dirty lookup); 61: the hinted pods are the first lanes of the next batch (the flushed
    rows); 58: they straddle the batch edge."""
    r = Ring(150)
    r.open(50, 1), r.open(51, 2), r.open(52, 3), r.open(90, 1)
    for _ in range(3):
        r.pod(A)
    r.fill(fillers)
    a = r.pod(A, hint=51)
    b = r.pod(A, hint=50)
    c = r.pod(A, hint=52)
    d = r.pod(A, hint=52)
    e = r.pod(A, hint=52)
    claims = dict(placed=7, nodes={0: 50, 1: 51, 2: 52, a: 51, b: 90, c: 52, d: 52, e: -1}, on_node=(52, 3, 2))
    return r.build(f"hints/written-{tag}", claims, 45)


def hint_values() -> FiltCase:
    """Hints -1, -5, n and n + 70 (no node: the pod is unhinted, no evaluation), a hint that
    fails with the pod joining the following run."""
    n = 130
    r = Ring(n)
    r.open(100, 9)
    for h in (-1, -5, n, n + 70):
        r.pod(A, hint=h, cls=0)
    r.pod(A, hint=3, cls=0)               # closed: one evaluation, then the run of class 0 goes on
    r.pod(A, cls=0)
    r.pod(A, cls=0)
    # the first scan evaluates 7 .. 100 (94 nodes); every later one starts at 101 and reaches node 100
    # at the end of its ring pass (n evaluations); the failing hint is one evaluation
    return r.build("hints/values", dict(placed=7, nodes={k: 100 for k in range(7)}, evals=94 + 6 * n + 1,
                                        last_index=101, hint_in_window={4: False}), 7)


def hint_batch_edge() -> FiltCase:
    """Hinted pods as the last lane of a batch and as the first of the next, one that lands
    and one that fails on each side."""
    r = Ring(150)
    r.open(120, 1), r.open(121, 1), r.open(20, 5)
    r.fill(62)
    r.pod(A, hint=120)                    # lane 62
    r.pod(A, hint=120)                    # lane 63: full by now
    r.pod(A, hint=121)                    # lane 0 of the next batch
    r.pod(A, hint=121)                    # lane 1: full
    return r.build("hints/batch-edge", dict(placed=4, nodes={62: 120, 63: 20, 64: 121, 65: 20}), 10)


# ---------------------------------------------------------------------------
# bitmap walk: shapes
# ---------------------------------------------------------------------------
def many_shapes(live: int, dead: int, path: str) -> FiltCase:
    r = Ring(90, loose=2, shape=(400, 400 * MI, 2 * GI))
    for s in range(live):
        r.pod((100 + s, 100 * MI, GI))
    for s in range(dead):
        r.pod((DEAD[0] + s, 100 * MI, GI), cls=s)
    for s in range(0, live, 3):
        r.pod((100 + s, 100 * MI, GI))
    claims = dict(placed=live + len(range(0, live, 3)), shapes=(live, dead))
    paths = ("bitmap", "window") if path == "bitmap" else ("window",)
    return r.build(f"shapes/live{live}-dead{dead}", claims, 5, paths=paths)


def collected_shapes() -> FiltCase:
    """1 030 distinct shapes, all but six of them dead: past FB_COLLECT_SHAPES the call takes
    the window kernel before the dead ones are merged."""
    r = Ring(10)
    r.open(4, 6)
    for s in range(1030):
        r.pod(A if s % 200 == 7 else (DEAD[0] + s, 100 * MI, GI), cls=s % 200 if s % 200 != 7 else -1)
    return r.build("shapes/collected-1030", dict(placed=6), 2, paths=("window",))


def all_dead(slots: bool) -> FiltCase:
    """Every shape dead: no node has the request, or (slots) no node has a free pod slot."""
    r = Ring(70)
    if slots:
        for i in range(70):
            r.close(i, 3)
    shapes = [A, B, ZERO] if slots else [DEAD, (DEAD[0] + 1, MI, MI)]
    for k in range(9):
        r.pod(shapes[k % len(shapes)], cls=k % 3, hint=k if k % 4 == 0 else -1)
    return r.build("shapes/no-free-slot" if slots else "shapes/all-dead",
                   dict(placed=0, keeps_last_index=True, shapes=(0, len(shapes))), 66)


# ---------------------------------------------------------------------------
# bitmap walk: the similar-pods cache
# ---------------------------------------------------------------------------
def owner_classes(k: int) -> FiltCase:
    """A controller with k failing classes (two pods each) between a controller with one and
    classless pods: past 10 the controller overflows and its pods scan the ring each."""
    n = 70
    r = Ring(n)
    r.open(33, 2)
    owner = [0] * k + [1]
    for c in range(k):
        r.pod(DEAD, cls=c)
        r.pod(DEAD, cls=c)
    r.pod(A, cls=k), r.pod(A, cls=k), r.pod(A, cls=k), r.pod(A, cls=k)
    marked = min(k, FO_MAX_PER_OWNER)
    scans = marked + 2 * (k - marked)                 # a marked class fails once, an unmarked one every time
    claims = dict(placed=2, overflowing=1 if k > FO_MAX_PER_OWNER else 0,
                  evals=scans * n + (33 - 3 + 1) + 2 * n)      # 3 .. 33, a whole pass back to 33, a failing pass
    return r.build(f"similar/owner-{k}-classes", claims, 3, class_owner=np.array(owner, np.int32))


def similar_rescans() -> FiltCase:
    """DaemonSet pods of a class and classless pods fail again and again (each scans the
    ring); a class marked in the first batch is met again in the second; a PreFilter failure
    inside a run of its class and as the last pod."""
    n = 70
    r = Ring(n)
    r.open(40, 3)
    for _ in range(3):
        r.pod(DEAD, cls=0, flags=DS)
    for _ in range(3):
        r.pod(DEAD)
    r.pod(DEAD, cls=1)                                 # marks class 1
    r.pod(A, cls=2), r.pod(A, cls=2, flags=PF), r.pod(A, cls=2)      # the PreFilter failure marks class 2
    r.fill(60)
    r.pod(DEAD, cls=1), r.pod(DEAD, cls=1)            # second batch: skipped
    r.pod(A, cls=3)
    r.pod(A, cls=3, flags=PF)
    claims = dict(placed=2, evals=7 * n + (40 - 6 + 1) + n, nodes={7: 40, 9: -1, 72: 40})
    return r.build("similar/rescans-marks-prefilter", claims, 6)


# ---------------------------------------------------------------------------
# bitmap walk: static classes and LDS
# ---------------------------------------------------------------------------
def static_small() -> FiltCase:
    """Taints on half the ring: three static classes whose words fit LDS."""
    n = 100
    r = Ring(n, loose=2)
    for i in range(n):
        r.taints[i] = (1 if i % 2 else 0) | (2 if i % 5 == 0 else 0)
    for k in range(24):
        r.pod(A if k % 3 else B, tol=(0, 1, 2, 3)[k % 4], hint=(k * 9) % n if k % 6 == 1 else -1)
    return r.build("static/in-lds", dict(placed=24, lds=dict(static_classes=3, static_in_lds=True)), 61)


def static_spill() -> FiltCase:
    """64 static classes on a ring sized by fb_lds so that their words do not fit LDS with
    the rest but the rest fits alone: the walk reads them from memory."""
    K = 64
    nw = 1
    while fb_lds(2, nw, K, True, 0, 0, False) <= FB_LDS_MAX:
        nw += 1
    n = 64 * nw - 11
    r = Ring(n)
    for i in range(n):
        r.taints[i] = np.uint64((i * 37) % 128)
    for x in range(5, n, 997):
        r.open(x, 2, B)
        r.taints[x] = np.uint64((x // 997) % 128)
    for k in range(K):
        r.pod(A if k % 2 else B, tol=k)                # tolerates the taint sets within its bits
        r.pod(A if k % 2 else B, tol=k, hint=5 + 997 * (k % 19) if k % 2 else -1)
    return r.build("static/spilled", dict(lds=dict(static_classes=K, static_in_lds=False, spill=(2, nw, K))), 64 * 9 + 5)


def lds_pair(over: bool) -> FiltCase:
    """64 live shapes on 64 * NW* nodes (the bitmap walk) and on one node more (the window
    kernel): NW* is the largest word count whose bitmaps fit FB_LDS_MAX."""
    nw = lds_edge_words(64)
    n = 64 * nw + (1 if over else 0)
    r = Ring(n)
    for x in (3, 64 * (nw - 1) + 63, n - 1, 4000):
        r.open(x, 60, (200, 200 * MI, 2 * GI))
    for s in range(64):
        r.pod((100 + s, 100 * MI, GI))
        r.pod((100 + s, 100 * MI, GI), hint=n - 1 if s % 8 == 0 else -1)
    claims = dict(placed=128, shapes=(64, 0), lds=dict(pair=(64, nw), over=over))
    return r.build(f"static/lds-pair-{'over' if over else 'fits'}", claims, 64 * (nw - 1) + 50,
                   paths=("window",) if over else ("bitmap", "window"))


def route_by_content(kind: str) -> FiltCase:
    """mixed/f25 with one more pod that only the window kernel handles."""
    r = Ring(100, loose=3, shape=B)
    for k in range(25):
        r.pod(A if k % 2 else B)
    if kind == "port":
        r.pod(A, port=5)
    elif kind == "scalar":
        r.scalar[:] = 4
        r.pod(A, scalar=1)
    else:
        r.pod(A, names=[7, 99])
    want = {k: (70 + k) % 100 for k in range(25)}
    want[25] = 99 if kind == "names" else 95          # from L = 95: the first listed node is 99
    return r.build(f"content/{kind}", dict(placed=26, nodes=want), 70, paths=("window",))


# ---------------------------------------------------------------------------
# window sequencer
# ---------------------------------------------------------------------------
def window_ring(n: int, off: int, tag: str, L0: int = 5) -> FiltCase:
    """The only node with room lies `off` positions from L0: inside the 512-row window, or in
    the block-wide ring scan behind it (8 192 positions a pass).  Three pods take it in turn;
    after each the window is loaded again at the same place."""
    r = Ring(n)
    x = (L0 + off) % n
    r.open(x, 3)
    for _ in range(3):
        r.pod(A)
    r.pod(A)
    resident = n <= SQ_WIN
    # the first scan stops at x; every later one starts behind x and meets it last
    claims = dict(placed=3, nodes={0: x, 1: x, 2: x, 3: -1}, last_index=(x + 1) % n, evals=off + 1 + 3 * n,
                  route=dict(window="resident" if resident else "moves"))
    return r.build(f"window/n{n}-{tag}", claims, L0)


def window_cursor() -> FiltCase:
    """A placement on the window's last row: the cursor runs off the window and the next pod
    loads a new one (no ring scan)."""
    n, L0 = 600, 20
    r = Ring(n)
    r.open(L0 + 511, 1), r.open(L0 + 530, 1)
    r.pod(A), r.pod(A)
    return r.build("window/cursor-off", dict(placed=2, nodes={0: L0 + 511, 1: L0 + 530}, last_index=L0 + 531,
                                            route=dict(window="cursor")), L0)


def window_ring_reload() -> FiltCase:
    """The scan leaves the window; the fit lies behind it and the window loaded at the new
    lastIndex wraps the ring's end."""
    n, L0 = 600, 500
    r = Ring(n)
    r.open(20, 1), r.open(450, 1), r.open(470, 1)          # window: 500 .. 599, 0 .. 411
    for _ in range(3):
        r.pod(A)
    return r.build("window/ring-reload-wraps", dict(placed=3, nodes={0: 20, 1: 450, 2: 470}, last_index=471, wraps=True,
                                                   route=dict(window="moves")), L0)


def window_staged(kind: str) -> FiltCase:
    n = 600
    r = Ring(n)
    if kind == "same-node":            # five slots hinted to one node outside the window, room for three
        r.open(550, 3), r.open(10, 9)
        for _ in range(5):
            r.pod(A, hint=550)
        claims = dict(placed=5, on_node=(550, 5, 3), nodes={3: 10, 4: 10})
    elif kind == "ring-onto-hinted":   # a ring-scan placement on the node later slots are hinted to
        r.open(560, 2), r.open(570, 1)
        r.pod(A)
        r.pod(A, hint=560)
        r.pod(A, hint=560)
        claims = dict(placed=3, nodes={0: 560, 1: 560, 2: 570}, on_node=(560, 2, 1))
    else:                              # the hinted node enters the window while its staged copy is dirty
        r.open(550, 2), r.open(540, 1), r.open(580, 1)
        r.pod(A, hint=550)
        r.pod(A)
        r.pod(A, hint=550)
        r.pod(A, hint=550)
        claims = dict(placed=4, nodes={0: 550, 1: 540, 2: 550, 3: 580}, on_node=(550, 3, 2))
    claims["route"] = dict(window="moves")
    return r.build(f"window/staged-{kind}", claims, 0)


def window_slot_edge(kind: str, at: int) -> FiltCase:
    """A mark, a ring scan or (with the case's own break) a failure on slot 63 of the first
    phase or slot 0 of the second."""
    n = 300 if kind == "mark" else 600         # the whole ring resident: a failing scan is a mark step
    x = n - 20
    r = Ring(n)
    r.open(x, 2, bind=0)
    if kind == "mark":
        r.fill(at)
        r.pod(DEAD, cls=0), r.pod(DEAD, cls=0), r.pod(A)
        claims = dict(placed=1, nodes={at: -1, at + 1: -1, at + 2: x}, evals=n + x + 1, route=dict(window="resident"))
    elif kind == "ring":
        r.fill(at)
        r.pod(A), r.pod(A), r.pod(A)
        claims = dict(placed=2, nodes={at: x, at + 1: x, at + 2: -1}, route=dict(window="moves"))
    else:                                      # (pods that land: a failing filler would be the break)
        r.open(100, 70)
        for _ in range(at):
            r.pod(A)
        r.pod(DEAD), r.pod(A)
        claims = dict(placed=at, tried=at + 1)
        return r.build(f"window/slot{at}-break", claims, 0, match=(abi.CA_MATCH_ALL, 0, 0, -1, None), brk=True)
    return r.build(f"window/slot{at}-{kind}", claims, 0)


def window_ports() -> FiltCase:
    """Pods of one host port by scan and by hint in one phase; a resident pod holds the port
    on the first node with room."""
    n = 80
    r = Ring(n)
    for x in (20, 21, 22, 60):
        r.open(x, 5)
    r.res_ports[20] = 5
    a = r.pod(A, port=5)                   # 20 holds the port: lands on 21
    b = r.pod(A, port=5, hint=21)          # conflicts with a: scans to 22
    c = r.pod(A, port=5, hint=60)
    d = r.pod(A, port=6, hint=21)          # another port: lands
    e = r.pod(A, port=5)                   # 20, 21, 22 and 60 hold it: nothing left
    return r.build("window/ports", dict(placed=4, nodes={a: 21, b: 22, c: 60, d: 21, e: -1}), 15, paths=("window",))


def window_scalar() -> FiltCase:
    """A scalar request that fits exactly once on the only node that has the resource."""
    n = 80
    r = Ring(n, loose=3)
    r.scalar[33] = 2
    a = r.pod(A, scalar=2)
    b = r.pod(A, scalar=2, hint=33)
    c = r.pod(A, scalar=1)
    return r.build("window/scalar", dict(placed=1, nodes={a: 33, b: -1, c: -1}), 30, paths=("window",))


# ---------------------------------------------------------------------------
# TrySchedulePods: planted breaks (the case's own match, break on failure)
# ---------------------------------------------------------------------------
def tsp_break(kind: str) -> FiltCase:
    n = 130
    r = Ring(n, loose=2)
    mask = np.zeros(n, np.uint8)
    mask[0:64] = 1                               # a RANGE-like mask that ends on the word edge
    match = (abi.CA_MATCH_MASK, 0, 0, -1, mask)
    if kind == "first":
        r.pod(DEAD), r.pod(A), r.pod(B)
        tried, placed = 1, 0
    elif kind == "lane63":
        for k in range(63):
            r.pod(A if k % 2 else B)
        r.pod(DEAD), r.pod(A)
        tried, placed = 64, 63
    elif kind == "hinted-outside-mask":          # the hint passes (hint_ok) but the node is not acceptable
        for i in range(64):
            r.close(i)
        r.pod(A, hint=100), r.pod(A)
        tried, placed = 1, 0
    else:                                        # a pod of a class: the break comes before any mark
        r.pod(A, cls=0), r.pod(DEAD, cls=1), r.pod(DEAD, cls=1), r.pod(A, cls=0)
        tried, placed = 2, 1
    return r.build(f"tsp/break-{kind}", dict(tried=tried, placed=placed), 3, match=match, brk=True)


# ---------------------------------------------------------------------------
def all_cases() -> dict:
    cases: list = []
    for n in RING_SIZES:
        for L0 in ring_L0s(n):
            cases += [ring_wrap(n, L0), ring_end(n, L0), ring_overfull(n, L0), ring_nothing(n, L0)]
        cases.append(ring_unsched(n))
    r = Ring(70, loose=2)
    e = r.build("ring/P0", dict(placed=0, keeps_last_index=True, evals=0), 75)
    cases.append(e)
    cases += [ring_pods(P) for P in (1, 63, 64, 65, 128, 129)]
    cases += [single_run(m, n) for n in (4096, 4160) for m in (1, 2, 63, 64, 65, 130)]
    cases += [mixed_run(f, 100, 70) for f in (2, 23, 24, 25, 30, 64)]              # NW = 2, across the ring's end
    cases += [mixed_run(f, 37, 30) for f in (2, 23, 24, 25)] + [mixed_run(64, 64, 61)]      # NW = 1: the rotate
    cases += [mixed_run(25, 128, 100), mixed_skip()]
    for dims, tag in (((0,), "cpu"), ((1,), "mem"), ((2,), "eph"), ((0, 1), "cpu-mem"), ((0, 1, 2), "all")):
        cases += [mixed_threshold(f, dims, tag) for f in (23, 24, 25, 64)]
    cases += [hint_clash(), hint_same_node(2, 1), hint_same_node(3, 2), hint_same_node(64, 40), hint_same_node(64, 64),
              hint_dirty(0, "same-batch"), hint_dirty(61, "previous-batch"), hint_dirty(58, "across-batches"),
              hint_values(), hint_batch_edge()]
    cases += [many_shapes(64, 0, "bitmap"), many_shapes(64, 3, "bitmap"), many_shapes(65, 0, "window"),
              collected_shapes(), all_dead(False), all_dead(True)]
    cases += [owner_classes(k) for k in (10, 11, 12)] + [similar_rescans()]
    cases += [static_small(), static_spill(), lds_pair(False), lds_pair(True)]
    cases += [route_by_content(k) for k in ("port", "scalar", "names")]
    cases += [window_ring(511, 510, "last-row"), window_ring(512, 511, "last-row"), window_ring(513, 512, "first-outside"),
              window_ring(577, 576, "last-node"), window_ring(8704, 8703, "end-of-pass"),
              window_ring(8705, 8704, "second-pass"), window_ring(8705, 512 + 15 * 512 + 3, "last-stride"),
              window_ring(8705, 512 + SQ_PASS - 1, "last-of-pass"),
              window_cursor(), window_ring_reload()]
    cases += [window_staged(k) for k in ("same-node", "ring-onto-hinted", "enters-window-dirty")]
    cases += [window_slot_edge(k, at) for k in ("mark", "ring", "break") for at in (63, 64)]
    cases += [window_ports(), window_scalar()]
    cases += [tsp_break(k) for k in ("first", "lane63", "hinted-outside-mask", "class-pod")]
    out = {c.name: c for c in cases}
    assert len(out) == len(cases)
    return out


FAMILIES = ("ring", "single", "mixed", "hints", "shapes", "similar", "static", "content", "window", "tsp")
