"""Generators of the node-reorder tests (ca_mirror_reorder_nodes, ClusterSnapshot.SetNodeOrder):
the permutations, the sizes, clusters that hold every kind of node the call must carry along,
three planted clusters whose nodes differ in one device column only, the model's `reorder`,
and the seeded sequence of tests/snapmodel.py extended by `reorder` and `set_hints` ops.

An order is what the C ABI takes: the node now at position order[k] moves to position k.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np

import snapmodel as S
from autoscaler_amd import abi

# the smallest sizes that cross an edge of the code: a wave and the 64-node block sums, a
# workgroup, the first row-buffer size (mirror.hip sync_nodes: 1024 rows)
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
PERM_KINDS = ("identity", "swap-ends", "reverse", "rot1", "rot63", "rot64", "rot65", "rand0", "rand1", "two")


def _rot(n: int, r: int) -> np.ndarray:
    return ((np.arange(n) + r) % n).astype(np.int32)


def permutation(kind: str, n: int) -> list:
    """The orders of one case, applied in a row (one, or two for "two").  The seeded random
    ones are redrawn until position 0 moves (n > 1), so a probe that scans from lastIndex 0
    sees every one of them."""
    ident = np.arange(n, dtype=np.int32)
    if kind == "identity":
        return [ident]
    if kind == "swap-ends":
        o = ident.copy()
        o[0], o[-1] = ident[-1], ident[0]
        return [o]
    if kind == "reverse":
        return [ident[::-1].copy()]
    if kind.startswith("rot"):
        return [_rot(n, int(kind[3:]))]
    if kind.startswith("rand"):
        rng = random.Random(f"reordergen/{kind}/{n}")
        while True:
            o = list(range(n))
            rng.shuffle(o)
            if n == 1 or o[0] != 0:
                return [np.array(o, np.int32)]
    if kind == "two":
        return [ident[::-1].copy(), _rot(n, 1)]
    raise ValueError(kind)


def compose(orders: list) -> np.ndarray:
    """The one order that equals applying `orders` in a row."""
    net = np.arange(len(orders[0]), dtype=np.int32)
    for o in orders:
        net = net[np.asarray(o)]
    return net


def inverse(order) -> np.ndarray:
    inv = np.zeros(len(order), np.int32)
    inv[np.asarray(order)] = np.arange(len(order), dtype=np.int32)
    return inv


def is_identity(order) -> bool:
    return bool((np.asarray(order) == np.arange(len(order))).all())


# ---------------------------------------------------------------------------
# the model's reorder
# ---------------------------------------------------------------------------
class ReorderModel(S.SnapModel):
    def reorder(self, order) -> None:
        assert not self.stack, "reorder inside a fork"
        assert sorted(int(v) for v in order) == list(range(len(self.nodes)))
        self.nodes = [self.nodes[int(x)] for x in order]     # hints are kept by name: nothing to do


# ---------------------------------------------------------------------------
# clusters
# ---------------------------------------------------------------------------
@dataclass
class Case:
    """n nodes after the load.  With `gone` set, n + 1 records are loaded and position `gone`
    is removed at depth 0 once the hints are set (a code < -1 then sits in the resident hints);
    `victim` is RemovePod'ed from a node with three pods (swap-with-last reshuffles its list)."""
    n: int
    nodes: np.ndarray
    table: abi.PodTable
    idx: list = field(default_factory=list)      # the pods in id order: record ...
    pos: list = field(default_factory=list)      # ... and position among the loaded records
    gone: int | None = None
    victim: int | None = None
    hints: list | None = None                    # per pod id: a position among the loaded records, or -1
    empty: int | None = None                     # a node (position after the load) without pods
    shuffled: int | None = None                  # the node (position after the load) of `victim`

    def survivors(self) -> list:
        return [x for x in range(len(self.nodes)) if x != self.gone]


def cluster(n: int, seed: int = 0) -> Case:
    rng = random.Random(f"reordergen/cluster/{n}/{seed}")
    table = S.gen_pod_table(rng, blockers=False)
    nodes = S.gen_nodes(rng, n + 1, 0)
    gone = rng.randrange(n + 1)
    c = Case(n, nodes, table, gone=gone)
    surv = c.survivors()
    empty = surv[0] if n >= 2 else None
    shuffled = surv[-1]
    for x in range(n + 1):
        k = 0 if x == empty else 3 if x == shuffled else rng.randrange(6)
        for _ in range(k):
            c.idx.append(rng.randrange(len(table)))
            c.pos.append(x)
    both = list(zip(c.idx, c.pos))
    rng.shuffle(both)                            # ids do not follow positions
    c.idx, c.pos = [b[0] for b in both], [b[1] for b in both]
    c.victim = c.pos.index(shuffled)             # the first pod of its list: the last takes its slot
    c.hints = [rng.choice((-1, gone, rng.randrange(n + 1), rng.randrange(n + 1))) for _ in c.idx]
    if c.idx:
        c.hints[0] = gone
    c.empty = None if empty is None else surv.index(empty)
    c.shuffled = surv.index(shuffled)
    return c


def load(backend, c: Case, model: ReorderModel | None = None, hints: bool = True) -> None:
    """The case into a backend (and the model), in the recorded order."""
    backend.clear()
    backend.add_nodes(c.nodes)
    if model is not None:
        model.add_nodes(c.nodes)
    if c.idx:
        ids = backend.add_pods(c.table, c.idx, c.pos).tolist()
        assert ids == list(range(len(c.idx)))
        if model is not None:
            assert model.add_pods(c.idx, c.pos) == ids
    if c.hints is not None and c.idx:
        if hints and hasattr(backend, "set_hints"):
            backend.set_hints(c.hints)
        if model is not None:
            model.set_hints(c.hints)
    if c.victim is not None:
        backend.remove_pod(c.victim)
        if model is not None:
            model.remove_pod(c.victim)
    if c.gone is not None:
        backend.remove_node(c.gone)
        if model is not None:
            model.remove_node(c.gone)


def load_fresh(backend, c: Case, order, model: ReorderModel | None = None) -> None:
    """The state `load` + reorder(order) leaves, built from scratch: the surviving nodes in the
    new order (the removed one after them), every pod in id order on its node, then the same
    RemovePod and RemoveNode.  Pod ids and every NodeInfo.Pods order agree with the reordered
    backend's."""
    surv = c.survivors()
    new_nodes = c.nodes[[surv[int(x)] for x in order] + ([c.gone] if c.gone is not None else [])]
    at = {surv[int(x)]: k for k, x in enumerate(order)}
    if c.gone is not None:
        at[c.gone] = c.n
    fresh = Case(c.n, new_nodes, c.table, list(c.idx), [at[x] for x in c.pos],
                 None if c.gone is None else c.n, c.victim,
                 None if c.hints is None else [(-1 if h < 0 else at[h]) for h in c.hints])
    load(backend, fresh, model, hints=False)


def planted(column: str, n: int = 65) -> tuple:
    """(case, probe table, field): n nodes that differ in `field` (and their name) only, which
    lands in one device column: free cpu in NodeHot, one extended resource in NodeExt, one
    taint and one label pair in NodeStatic.  Each probe fits a set of nodes that only that
    field decides, so a gather that leaves the column in the old order answers for the node
    that used to be at a position.  (Every node carries an extended resource and a taint, so
    the flags in NodeHot are equal too.)"""
    nodes = abi.empty_nodes(n)
    nodes[:] = S.node_record(0, 4000, 16 * S.GI, 10 * S.GI, 110, 4, taints=0b11)[0]
    nodes["name_id"] = np.arange(n)
    if column == "hot":
        fld = "alloc_milli_cpu"
        nodes[fld] = 1000 + 10 * np.arange(n)
        recs = [S.pod_record(cpu=1000 + 10 * j, **S.RES_TOL) for j in (0, n // 2, n - 2, n - 1)]
    elif column == "ext":
        fld = "alloc_scalar"
        nodes[fld][:, S.SCALAR_COL] = 1 + np.arange(n)
        recs = [S.pod_record(scalar=1 + j, flags=abi.CA_POD_HAS_SCALAR_KEYS | abi.CA_POD_TOLERATES_UNSCHED,
                             tolerated=S.U64) for j in (0, n // 2, n - 2, n - 1)]
    elif column == "static":
        fld = ("taints", "label_pairs")
        nodes["taints"][n // 3] = np.uint64(0b01)
        nodes["label_pairs"][(2 * n) // 3, 0] = np.uint64(0b001)
        recs = [S.pod_record(tolerated=0b01), S.pod_record(selector=0b001, **S.RES_TOL)]
    else:
        raise ValueError(column)
    return Case(n, nodes, abi.PodTable(np.concatenate(recs))), abi.PodTable(np.concatenate(recs)), fld


def last_indexes(n: int) -> list:
    return sorted({0, 1 % n, n - 1})


def probe_answers(backend, table: abi.PodTable, n: int, match=None) -> list:
    """fits_any_node of every probe from lastIndex 0, 1 and n - 1: (node, lastIndex out,
    PreFilter failure, evaluations)."""
    return [backend.fits_any_node(table, p, match, L) for p in range(len(table)) for L in last_indexes(n)]


def sample_probes(model: S.SnapModel, k: int = 10) -> abi.PodTable:
    """At most about k of the model's bracketing probes, evenly spaced, and one that fits every
    node with a free slot."""
    pr = S.probes(model)
    sel = sorted(set(np.linspace(0, len(pr.table) - 1, k).astype(int).tolist()))
    return abi.PodTable(np.concatenate([pr.table.pods[sel], S.pod_record(**S.RES_TOL)]))


# ---------------------------------------------------------------------------
# the seeded sequence with reorders and hints
# ---------------------------------------------------------------------------
AFTER = ("revert", "commit", "remove_node_depth0")


class ReorderSequence(S.Sequence):
    """tests/snapmodel.py's sequence with two more ops: `set_hints` (random hints for every
    pod id) and `reorder`, chosen at depth 0 only — more often while a revert, a commit or a
    depth-0 RemoveNode has happened since the last one.  cov counts the reorders that follow
    each of those, and those with hints set."""

    def __init__(self, seed: int, n_nodes: int = 12, max_depth: int = 3):
        super().__init__(seed, n_nodes, max_depth)
        self.model = ReorderModel(self.table)
        self.since: set = set()
        self.cov.update(reorder=0, set_hints=0, reorder_with_hints=0, reorder_identity=0)
        self.cov.update({f"reorder_after_{k}": 0 for k in AFTER})

    def _order(self) -> np.ndarray:
        n, rng = self.model.node_count(), self.rng
        kind = rng.choice(("shuffle", "shuffle", "rot1", "swap-ends", "reverse", "identity"))
        if kind == "shuffle":
            o = list(range(n))
            rng.shuffle(o)
            return np.array(o, np.int32)
        return permutation(kind, n)[0]

    def _choose(self) -> str:
        """The base choice, with the ops a reorder has to follow drawn more often while none
        of their kind waits for one."""
        op = super()._choose()
        m, r = self.model, self.rng.random()
        if op == "remove_blocker":
            return op
        if m.depth and "commit" not in self.since and r < 0.2:
            return "commit"
        if m.depth and "revert" not in self.since and 0.2 <= r < 0.3:
            return "revert"
        if not m.depth and "remove_node_depth0" not in self.since and m.node_count() > self.min_nodes and r < 0.1:
            return "remove_node"
        return op

    def next(self, backends) -> str:
        m, rng = self.model, self.rng
        r = rng.random()
        if m.depth == 0 and r < (0.5 if self.since else 0.08):
            self.step += 1
            self.op = "reorder"
            order = self._order()
            self.cov["reorder"] += 1
            self.cov["reorder_identity"] += int(is_identity(order))
            self.cov["reorder_with_hints"] += int(bool(m.hints))
            for k in self.since:
                self.cov[f"reorder_after_{k}"] += 1
            self.since.clear()
            m.reorder(order)
            for b in backends:
                b.reorder_nodes(order)
            return "reorder"
        # (hints are set at depth 0: one to a node added inside a fork would outlive the node's
        # Revert as a bare position, which no reorder could follow)
        if m.depth == 0 and len(m.pod_rec) and 0.85 < r < 0.95:
            self.step += 1
            self.op = "set_hints"
            self.cov["set_hints"] += 1
            hints = [rng.choice((-1, rng.randrange(m.node_count()))) for _ in m.pod_rec]
            m.set_hints(hints)
            for b in backends:
                b.set_hints(hints)
            return "set_hints"
        depth = m.depth
        op = super().next(backends)
        if op in ("revert", "commit"):
            self.since.add(op)
        elif op == "remove_node" and depth == 0:
            self.since.add("remove_node_depth0")
        return op
