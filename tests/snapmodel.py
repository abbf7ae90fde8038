"""A copy-on-fork model of the snapshot, seeded op sequences, bracketing probes, and the
whole-state checker that compares a backend (the GPU mirror or the CPU oracle) with it.

The mirror and the oracle both implement Fork / Revert / Commit with an undo journal of the
same design; the reference's semantics are simpler (a fork is a copy, a revert throws the copy
away), and `SnapModel` does exactly that.  Nothing here stores a free value: they are summed
on demand, as Python ints, over the pods a node holds.

The fit rule (`expected_fits`) is the reference's, in the kernel's order: NodeUnschedulable,
TaintToleration, nodeSelector, NodePorts, the pod-slot check, then fitsRequest, which returns
early only when cpu, memory and ephemeral-storage are all 0 and CA_POD_HAS_SCALAR_KEYS is
unset; otherwise the three are compared as req > free even at req == 0 (a memory-only pod
fails on a node whose free cpu is negative), and scalar columns are skipped at req == 0.
Ports are a set: RemovePod clears the pod's bits even if another pod on the node holds them.
"""
from __future__ import annotations

import ctypes as C
import random

import numpy as np

from autoscaler_amd import abi
from quantgen import CPU_REQ, EPH_REQ, MEM_REQ

GI = 1 << 30
U64 = (1 << 64) - 1
SCALAR_COL = 0                                   # the one scalar column the generator uses
PORT_BITS = (0, 3, 17, 63, 64 + 5)               # both port words, the top bit of word 0
TAINT_SETS = (0, 0b01, 0b10, 0b11)               # node taints / pod toleration sets
LABEL_SETS = (0, 0b001, 0b010, 0b101, 0b110)     # node label pairs (word 0) / pod selectors
SELECTORS = (0b001, 0b100, 0b101)
# the seed sets of the sequence tests: the CPU test (tests/test_snapshot_model.py) and the GPU
# test (tests/test_gpu_snapshot_state.py) share them
LIST_SEEDS, LIST_STEPS = range(30), 400          # lists only
PROBE_SEEDS, PROBE_STEPS = range(12), 300        # lists and the probe matrix
RES_TOL = dict(tolerated=U64, flags=abi.CA_POD_TOLERATES_UNSCHED)   # the resource probes see every row


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
class _Node:
    __slots__ = ("rec", "pods", "ports")

    def __init__(self, rec):
        self.rec = rec                           # one NODE_DTYPE record (never written)
        self.pods: list = []
        self.ports = [0] * abi.CA_PORT_WORDS

    def clone(self):
        n = _Node(self.rec)
        n.pods = list(self.pods)
        n.ports = list(self.ports)
        return n


class SnapModel:
    def __init__(self, table: abi.PodTable):
        self.table = table
        self._req = {f: table.pods[f].tolist() for f in ("req_milli_cpu", "req_memory", "req_ephemeral", "req_scalar",
                                                         "port_use", "flags")}
        self.nodes: list = []
        self.pod_rec: list = []                  # pod id -> record index in `table`; ids are never reused
        self.stack: list = []                    # the forks' copies of `nodes`
        self.hints: dict = {}                    # pod id -> name_id of the hinted node

    # -- ops ------------------------------------------------------------------
    def add_nodes(self, recs) -> int:
        first = len(self.nodes)
        for r in recs:
            self.nodes.append(_Node(r.copy()))
        return first

    def add_pods(self, idx, pos) -> list:
        ids = []
        for i, x in zip(idx, pos):
            pid = len(self.pod_rec)
            self.pod_rec.append(int(i))
            nd = self.nodes[x]
            nd.pods.append(pid)
            use = self._req["port_use"][int(i)]
            for w in range(abi.CA_PORT_WORDS):
                nd.ports[w] |= use[w]
            ids.append(pid)
        return ids

    def remove_pod(self, pid: int) -> None:
        x = self.pod_node(pid)
        assert x >= 0
        nd = self.nodes[x]
        s = nd.pods.index(pid)
        nd.pods[s] = nd.pods[-1]                 # swap with the last
        nd.pods.pop()
        use = self._req["port_use"][self.pod_rec[pid]]
        for w in range(abi.CA_PORT_WORDS):
            nd.ports[w] &= ~use[w] & U64

    def remove_node(self, pos: int) -> None:
        del self.nodes[pos]

    def fork(self) -> None:
        self.stack.append([n.clone() for n in self.nodes])

    def revert(self) -> None:
        self.nodes = self.stack.pop()

    def commit(self) -> None:
        self.stack.pop()

    # -- views ----------------------------------------------------------------
    @property
    def depth(self) -> int:
        return len(self.stack)

    def node_count(self) -> int:
        return len(self.nodes)

    def pod_nodes(self) -> list:
        where = [-1] * len(self.pod_rec)
        for x, nd in enumerate(self.nodes):
            for pid in nd.pods:
                where[pid] = x
        return where

    def pod_node(self, pid: int) -> int:
        for x, nd in enumerate(self.nodes):
            if pid in nd.pods:
                return x
        return -1

    def placed(self) -> list:
        return [pid for nd in self.nodes for pid in nd.pods]

    def scope_blockers(self) -> int:
        f = self._req["flags"]
        return sum(1 for pid in self.placed() if f[self.pod_rec[pid]] & abi.CA_POD_REQUIRED_ANTI_AFFINITY)

    def free(self, x: int) -> dict:
        """cpu, mem, eph, slots, scalar[8] of node x: alloc minus the sums over its pods."""
        nd, p = self.nodes[x], self._req
        rec = [self.pod_rec[pid] for pid in nd.pods]
        tot = lambda f: sum(p[f][i] for i in rec)                              # noqa: E731
        return {"cpu": int(nd.rec["alloc_milli_cpu"]) - tot("req_milli_cpu"),
                "mem": int(nd.rec["alloc_memory"]) - tot("req_memory"),
                "eph": int(nd.rec["alloc_ephemeral"]) - tot("req_ephemeral"),
                "slots": int(nd.rec["alloc_pods"]) - len(nd.pods),
                "scalar": [int(nd.rec["alloc_scalar"][k]) - sum(p["req_scalar"][i][k] for i in rec)
                           for k in range(abi.CA_MAX_SCALAR)]}

    # -- hints, by node name ----------------------------------------------------
    def set_hints(self, hints) -> None:
        """hints[pid] = node position now (or -1): remembered as the node's name_id."""
        self.hints = {pid: int(self.nodes[h].rec["name_id"]) for pid, h in enumerate(hints) if h >= 0}

    def expected_hints(self) -> list:
        """Per pod id: the hinted node's position now, -1 for no hint, None for "some value < 0"
        (the hinted node is not in the snapshot)."""
        pos = {int(nd.rec["name_id"]): x for x, nd in enumerate(self.nodes)}
        return [(-1 if pid not in self.hints else pos.get(self.hints[pid])) for pid in range(len(self.pod_rec))]


# ---------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------
def pod_record(cpu=0, mem=0, eph=0, scalar=0, port=None, tolerated=0, selector=0, flags=0) -> np.ndarray:
    p = abi.empty_pods(1)
    p["req_milli_cpu"], p["req_memory"], p["req_ephemeral"] = cpu, mem, eph
    p["score_milli_cpu"], p["score_memory"] = cpu, mem
    if scalar is not None and scalar != 0:
        p["req_scalar"][0][SCALAR_COL] = scalar
    if port is not None:
        p["port_use"][0][port >> 6] = p["port_conflict"][0][port >> 6] = np.uint64(1 << (port & 63))
    p["tolerated_taints"] = np.uint64(tolerated)
    if selector:
        p["node_selector"][0][0] = np.uint64(selector)
        flags |= abi.CA_POD_AFFINITY_FILTER
    p["flags"] = flags
    return p


def node_record(name_id, cpu, mem, eph=0, pods=110, scalar=0, taints=0, labels=0, unsched=False) -> np.ndarray:
    n = abi.empty_nodes(1)
    n["alloc_milli_cpu"], n["alloc_memory"], n["alloc_ephemeral"], n["alloc_pods"] = cpu, mem, eph, pods
    n["alloc_scalar"][0][SCALAR_COL] = scalar
    n["taints"] = np.uint64(taints)
    n["label_pairs"][0][0] = np.uint64(labels)
    n["flags"] = abi.CA_NODE_UNSCHEDULABLE if unsched else 0
    n["name_id"] = name_id
    return n


NODE_CPU = (1000, 4000, 7777)
NODE_MEM = (4 * GI + 3, 16 * GI, 40 * GI + 1)
NODE_EPH = (0, 10 * GI, 100 * GI + 1)


def gen_nodes(rng: random.Random, n: int, first_name: int, plain: float = 0.5) -> np.ndarray:
    """n node records with distinct name_ids first_name ...; `plain` of them carry neither
    taints, labels nor the unschedulable flag."""
    out = abi.empty_nodes(n)
    for i in range(n):
        bare = rng.random() < plain
        out[i] = node_record(first_name + i, rng.choice(NODE_CPU), rng.choice(NODE_MEM), rng.choice(NODE_EPH),
                             rng.choice((3, 10, 110)), rng.choice((0, 4)),
                             0 if bare else rng.choice(TAINT_SETS), 0 if bare else rng.choice(LABEL_SETS),
                             (not bare) and rng.random() < 0.2)[0]
    return out


def gen_pod_table(rng: random.Random, blockers: bool = True) -> abi.PodTable:
    """The pod shapes a sequence draws from: requests from small sets that are no powers of two,
    all-zero pods, scalar requests, single port bits, tolerations; one scope blocker."""
    recs = [pod_record(), pod_record(tolerated=0b11), pod_record(flags=abi.CA_POD_HAS_SCALAR_KEYS)]
    for _ in range(24):
        kind = rng.random()
        recs.append(pod_record(
            cpu=rng.choice((0, CPU_REQ, 2 * CPU_REQ + 1)), mem=rng.choice((0, MEM_REQ, 3 * MEM_REQ)),
            eph=rng.choice((0, 0, EPH_REQ)),
            scalar=rng.choice((1, 3)) if kind < 0.25 else 0,
            port=rng.choice(PORT_BITS) if 0.2 < kind < 0.5 else None,
            tolerated=rng.choice(TAINT_SETS), selector=rng.choice((0, 0, 0) + SELECTORS),
            flags=abi.CA_POD_HAS_SCALAR_KEYS if kind < 0.25 else 0))
    for b in PORT_BITS[:2]:                       # shared port triples come up often
        recs.append(pod_record(cpu=CPU_REQ, port=b))
        recs.append(pod_record(mem=MEM_REQ, port=b))
    if blockers:
        recs.append(pod_record(cpu=CPU_REQ, flags=abi.CA_POD_REQUIRED_ANTI_AFFINITY))
    return abi.PodTable(np.concatenate(recs))


# ---------------------------------------------------------------------------
# probes and the fit rule
# ---------------------------------------------------------------------------
class Probes:
    def __init__(self, recs, tags):
        self.table = abi.PodTable(np.concatenate(recs))
        self.tags = tags                         # per probe: (dimension, what)
        self.dims = sorted({t[0] for t in tags})


def probes_from_free(free: dict, scalar_cols=(SCALAR_COL,), extra=True) -> Probes:
    """free: dimension -> iterable of the nodes' free values.  One probe at f and one at f + 1
    for every distinct positive f, an all-zero and a memory-only probe (free cpu 0 against
    free cpu < 0), one per port bit, toleration set and selector of the generator."""
    recs, tags = [], []

    def add(rec, dim, what):
        recs.append(rec)
        tags.append((dim, what))

    def bracket(dim, values, write):             # the records in one array: thousands of probes at 300 nodes
        req = [r for f in sorted({int(v) for v in values if v > 0}) for r in (f, f + 1)]
        if not req:
            return
        p = abi.empty_pods(len(req))
        p["tolerated_taints"] = np.uint64(U64)
        p["flags"] = abi.CA_POD_TOLERATES_UNSCHED
        write(p, np.array(req, np.int64))
        recs.append(p)
        tags.extend((dim, f"{dim}={r}") for r in req)

    def column(field):
        def write(p, req):
            p[field] = req
            if field != "req_ephemeral":
                p["score_milli_cpu" if field == "req_milli_cpu" else "score_memory"] = req
        return write

    def scalar(k):
        def write(p, req):
            p["req_scalar"][:, k] = req
            p["flags"] |= abi.CA_POD_HAS_SCALAR_KEYS
        return write

    bracket("cpu", free.get("cpu", ()), column("req_milli_cpu"))
    bracket("mem", free.get("mem", ()), column("req_memory"))
    bracket("eph", free.get("eph", ()), column("req_ephemeral"))
    for k in scalar_cols:
        bracket(f"scalar{k}", free.get(f"scalar{k}", ()), scalar(k))
    add(pod_record(**RES_TOL), "zero", "all-zero")
    add(pod_record(mem=1, **RES_TOL), "zero", "memory-only")
    if extra:
        p = pod_record(**RES_TOL)
        p["flags"] |= abi.CA_POD_HAS_SCALAR_KEYS
        add(p, "zero", "all-zero+scalar-keys")
        for b in PORT_BITS:
            add(pod_record(port=b, **RES_TOL), "ports", f"port{b}")
        for t in TAINT_SETS:
            add(pod_record(tolerated=t), "taints", f"tolerates={t:#b}")
        for s in SELECTORS:
            add(pod_record(selector=s, **RES_TOL), "labels", f"selector={s:#b}")
    return Probes(recs, tags)


def probes(model: SnapModel) -> Probes:
    fr = [model.free(x) for x in range(model.node_count())]
    free = {d: [f[d] for f in fr] for d in ("cpu", "mem", "eph")}
    free[f"scalar{SCALAR_COL}"] = [f["scalar"][SCALAR_COL] for f in fr]
    return probes_from_free(free)


def _fit_rule(pods, unsched, taints, labels, ports, slots, cpu, mem, eph, scalar) -> np.ndarray:
    """[probe][node] fits, a numpy broadcast of the rule in the module docstring.  Node columns
    are arrays over the nodes (labels [N][4], ports [N][2], scalar [N][8])."""
    P = lambda f: pods[f][:, None]                                             # noqa: E731
    flags = P("flags")
    ok = ~(unsched[None, :] & ((flags & abi.CA_POD_TOLERATES_UNSCHED) == 0))
    ok &= (taints[None, :] & ~P("tolerated_taints")) == 0
    sel = pods["node_selector"][:, None, :]
    aff = ((labels[None, :, :] & sel) == sel).all(axis=2)
    ok &= ((flags & abi.CA_POD_AFFINITY_FILTER) == 0) | aff
    ok &= ((ports[None, :, :] & pods["port_conflict"][:, None, :]) == 0).all(axis=2)
    ok &= slots[None, :] >= 1                                                  # npods + 1 <= alloc_pods
    all_zero = ((P("req_milli_cpu") == 0) & (P("req_memory") == 0) & (P("req_ephemeral") == 0) &
                ((flags & abi.CA_POD_HAS_SCALAR_KEYS) == 0))
    rs = pods["req_scalar"][:, None, :]
    res = ((P("req_milli_cpu") <= cpu[None, :]) & (P("req_memory") <= mem[None, :]) &
           (P("req_ephemeral") <= eph[None, :]) & ((rs == 0) | (rs <= scalar[None, :, :])).all(axis=2))
    ok &= all_zero | res
    return ok.astype(np.uint8)


def expected_fits(model: SnapModel, pr: Probes) -> np.ndarray:
    n = model.node_count()
    fr = [model.free(x) for x in range(n)]
    recs = [nd.rec for nd in model.nodes]
    i64 = lambda v: np.array(v, np.int64)                                      # noqa: E731
    return _fit_rule(
        pr.table.pods,
        np.array([bool(int(r["flags"]) & abi.CA_NODE_UNSCHEDULABLE) for r in recs], bool),
        np.array([int(r["taints"]) for r in recs], np.uint64),
        np.array([r["label_pairs"] for r in recs], np.uint64).reshape(n, abi.CA_LABEL_WORDS),
        np.array([nd.ports for nd in model.nodes], np.uint64).reshape(n, abi.CA_PORT_WORDS),
        i64([f["slots"] for f in fr]), i64([f["cpu"] for f in fr]), i64([f["mem"] for f in fr]),
        i64([f["eph"] for f in fr]), np.array([f["scalar"] for f in fr], np.int64).reshape(n, abi.CA_MAX_SCALAR))


def probe_coverage(pr: Probes, exp: np.ndarray) -> bool:
    """Every dimension of the probe set has a fitting and a non-fitting (probe, node) cell."""
    dim_of = np.array([t[0] for t in pr.tags])
    for d in pr.dims:
        cells = exp[dim_of == d]
        if cells.size == 0 or cells.min() == cells.max():
            return False
    return True


# ---------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------
def backend_fits(backend, pr: Probes, n_nodes: int) -> np.ndarray:
    """[probe][node] of the backend: the mirror's fits_matrix in batches of at most 4096 probes,
    the oracle's check_predicates cell by cell."""
    t = pr.table
    if hasattr(backend, "fits_matrix"):
        if len(t) <= 4096:
            return backend.fits_matrix(t)
        parts = [backend.fits_matrix(abi.PodTable(t.pods[a:a + 4096])) for a in range(0, len(t), 4096)]
        return np.concatenate(parts)
    out = np.zeros((len(t), n_nodes), np.uint8)
    r = abi.PredResultC()
    fn, h, ref, rr = backend.lib.or_check_predicates, backend.h, t.ref, C.byref(r)
    for p in range(len(t)):
        for x in range(n_nodes):
            st = fn(h, ref, p, x, rr)
            if st != abi.CA_OK:
                e = RuntimeError(f"or_check_predicates: status {st}")
                e.status = st
                raise e
            out[p, x] = r.type == abi.CA_PRED_OK
    return out


def _diff_cell(pr: Probes, got: np.ndarray, exp: np.ndarray) -> str:
    p, x = (int(v[0]) for v in np.nonzero(got != exp))
    dim, what = pr.tags[p]
    return (f"node {x}, probe {p} ({what}), dimension {dim}: backend fits={int(got[p, x])}, expected "
            f"{int(exp[p, x])} ({int((got != exp).sum())} cells differ)")


def assert_lists(backend, n: int, node_pods, pod_node, blockers: int, ctx: str) -> None:
    who = backend.backend_name
    assert backend.node_count() == n, f"{ctx}: {who} node_count {backend.node_count()} != {n}"
    for x in range(n):
        got = backend.node_pods(x)
        assert got == node_pods[x], f"{ctx}: {who} node {x} pods {got} != {node_pods[x]}"
    for pid, x in enumerate(pod_node):
        got = backend.pod_node(pid)
        assert got == x, f"{ctx}: {who} pod {pid} on node {got}, expected {x}"
    assert backend.scope_blockers() == blockers, f"{ctx}: {who} scope_blockers {backend.scope_blockers()} != {blockers}"


def assert_state(backend, model: SnapModel, ctx: str = "", with_probes: bool = True, hints: bool = False,
                 stats: dict | None = None) -> None:
    """The backend's whole state against the model.  ctx names the seed, the step and the op."""
    n = model.node_count()
    blockers = model.scope_blockers()
    assert_lists(backend, n, [nd.pods for nd in model.nodes], model.pod_nodes(), blockers, ctx)
    if with_probes and n:
        pr = probes(model)
        if blockers:                             # kernel scope: every simulation is refused
            try:
                backend_fits(backend, Probes([pr.table.pods[:1]], pr.tags[:1]), n)
                refused = False
            except RuntimeError as e:
                refused = getattr(e, "status", None) == abi.CA_EUNSUPPORTED
            assert refused, f"{ctx}: {backend.backend_name} evaluated predicates with {blockers} scope blockers"
        else:
            exp = expected_fits(model, pr)
            got = backend_fits(backend, pr, n)
            if stats is not None:
                stats["checked"] = stats.get("checked", 0) + 1
                stats["covered"] = stats.get("covered", 0) + int(probe_coverage(pr, exp))
            assert np.array_equal(got, exp), f"{ctx}: {backend.backend_name} {_diff_cell(pr, got, exp)}"
    if hints and len(model.pod_rec):
        got = backend.get_hints(len(model.pod_rec))
        for pid, want in enumerate(model.expected_hints()):
            g = int(got[pid])
            assert (g < 0) if want is None else (g == want), \
                f"{ctx}: pod {pid} hint {g}, expected {'< 0 (node gone)' if want is None else want}"


def assert_state_oracle(backend, oracle, n_pods: int, ctx: str = "", scalar_cols=(), port_bits=()) -> None:
    """The second form: the expectation comes from a driven oracle.  node_state gives the free
    cpu, memory, ephemeral-storage and slots (bracketed by probes as above; every other column
    of those probes is neutral), check_predicates the cells of the scalar and port probes and of
    one probe that tolerates nothing (the static column)."""
    n = oracle.node_count()
    assert_lists(backend, n, [oracle.node_pods(x) for x in range(n)], [oracle.pod_node(i) for i in range(n_pods)],
                 oracle.scope_blockers(), ctx)
    if not n:
        return
    st = np.array([oracle.node_state(x) for x in range(n)], np.int64).reshape(n, 4)
    pr = probes_from_free({"cpu": st[:, 0], "mem": st[:, 1], "eph": st[:, 2]}, scalar_cols=(), extra=False)
    z = np.zeros(n, np.uint64)
    exp = _fit_rule(pr.table.pods, np.zeros(n, bool), z, np.zeros((n, abi.CA_LABEL_WORDS), np.uint64),
                    np.zeros((n, abi.CA_PORT_WORDS), np.uint64), st[:, 3], st[:, 0], st[:, 1], st[:, 2],
                    np.zeros((n, abi.CA_MAX_SCALAR), np.int64))
    got = backend_fits(backend, pr, n)
    assert np.array_equal(got, exp), f"{ctx}: {backend.backend_name} {_diff_cell(pr, got, exp)}"
    recs, tags = [pod_record()], [("static", "all-zero, tolerates nothing")]
    for k in scalar_cols:
        for r in (1, 2, 3, 4, 5):
            p = pod_record(**RES_TOL)
            p["req_scalar"][0][k] = r
            p["flags"] |= abi.CA_POD_HAS_SCALAR_KEYS
            recs.append(p)
            tags.append((f"scalar{k}", f"scalar{k}={r}"))
    for b in port_bits:
        recs.append(pod_record(port=b, **RES_TOL))
        tags.append(("ports", f"port{b}"))
    pr = Probes(recs, tags)
    exp, got = backend_fits(oracle, pr, n), backend_fits(backend, pr, n)
    assert np.array_equal(got, exp), f"{ctx}: {backend.backend_name} {_diff_cell(pr, got, exp)}"


# ---------------------------------------------------------------------------
# seeded sequences
# ---------------------------------------------------------------------------
OPS = ("fork", "add_pods", "remove_pod", "remove_node", "add_nodes", "revert", "commit")
KINDS = ("add_node", "add_pod", "remove_pod", "remove_node")


class Sequence:
    """One seeded run: every step picks an op from the model's state, applies it to the model
    and to every backend, and records what the coverage assertions ask about."""

    def __init__(self, seed: int, n_nodes: int = 12, max_depth: int = 3):
        self.seed, self.rng = seed, random.Random(f"snapmodel/{seed}")
        self.table = gen_pod_table(self.rng)
        self.model = SnapModel(self.table)
        self.first_nodes = gen_nodes(self.rng, n_nodes, 0)
        self.next_name = n_nodes
        self.min_nodes, self.max_nodes, self.max_depth = max(3, n_nodes - 6), n_nodes + 8, max_depth
        self.frames: list = []                   # per open fork: journal kinds, names added, inner commit seen
        self.cov = {op: 0 for op in OPS}
        self.cov.update({f"revert_over_{k}": 0 for k in KINDS})
        self.cov.update(max_depth=0, commit_then_outer_revert=0, remove_node_depth0=0, node_added_removed_in_fork=0,
                        shared_port=0, overcommitted=0, blockers=0)
        self.step = 0
        self.op = "load"

    def load(self, backends) -> None:
        self.model.add_nodes(self.first_nodes)
        for b in backends:
            b.clear()
            b.add_nodes(self.first_nodes)

    def ctx(self) -> str:
        return f"seed {self.seed} step {self.step} op {self.op}"

    def _note(self, kind: str) -> None:
        if self.frames:
            self.frames[-1]["kinds"].add(kind)

    def _choose(self) -> str:
        m, rng = self.model, self.rng
        placed = m.placed()
        if m.scope_blockers() and rng.random() < 0.6:
            return "remove_blocker"
        w = {"fork": 2 if m.depth < self.max_depth else 0, "add_pods": 7, "remove_pod": 3 if placed else 0,
             "remove_node": 1 if m.node_count() > self.min_nodes else 0,
             "add_nodes": 1 if m.node_count() < self.max_nodes else 0,
             "revert": 2 if m.depth else 0, "commit": 1 if m.depth else 0}
        return rng.choices(list(w), list(w.values()))[0]

    def next(self, backends) -> str:
        """Apply one op everywhere; returns its name."""
        m, rng = self.model, self.rng
        self.step += 1
        op = self._choose()
        if op == "remove_blocker":
            f = self.table.pods["flags"]
            pid = next(p for p in m.placed() if int(f[m.pod_rec[p]]) & abi.CA_POD_REQUIRED_ANTI_AFFINITY)
            op, arg = "remove_pod", pid
        elif op == "remove_pod":
            arg = rng.choice(m.placed())
        elif op == "add_pods":
            k = rng.choice((1, 1, 2, 3))
            x0 = rng.randrange(m.node_count())
            # (clustered on a few nodes: shared ports, overcommitted rows and full nodes come up)
            arg = ([rng.randrange(len(self.table)) for _ in range(k)],
                   [x0 if rng.random() < 0.6 else rng.randrange(m.node_count()) for _ in range(k)])
        elif op == "remove_node":
            arg = rng.choice((0, m.node_count() - 1, rng.randrange(m.node_count())))
        elif op == "add_nodes":
            k = rng.choice((1, 2))
            arg = gen_nodes(rng, k, self.next_name)
            self.next_name += k
        else:
            arg = None
        self.op = op
        self.cov[op] += 1
        # the records the coverage assertions ask about
        if op == "fork":
            self.frames.append({"kinds": set(), "names": set(), "inner_commit": False})
            self.cov["max_depth"] = max(self.cov["max_depth"], m.depth + 1)
        elif op == "add_pods":
            self._note("add_pod")
            for i, x in zip(*arg):
                use = self.table.pods[i]["port_use"]
                if any(int(use[w]) & m.nodes[x].ports[w] for w in range(abi.CA_PORT_WORDS)):
                    self.cov["shared_port"] += 1
                if int(self.table.pods[i]["flags"]) & abi.CA_POD_REQUIRED_ANTI_AFFINITY:
                    self.cov["blockers"] += 1
        elif op == "remove_pod":
            self._note("remove_pod")
        elif op == "remove_node":
            self._note("remove_node")
            name = int(m.nodes[arg].rec["name_id"])
            if not m.depth:
                self.cov["remove_node_depth0"] += 1
            elif name in self.frames[-1]["names"]:
                self.cov["node_added_removed_in_fork"] += 1
        elif op == "add_nodes":
            self._note("add_node")
            if self.frames:
                self.frames[-1]["names"].update(int(v) for v in arg["name_id"])
        elif op == "revert":
            fr = self.frames.pop()
            for k in fr["kinds"]:
                self.cov[f"revert_over_{k}"] += 1
            self.cov["commit_then_outer_revert"] += int(fr["inner_commit"])
        elif op == "commit":
            fr = self.frames.pop()
            if self.frames:                      # the entries now belong to the enclosing fork
                self.frames[-1]["kinds"] |= fr["kinds"]
                self.frames[-1]["names"] |= fr["names"]
                self.frames[-1]["inner_commit"] = True
        # the op itself
        if op == "add_pods":
            ids = m.add_pods(*arg)
            for b in backends:
                got = b.add_pods(self.table, *arg).tolist()
                assert got == ids, f"{self.ctx()}: {b.backend_name} issued ids {got}, expected {ids}"
            x = arg[1][0]
            f = m.free(x)
            self.cov["overcommitted"] += int(min(f["cpu"], f["mem"], f["eph"], f["slots"]) < 0)
        else:
            a = () if arg is None else (arg,)
            getattr(m, op)(*a)
            for b in backends:
                getattr(b, op)(*a)
        return op


def run_sequence(seed: int, backends, steps: int, n_nodes: int = 12, every: int = 1, with_probes: bool = True,
                 stats: dict | None = None) -> Sequence:
    """Drive `backends` and the model through `steps` ops, assert_state after every `every`-th
    mutating step and at the end."""
    s = Sequence(seed, n_nodes)
    s.load(backends)
    for b in backends:
        assert_state(b, s.model, s.ctx(), with_probes, stats=stats)
    for i in range(steps):
        s.next(backends)
        if (i + 1) % every == 0 or i + 1 == steps:
            for b in backends:
                assert_state(b, s.model, s.ctx(), with_probes, stats=stats)
    return s
