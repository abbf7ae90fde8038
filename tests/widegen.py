"""Seeded clusters of API objects over a vocabulary sized just inside every fixed width of
the ABI records: 256 label pairs over 60 keys, 64 Exists / DoesNotExist keys, 4 Gt / Lt
keys, 63 taint classes, 128 host-port triples (32 (protocol, port) groups of a wildcard
and three addresses), 8 extended resources.

Interner ids are given in observation order (nodes, then pods).  Each vocabulary is
walked in a seeded permutation by the first objects ("cover" taints, resources,
requirements and ports: one slice each), so every id up to the last position of each
width is assigned, to a random member; everything else draws from the whole vocabulary,
so the ids the objects use are spread over every word.

`extra_taint` adds one taint class past the width on the last node (bit 63 of its record).
"""
from __future__ import annotations

import random
from dataclasses import dataclass

import numpy as np

from autoscaler_amd import abi
from autoscaler_amd.intern import Interner
from autoscaler_amd.k8s import (Affinity, Container, ContainerPort, Node, NodeSelectorRequirement, NodeSelectorTerm,
                                OwnerReference, Pod, Quantity, Taint, Toleration)

LKEYS = [f"lk{i}" for i in range(60)]
LVALS = {k: [f"v{j}" for j in range(5 if i < 16 else 4)] for i, k in enumerate(LKEYS)}       # 16*5 + 44*4 = 256
PAIRS = [(k, v) for k in LKEYS for v in LVALS[k]]
XKEYS = LKEYS + [f"xk{i}" for i in range(4)]                                                # 64
IKEYS = [f"rank{i}" for i in range(4)]
TKEYS = [f"tk{i}" for i in range(9)]
TAINTS = [(TKEYS[c % 9], f"tv{c // 9}", "NoSchedule" if c % 2 else "NoExecute") for c in range(63)]
OVER_TAINT = ("tk-over", "x", "NoSchedule")
IPS = ["0.0.0.0", "10.0.0.1", "10.0.0.2", "10.0.0.3"]
PORTS = [(ip, proto, 8000 + g) for g in range(16) for proto in ("TCP", "UDP") for ip in IPS]  # 128
EXT = [f"example.com/r{i}" for i in range(8)]
assert len(PAIRS) == 256 and len(XKEYS) == 64 and len(TAINTS) == 63 and len(PORTS) == 128


@dataclass
class WideCase:
    seed: int
    nodes: list
    pods: list                 # every pod, in the order the interner observes them
    sched_pos: list            # positions in `pods` of the scheduled pods (spread over the list)
    node_of: list              # their node positions
    pend_pos: list             # positions in `pods` of the pending pods
    templates: list            # (Node, [DaemonSet pods])
    groups: list               # per template: indices into `pend_pos`

    @property
    def scheduled(self) -> list:
        return [(self.pods[i], self.node_of[k]) for k, i in enumerate(self.sched_pos)]

    @property
    def pending(self) -> list:
        return [self.pods[i] for i in self.pend_pos]


@dataclass
class Encoded:
    it: Interner
    node_recs: np.ndarray
    table: abi.PodTable        # every pod of the case, in observation order
    sched_idx: np.ndarray      # table rows of the scheduled pods: mirror pod k is row sched_idx[k]
    node_of: np.ndarray
    pending: np.ndarray        # table rows of the pending pods
    templates: np.ndarray
    group_off: np.ndarray
    pod_idx: np.ndarray

    @property
    def n_sched(self) -> int:
        return len(self.sched_idx)

    def load(self, b) -> None:
        b.clear()
        b.add_nodes(self.node_recs)
        if self.n_sched:
            b.add_pods(self.table, self.sched_idx, self.node_of)


def _node(rng: random.Random, name: str, big: bool = False) -> Node:
    labels = {}
    for k in LKEYS:
        if rng.random() < 0.6:
            labels[k] = rng.choice(LVALS[k]) if rng.random() < 0.9 else "other"
    for k in XKEYS[60:]:
        if rng.random() < 0.5:
            labels[k] = "y"
    for k in IKEYS:
        if rng.random() < 0.7:
            labels[k] = str(rng.randint(-5, 20)) if rng.random() < 0.9 else "NaN"
    scale = 4 if big else 1
    alloc = {"cpu": Quantity.milli(rng.choice([4000, 8000, 16000]) * scale),
             "memory": Quantity(rng.choice([8, 16, 32]) * (1 << 30) * scale),
             "pods": Quantity(rng.choice([8, 30, 110]))}
    if rng.random() < 0.3:
        alloc["ephemeral-storage"] = Quantity(20 << 30)
    for r in rng.sample(EXT, rng.randint(1, 4)):
        alloc[r] = Quantity(rng.randint(1, 8) * scale)
    return Node(name=name, labels=labels, taints=[], allocatable=alloc, unschedulable=rng.random() < 0.04)


def _tolerations(rng: random.Random) -> list:
    if rng.random() < 0.2:
        return [Toleration(operator="Exists")]
    tols = [Toleration(key=k, operator="Exists") for k in TKEYS if rng.random() < 0.8]
    for _ in range(rng.randint(0, 3)):
        k, v, e = rng.choice(TAINTS)
        tols.append(Toleration(key=k, operator="Equal", value=v, effect=rng.choice([e, ""])))
    if rng.random() < 0.1:
        tols.append(Toleration(key=OVER_TAINT[0], operator="Exists"))
    if rng.random() < 0.1:
        tols.append(Toleration(key="node.kubernetes.io/unschedulable", operator="Exists", effect="NoSchedule"))
    return tols


def _expr(rng: random.Random) -> NodeSelectorRequirement:
    op = rng.choice(["In", "In", "NotIn", "Exists", "DoesNotExist", "Gt", "Lt"])
    if op in ("In", "NotIn"):
        k = rng.choice(LKEYS)
        return NodeSelectorRequirement(k, op, rng.sample(LVALS[k], rng.randint(1, 3)))
    if op in ("Exists", "DoesNotExist"):
        return NodeSelectorRequirement(rng.choice(XKEYS), op, [])
    return NodeSelectorRequirement(rng.choice(IKEYS), op, [str(rng.randint(-3, 15))])


def _pod(rng: random.Random, name: str, light: bool = False) -> Pod:
    req = {"cpu": Quantity.milli(rng.choice([0, 50, 100, 250, 500, 1000])),
           "memory": Quantity(rng.choice([0, 64, 256, 1024]) << 20)}
    if rng.random() < 0.3:
        for r in rng.sample(EXT, rng.randint(1, 2)):
            req[r] = Quantity(rng.choice([1, 1, 2]))
    ports = []
    if rng.random() < 0.3:
        ip, proto, port = rng.choice(PORTS)
        ports.append(ContainerPort(host_port=port, host_ip=rng.choice([ip, "" if ip == "0.0.0.0" else ip]),
                                   protocol=rng.choice([proto, "" if proto == "TCP" else proto])))
    p = Pod(name=name, uid=name, containers=[Container(requests=req, ports=ports)], tolerations=_tolerations(rng))
    if rng.random() < (0.1 if light else 0.3):
        k = rng.choice(LKEYS)
        p.node_selector = {k: rng.choice(LVALS[k])}
    if rng.random() < (0.25 if light else 0.5):
        p.affinity = Affinity(required_terms=[NodeSelectorTerm([_expr(rng) for _ in range(rng.randint(1, 2))])
                                              for _ in range(rng.randint(1, 2))])
    if rng.random() < 0.7:
        rs = f"rs{rng.randint(0, 9)}"
        p.owner_refs = [OwnerReference("ReplicaSet", rs, rs)]
    return p


def _add_term(rng: random.Random, p: Pod, r: NodeSelectorRequirement) -> None:
    """A cover requirement: mostly a term of its own (terms are ORed), else inside the first."""
    if p.affinity is None or not p.affinity.required_terms:
        p.affinity = Affinity(required_terms=[NodeSelectorTerm([r])])
    elif rng.random() < 0.7:
        p.affinity.required_terms.append(NodeSelectorTerm([r]))
    else:
        p.affinity.required_terms[0].match_expressions.append(r)


def wide_case(seed: int, n_nodes: int = 24, n_sched: int = 48, n_pending: int = 120, n_templates: int = 5,
              extra_taint: bool = False) -> WideCase:
    assert n_nodes >= 8 and n_sched + n_pending >= 64
    rng = random.Random(f"widegen/{seed}/{n_nodes}/{n_sched}/{n_pending}/{extra_taint}")
    perm = lambda n: rng.sample(range(n), n)                                   # noqa: E731
    tperm, eperm, kperm, xperm, iperm, pperm = perm(63), perm(8), perm(60), perm(64), perm(4), perm(128)
    nodes = [_node(rng, f"n{i}") for i in range(n_nodes)]
    for i, n in enumerate(nodes):
        for c in tperm[i::n_nodes]:                                            # cover: every class, in tperm order
            n.taints.append(Taint(*TAINTS[c]))
        if rng.random() < 0.4:
            t = Taint(*rng.choice(TAINTS))
            if t not in n.taints:
                n.taints.append(t)
        if rng.random() < 0.2:
            n.taints.append(Taint("soft", "x", "PreferNoSchedule"))
        if i < 8:
            n.allocatable.setdefault(EXT[eperm[i]], Quantity(rng.randint(1, 8)))
    if extra_taint:
        nodes[-1].taints.append(Taint(*OVER_TAINT))
    # scheduled pods sit at random places of the observation order, so the rows' used ports
    # and the movable pods' requirements get ids of every word too
    sched_pos = sorted(rng.sample(range(n_sched + n_pending), n_sched))
    is_sched = set(sched_pos)
    pods = [_pod(rng, f"s{j}", light=True) if j in is_sched else _pod(rng, f"p{j}") for j in range(n_sched + n_pending)]
    for j, p in enumerate(pods[:64]):
        if j < 60:
            k = LKEYS[kperm[j]]
            _add_term(rng, p, NodeSelectorRequirement(k, rng.choice(["In", "In", "NotIn"]),
                                                      rng.sample(LVALS[k], len(LVALS[k]))))
        _add_term(rng, p, NodeSelectorRequirement(XKEYS[xperm[j]], rng.choice(["Exists", "DoesNotExist"]), []))
        if j < 4:
            _add_term(rng, p, NodeSelectorRequirement(IKEYS[iperm[j]], rng.choice(["Gt", "Lt"]), [str(rng.randint(0, 12))]))
        for x in pperm[2 * j:2 * j + 2]:
            ip, proto, port = PORTS[x]
            p.containers[0].ports.append(ContainerPort(host_port=port, host_ip=ip, protocol=proto))
    pend_pos = [j for j in range(len(pods)) if j not in is_sched]
    templates, groups = [], []
    for g in range(n_templates):
        t = _node(rng, f"tmpl{g}", big=True)
        t.unschedulable = False
        for c in rng.sample(range(63), rng.randint(0, 3)):
            t.taints.append(Taint(*TAINTS[c]))
        ds = []
        for d in range(rng.randint(1, 2)):
            q = _pod(rng, f"ds{g}-{d}", light=True)
            q.affinity, q.node_selector = None, None
            for ip, proto, port in rng.sample(PORTS, 2):                       # template rows carry used ports
                q.containers[0].ports.append(ContainerPort(host_port=port, host_ip=ip, protocol=proto))
            q.owner_refs = [OwnerReference("DaemonSet", f"ds{g}", f"ds{g}")]
            ds.append(q)
        templates.append((t, ds))
        groups.append([i for i in range(n_pending) if rng.random() < 0.7])
    return WideCase(seed, nodes, pods, sched_pos, [k % n_nodes for k in range(n_sched)], pend_pos, templates, groups)


def encode(case: WideCase) -> Encoded:
    pods = case.pods
    it = Interner(case.nodes, pods, case.templates)
    node_recs = it.encode_nodes(case.nodes)
    table = it.encode_pods(pods)
    tm = np.zeros(len(case.templates), abi.TEMPLATE_DTYPE)
    for g, (t, ds) in enumerate(case.templates):
        tm[g] = it.encode_template(t, ds)
    off, idx = [0], []
    for sel in case.groups:
        idx.extend(case.pend_pos[i] for i in sel)
        off.append(len(idx))
    return Encoded(it, node_recs, table, np.array(case.sched_pos, np.int32), np.array(case.node_of, np.int32),
                   np.array(case.pend_pos, np.int32), tm, np.array(off, np.int32), np.array(idx, np.int32))


# The upper part of every fixed width: what a kernel, a staging loop or a host row builder
# that dropped or mis-indexed the upper words would lose.
UPPER_PARTS = ("label-word-1", "label-word-2", "label-word-3", "keys-32+", "taints-32+", "port-word-1",
               "scalars-2+", "int-keys-1+")
HI32 = np.uint64(0xFFFFFFFF00000000)
LO32 = np.uint64(0x00000000FFFFFFFF)


def upper_bits(e: Encoded) -> dict:
    """part -> does any node / pod / requirement / template record use it."""
    n, p, r, t = e.node_recs, e.table.pods, e.table.reqs, e.templates
    exists = np.isin(r["op"], (abi.CA_OP_EXISTS, abi.CA_OP_DOESNOTEXIST))
    gtlt = np.isin(r["op"], (abi.CA_OP_GT, abi.CA_OP_LT))
    out = {}
    for w in (1, 2, 3):
        out[f"label-word-{w}"] = {"node": bool(n["label_pairs"][:, w].any()), "selector": bool(p["node_selector"][:, w].any()),
                                  "req": bool(r["pairs"][:, w].any()), "template": bool(t["node"]["label_pairs"][:, w].any())}
    out["keys-32+"] = {"node": bool((n["label_keys"] & HI32).any()), "req": bool((r["key"][exists] >= 32).any()),
                       "last": bool((r["key"][exists] == 63).any()) and bool(((n["label_keys"] >> np.uint64(63)) & np.uint64(1)).any())}
    out["taints-32+"] = {"node": bool((n["taints"] & HI32).any()), "pod": bool((p["tolerated_taints"] & HI32).any()),
                         "last": bool(((n["taints"] >> np.uint64(62)) & np.uint64(1)).any()),
                         "template": bool((t["node"]["taints"] & HI32).any())}
    out["port-word-1"] = {"use": bool(p["port_use"][:, 1].any()), "conflict": bool(p["port_conflict"][:, 1].any()),
                          "last": bool(((p["port_use"][:, 1] >> np.uint64(63)) & np.uint64(1)).any()),
                          "template": bool(t["used_ports"][:, 1].any())}
    out["scalars-2+"] = {"node": bool(n["alloc_scalar"][:, 2:].any()), "pod": bool(p["req_scalar"][:, 2:].any()),
                         "last": bool(n["alloc_scalar"][:, 7].any()) and bool(p["req_scalar"][:, 7].any()),
                         "template": bool(t["node"]["alloc_scalar"][:, 2:].any())}
    out["int-keys-1+"] = {"node": bool((n["int_label_valid"] & 0xE).any()), "req": bool((r["key"][gtlt] >= 1).any()),
                          "last": bool((r["key"][gtlt] == 3).any()) and bool((n["int_label_valid"] & 0x8).any())}
    return out


def clear_upper(e: Encoded, part: str) -> Encoded:
    """A copy of the records with only that upper part cleared (node, template and pod side)."""
    n, t = e.node_recs.copy(), e.templates.copy()
    p, r = e.table.pods.copy(), e.table.reqs.copy()
    if part.startswith("label-word-"):
        w = int(part[-1])
        n["label_pairs"][:, w] = 0
        t["node"]["label_pairs"][:, w] = 0
        p["node_selector"][:, w] = 0
        r["pairs"][:, w] = 0
    elif part == "keys-32+":
        n["label_keys"] &= LO32
        t["node"]["label_keys"] &= LO32
    elif part == "taints-32+":
        n["taints"] &= LO32
        t["node"]["taints"] &= LO32
    elif part == "port-word-1":
        p["port_use"][:, 1] = 0
        p["port_conflict"][:, 1] = 0
        t["used_ports"][:, 1] = 0
    elif part == "scalars-2+":
        n["alloc_scalar"][:, 2:] = 0
        t["node"]["alloc_scalar"][:, 2:] = 0
    elif part == "int-keys-1+":
        n["int_label_valid"] &= 1
        t["node"]["int_label_valid"] &= 1
    else:
        raise KeyError(part)
    return Encoded(e.it, n, abi.PodTable(p, e.table.terms, r, e.table.names), e.sched_idx, e.node_of, e.pending, t,
                   e.group_off, e.pod_idx)


def sweep_args(e: Encoded, seed: int):
    """FindNodesToRemove / Planner inputs over every node of the cluster."""
    rng = random.Random(f"widegen/sweep/{seed}")
    n = len(e.node_recs)
    cands = np.array(rng.sample(range(n), n), np.int32)
    off, moves = [0], []
    for c in cands.tolist():
        moves.extend(np.nonzero(e.node_of == c)[0].tolist())
        off.append(len(moves))
    hints = np.array([rng.choice([-1, -1, rng.randrange(n)]) for _ in range(e.n_sched)], np.int32)
    return (cands, np.ones(n, np.uint8), np.zeros(n, np.int32), np.array(off, np.int32),
            np.array(moves, np.int32)), hints


# (seed, nodes, scheduled, pending): 12-64 nodes, 40-400 pods.  The seeds are chosen so that
# every upper part decides verdicts (tests/test_edges_oracle.py checks that it does).
SIZES = [(5, 12, 24, 40), (1, 24, 48, 120), (2, 64, 128, 272)]


def plain_table(table: abi.PodTable) -> abi.PodTable:
    """The records without their host ports and extended-resource requests (the scope of the
    feasibility-bitmap walk and of the planner's device chain); labels, keys, taints and
    Gt/Lt stay."""
    p = table.pods.copy()
    p["port_use"] = 0
    p["port_conflict"] = 0
    p["req_scalar"] = 0
    p["tpu_scalar_mask"] = 0
    p["flags"] &= ~np.uint32(abi.CA_POD_HAS_SCALAR_KEYS | abi.CA_POD_HAS_NONTPU_SCALAR_KEYS)
    return abi.PodTable(p, table.terms, table.reqs, table.names)


def plain_encoded(e: Encoded) -> Encoded:
    """The cluster with every pod, scheduled ones included, stripped as plain_table does."""
    return Encoded(e.it, e.node_recs, plain_table(e.table), e.sched_idx, e.node_of, e.pending, e.templates,
                   e.group_off, e.pod_idx)


def filter_args(e: Encoded, plain: bool):
    """FilterOutSchedulable inputs: the table, the pending pods in table order, the
    controllers of their similar-pods classes, and hints for a third of them.  `plain`: the
    pending records without their host ports and extended-resource requests (the
    feasibility-bitmap walk takes only such pods; labels, keys, taints and Gt/Lt stay)."""
    table = plain_table(e.table) if plain else e.table
    order = e.pending
    rng = random.Random(f"widegen/filter/{len(table)}")
    n = len(e.node_recs)
    hints = np.array([rng.randrange(n) if rng.random() < 0.3 else -1 for _ in order], np.int32)   # per order slot
    owners = e.it.class_owners(int(table.pods["similar_class"].max()) + 1)
    return table, order, owners, hints
