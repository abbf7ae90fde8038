"""Scale-down eligibility from the mirror (ca_mirror_utilization, ca_scale_down_candidates):
the default / override row rule and the classification stated in numpy, and the cases, placed
where the kernels can go wrong.

A case is a cluster as the mirror holds it: node records, pod records by mirror pod id, the
node each pod was added to, and the ids removed afterwards (RemovePod swaps the node's last pod
into the hole, so NodeInfo.Pods order is not id order), plus the caller's override rows, the
clock, the thresholds and the eligibility mask.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from autoscaler_amd import abi

GI, MI = 1 << 30, 1 << 20
NOW = 1_608_310_800 * 10**9
DRAIN_BITS = abi.CA_UPOD_MOVABLE | abi.CA_UPOD_BLOCKING
HAS = abi.CA_UNODE_HAS_CPU | abi.CA_UNODE_HAS_MEM


# ---------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------
def rows_of(nodes, pod_specs, node_lists, node_over=None, pod_over=None):
    """(ca_util_node rows, pod_off, ca_util_pod rows in NodeInfo.Pods order): the table a caller
    of ca_util_table_create would have built.  nodes: NODE_DTYPE by position; pod_specs:
    POD_DTYPE by mirror pod id; node_lists[i]: node i's pod ids in NodeInfo.Pods order;
    node_over = (positions, UTIL_NODE rows) and pod_over = (ids, UTIL_POD rows) replace whole rows."""
    n = len(nodes)
    un = np.zeros(n, abi.UTIL_NODE_DTYPE)
    un["alloc_milli"][:, 0] = nodes["alloc_milli_cpu"]
    un["alloc_milli"][:, 1] = nodes["alloc_memory"] * 1000
    un["flags"] = HAS
    if node_over is not None and len(node_over[0]):
        un[np.asarray(node_over[0])] = node_over[1]
    up_all = pod_rows_by_id(pod_specs, pod_over)
    off = np.zeros(n + 1, np.int32)
    np.cumsum([len(l) for l in node_lists], out=off[1:])
    ids = np.fromiter((i for l in node_lists for i in l), np.int64, int(off[-1]))
    return un, off, up_all[ids]


def pod_rows_by_id(pod_specs, pod_over=None):
    """The ca_util_pod row of every mirror pod id (default, or its override)."""
    up = np.zeros(len(pod_specs), abi.UTIL_POD_DTYPE)
    up["req_milli"][:, 0] = pod_specs["score_milli_cpu"]
    up["req_milli"][:, 1] = pod_specs["score_memory"] * 1000
    ds = (pod_specs["flags"] & abi.CA_POD_DAEMONSET) != 0
    up["flags"] = np.where(ds, abi.CA_UPOD_DAEMONSET, abi.CA_UPOD_MOVABLE)
    if pod_over is not None and len(pod_over[0]):
        up[np.asarray(pod_over[0])] = pod_over[1]
    return up


def drain_of(pod_off, pods):
    """Per node: OR of CA_UPOD_MOVABLE | CA_UPOD_BLOCKING over its rows."""
    out = np.zeros(len(pod_off) - 1, np.int32)
    for i in range(len(out)):
        f = pods["flags"][pod_off[i]:pod_off[i + 1]]
        out[i] = int(np.bitwise_or.reduce(f & DRAIN_BITS)) if len(f) else 0
    return out


def candidates_of(info, drain, thr, gpu_thr, eligible, node_lists, pod_flags):
    """The classes and lists of ca_scale_down_candidates: dict(node_class, empty, cand,
    cand_status, move_off, move_pods).  pod_flags: CA_UPOD_* by mirror pod id."""
    n = len(info)
    cls = np.zeros(n, np.uint8)
    for i in range(n):
        t = gpu_thr if info["resource"][i] == abi.CA_UTIL_GPU else thr
        if eligible is not None and not eligible[i]:
            cls[i] = abi.CA_SD_INELIGIBLE
        elif info["status"][i] != abi.CA_UTIL_OK:
            cls[i] = abi.CA_SD_UTIL_ERROR
        elif info["utilization"][i] >= t:                      # NaN: not >=, so below
            cls[i] = abi.CA_SD_NOT_BELOW
        else:
            cls[i] = abi.CA_SD_EMPTY if drain[i] == 0 else abi.CA_SD_CANDIDATE
    cand = np.nonzero(cls == abi.CA_SD_CANDIDATE)[0].astype(np.int32)
    status = np.where(drain[cand] & abi.CA_UPOD_BLOCKING, abi.CA_UNREMOVABLE_BLOCKED_BY_POD, 0).astype(np.int32)
    off, moves = [0], []
    for c in cand:
        moves += [i for i in node_lists[c] if pod_flags[i] & abi.CA_UPOD_MOVABLE]
        off.append(len(moves))
    return dict(node_class=cls, empty=np.nonzero(cls == abi.CA_SD_EMPTY)[0].astype(np.int32), cand=cand,
                cand_status=status, move_off=np.array(off, np.int32), move_pods=np.array(moves, np.int32))


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    nodes: np.ndarray                       # NODE_DTYPE
    pods: np.ndarray                        # POD_DTYPE by mirror pod id
    pod_node: np.ndarray                    # node each id is added to
    removed: list = field(default_factory=list)
    node_over: tuple = None
    pod_over: tuple = None
    now_ns: int = NOW
    thr: float = 0.5
    gpu_thr: float = 0.5
    eligible: np.ndarray = None
    claims: dict = field(default_factory=dict)   # what the case is there for (test_mirror_util checks them)

    def node_lists(self) -> list:
        lists = [[] for _ in range(len(self.nodes))]
        for i, x in enumerate(self.pod_node.tolist()):
            lists[x].append(i)
        for i in self.removed:                                  # RemovePod: the last pod takes the slot
            l = lists[int(self.pod_node[i])]
            l[l.index(i)] = l[-1]
            l.pop()
        return lists

    def rows(self):
        return rows_of(self.nodes, self.pods, self.node_lists(), self.node_over, self.pod_over)

    def pod_flags(self):
        return pod_rows_by_id(self.pods, self.pod_over)["flags"]

    def load(self, backend) -> None:
        backend.clear()
        if len(self.nodes):
            backend.add_nodes(self.nodes)
        if len(self.pods):
            ids = backend.add_pods(abi.PodTable(self.pods), np.arange(len(self.pods), dtype=np.int32), self.pod_node)
            assert ids.tolist() == list(range(len(self.pods)))
        for i in self.removed:
            backend.remove_pod(int(i))


def _nodes(n, cpu=4000, mem=16 * GI):
    out = abi.empty_nodes(n)
    out["alloc_milli_cpu"], out["alloc_memory"], out["alloc_pods"] = cpu, mem, 1 << 20
    out["name_id"] = np.arange(n)
    return out


def _pods(cpu, mem, flags=0):
    cpu = np.atleast_1d(np.asarray(cpu, np.int64))
    p = abi.empty_pods(len(cpu))
    p["req_milli_cpu"] = p["score_milli_cpu"] = cpu
    p["req_memory"] = p["score_memory"] = mem
    p["flags"] = flags
    return p


def _upod(cpu=0, mem_milli=0, gpu=0, flags=abi.CA_UPOD_MOVABLE, deletion_ns=0, grace_s=0):
    r = np.zeros(1, abi.UTIL_POD_DTYPE)
    r["req_milli"][0] = (cpu, mem_milli, gpu)
    r["flags"], r["deletion_ns"], r["grace_s"] = flags, deletion_ns, grace_s
    return r


def _unode(cpu=0, mem_milli=0, gpu=0, flags=HAS):
    r = np.zeros(1, abi.UTIL_NODE_DTYPE)
    r["alloc_milli"][0] = (cpu, mem_milli, gpu)
    r["flags"] = flags
    return r


def _random(name, seed, n_nodes, counts, **kw) -> Case:
    """n_nodes nodes of mixed sizes, counts[i] pods on node i (ids dealt out in shuffled order),
    10% DaemonSet pods: about half of the nodes end below 0.5."""
    rng = np.random.default_rng(seed)
    nodes = _nodes(n_nodes)
    if n_nodes:
        nodes["alloc_milli_cpu"] = rng.choice([4000, 8000, 16000], n_nodes)
        nodes["alloc_memory"] = rng.choice([16, 32, 64], n_nodes) * GI
    pod_node = np.repeat(np.arange(n_nodes, dtype=np.int32), counts)
    rng.shuffle(pod_node)
    P = len(pod_node)
    per = np.maximum(np.asarray(counts)[pod_node], 1) if P else np.zeros(0, np.int64)
    share = rng.uniform(0.2, 1.8, P)                            # of an even split of the node's cpu / memory
    cpu = (nodes["alloc_milli_cpu"][pod_node] * share / (2 * per)).astype(np.int64) if P else np.zeros(0, np.int64)
    mem = ((nodes["alloc_memory"][pod_node] * rng.uniform(0.2, 1.8, P) / (2 * per)).astype(np.int64) // MI * MI
           if P else np.zeros(0, np.int64))
    flags = np.where(rng.random(P) < 0.1, abi.CA_POD_DAEMONSET, 0).astype(np.uint32)
    return Case(name, nodes, _pods(cpu, mem, flags), pod_node, **kw)


def _over_rows(c: Case, ids, seed=3):
    """Override rows for `ids`: other requests, and every flag kind."""
    rng = np.random.default_rng(seed)
    rows = np.zeros(len(ids), abi.UTIL_POD_DTYPE)
    rows["req_milli"][:, 0] = rng.choice([10, 100, 700], len(ids))
    rows["req_milli"][:, 1] = rng.choice([64, 512], len(ids)) * MI * 1000
    rows["flags"] = rng.choice([abi.CA_UPOD_MOVABLE, abi.CA_UPOD_MIRROR, abi.CA_UPOD_DAEMONSET, 0,
                                abi.CA_UPOD_MOVABLE | abi.CA_UPOD_DELETED, abi.CA_UPOD_BLOCKING], len(ids))
    rows["deletion_ns"] = c.now_ns - rng.choice([0, 100], len(ids)) * 10**9
    rows["grace_s"] = 30
    return np.asarray(ids, np.int32), rows


def _edges() -> Case:
    """One node per numeric or row edge; every pod has an override or is a DaemonSet default."""
    nodes = _nodes(16, cpu=1000, mem=GI)
    nodes["alloc_milli_cpu"][3] = 2**53 + 1
    pods, where, po, claims = [], [], [], {}

    def pod(node, rec, over=None):
        pods.append(rec)
        where.append(node)
        if over is not None:
            po.append((len(pods) - 1, over))

    big = 1 << 61
    pod(0, _pods(0, 0), _upod(big, big))                        # node 0: sums of 2^62 against 2^62 + 2^61
    pod(0, _pods(0, 0), _upod(big, big))
    pod(1, _pods(1000, GI, abi.CA_POD_DAEMONSET))               # node 1: DaemonSet share == allocatable
    pod(1, _pods(10, MI))                                       #   skip_ds: 10 / 0 -> +inf
    pod(2, _pods(1000, GI, abi.CA_POD_DAEMONSET))               # node 2: the same alone: 0 / 0 -> NaN; empty
    pod(3, _pods(2**52, 0))                                     # node 3: allocatable 2^53 + 1 rounds in float64
    pod(4, _pods(500, 0))                                       # node 4: exactly the threshold 0.5
    pod(5, _pods(0, 0), _upod(600, 0, flags=abi.CA_UPOD_MOVABLE | abi.CA_UPOD_DELETED,
                              deletion_ns=NOW - 60 * 10**9, grace_s=30))       # deletion + grace + 30 s == now: counted
    pod(6, _pods(0, 0), _upod(600, 0, flags=abi.CA_UPOD_MOVABLE | abi.CA_UPOD_DELETED,
                              deletion_ns=NOW - 60 * 10**9 - 1, grace_s=30))   # 1 ns past: long-terminating, dropped
    pod(7, _pods(100, MI), _upod(100, MI * 1000, gpu=4000))     # node 7: GPU config with the resource
    pod(8, _pods(100, MI), _upod(100, MI * 1000, gpu=4000))     # node 8: GPU config without it
    pod(9, _pods(100, MI))                                      # nodes 9-12: absent / zero cpu / memory
    pod(10, _pods(100, MI))
    pod(11, _pods(100, MI))
    pod(12, _pods(100, MI))
    pod(13, _pods(100, MI), _upod(100, MI * 1000, flags=abi.CA_UPOD_BLOCKING))  # node 13: one BLOCKING pod
    pod(13, _pods(100, MI))
    pod(14, _pods(100, MI), _upod(100, MI * 1000, flags=abi.CA_UPOD_MIRROR))     # node 14: a mirror pod, not movable
    no = [(0, _unode((1 << 62) + big, (1 << 62) + big)),
          (7, _unode(1000, GI * 1000, 8000, HAS | abi.CA_UNODE_GPU_CONFIG | abi.CA_UNODE_HAS_GPU)),
          (8, _unode(1000, GI * 1000, 0, HAS | abi.CA_UNODE_GPU_CONFIG)),
          (9, _unode(0, GI * 1000, 0, abi.CA_UNODE_HAS_MEM)), (10, _unode(1000, 0, 0, abi.CA_UNODE_HAS_CPU)),
          (11, _unode(0, GI * 1000)), (12, _unode(1000, 0))]
    claims = dict(sum62=0, inf=1, nan=2, rounded=3, equal=4, counted=5, dropped=6, gpu=7, gpu_unready=8,
                  status={9: abi.CA_UTIL_NO_CPU, 10: abi.CA_UTIL_NO_MEM, 11: abi.CA_UTIL_ZERO_CPU,
                          12: abi.CA_UTIL_ZERO_MEM}, blocked=13, empty=[2, 14, 15])
    return Case("edges", nodes, np.concatenate(pods), np.array(where, np.int32),
                node_over=(np.array([k for k, _ in no], np.int32), np.concatenate([r for _, r in no])),
                pod_over=(np.array([k for k, _ in po], np.int32), np.concatenate([r for _, r in po])),
                gpu_thr=0.6, claims=claims)


def _build() -> dict:
    cases = [Case("n_0", _nodes(0), _pods([], 0), np.zeros(0, np.int32)),
             Case("n_1_p_0", _nodes(1), _pods([], 0), np.zeros(0, np.int32))]
    for k, n in enumerate((63, 64, 65, 255, 256, 257, 1023, 1024, 1025)):
        rng = np.random.default_rng(100 + k)
        cases.append(_random(f"n_{n}", 200 + k, n, rng.integers(0, 7, n)))
    # atomic contention on one node, and the pod counts around the table form's 16-lane segment
    cases.append(_random("pods_per_node", 7, 10, [0, 1, 15, 16, 17, 255, 256, 257, 3, 2]))
    for P in (65535, 65536, 65537):                              # the ChunkVec chunk edge of the pod -> node staging
        counts = np.full(300, P // 300)
        counts[:P - counts.sum()] += 1
        cases.append(_random(f"p_{P}", P, 300, counts))
    c = _random("detached", 11, 70, np.full(70, 6))
    c.removed = list(range(0, len(c.pods), 3)) + [len(c.pods) - 1]
    cases.append(c)
    c = _random("over_first_last", 12, 70, np.full(70, 5))
    c.pod_over = _over_rows(c, [0, len(c.pods) - 1])
    cases.append(c)
    c = _random("over_all", 13, 300, np.full(300, 4))
    c.pod_over = _over_rows(c, np.arange(len(c.pods)))
    cases.append(c)
    c = _random("over_detached", 14, 40, np.full(40, 4))
    c.removed = [5, 77]
    c.pod_over = _over_rows(c, [5, 6, 77])
    cases.append(c)
    c = _random("eligible_none", 15, 65, np.full(65, 3))
    c.eligible = np.zeros(65, np.uint8)
    cases.append(c)
    c = _random("eligible_some", 16, 130, np.full(130, 3))
    c.eligible = (np.arange(130) % 3 != 1).astype(np.uint8)
    cases.append(c)
    e = _edges()
    cases.append(e)
    # the same cluster one ulp under a raised threshold: node 4 (0.5) is now below
    import dataclasses
    cases.append(dataclasses.replace(e, name="edges_ulp", thr=float(np.nextafter(0.5, 1.0))))
    return {c.name: c for c in cases}


@lru_cache(maxsize=None)
def all_cases() -> dict:
    return _build()


CASE_NAMES = ["n_0", "n_1_p_0", "n_63", "n_64", "n_65", "n_255", "n_256", "n_257", "n_1023", "n_1024", "n_1025",
              "pods_per_node", "p_65535", "p_65536", "p_65537", "detached", "over_first_last", "over_all",
              "over_detached", "eligible_none", "eligible_some", "edges", "edges_ulp"]


def case(name: str) -> Case:
    return all_cases()[name]


@lru_cache(maxsize=None)
def expected(name: str, skip_ds: bool, skip_mirror: bool):
    """(info rows, drain) of the case from the CPU oracle on rows_of: computed once per case."""
    import pyoracle
    c = case(name)
    un, off, up = c.rows()
    info = pyoracle.node_utilization(un, off, up, skip_ds, skip_mirror, c.now_ns)
    info.setflags(write=False)
    return info, drain_of(off, up)
