"""Resident pod columns (ca_mirror_fetch_pod_columns, the _resident scale-down calls): the
column rule stated in numpy, and cases placed at the edges of the kernels that read the columns.

expected_columns is the whole rule: a pod's node is the position of the list it is in, its slot
its index there.  The cases are utilgen.Case clusters (so utilgen.rows_of / candidates_of are the
expected side) built so that the candidates' pod counts, the slot table's size and the number of
candidates land on the widths the move-list kernels are built around: a wave (64), a workgroup
of the pod kernels (256), the offset scan's workgroup (1024) and the compaction's tile (2048).

Every case carries removals.  RemovePod swaps the node's last pod into the hole, so on a node
that lost its first pod NodeInfo.Pods order is not id order: a kernel that lists a candidate's
pods by ascending id fails wherever claims["unordered"] names a candidate.  The claim is None
only where the edge itself rules it out (no candidate, or a slot table of at most one entry).
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import utilgen
from autoscaler_amd import abi
from utilgen import Case, MI

TILE = 2048


def expected_columns(node_lists, n_pods: int):
    """(node, slot) int32 per mirror pod id from the nodes' pod lists in NodeInfo.Pods order;
    (-1, -1) for a pod on no node (the slot is meaningless there)."""
    node = np.full(n_pods, -1, np.int32)
    slot = np.full(n_pods, -1, np.int32)
    for x, l in enumerate(node_lists):
        for s, pid in enumerate(l):
            node[pid], slot[pid] = x, s
    return node, slot


def step_with_reorder(s, backends, rng) -> str:
    """One step of the sequence, or (at depth 0, one time in eight) a reorder of the nodes."""
    if s.model.depth == 0 and s.model.node_count() > 1 and rng.random() < 0.125:
        order = list(range(s.model.node_count()))
        rng.shuffle(order)
        s.model.nodes = [s.model.nodes[k] for k in order]
        for b in backends:
            b.reorder_nodes(np.array(order, np.int32))
        s.step += 1
        s.op = "reorder"
        return "reorder"
    return s.next(backends)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
HOT, IDLE = -1, 0                                 # a node's kind: one pod above the threshold / no pod at all


def _cluster(name: str, kinds, pod_over_fn=None, **claims) -> Case:
    """kinds[i]: HOT (one 3000m pod on a 4000m node: not below 0.5), IDLE (no pod: class empty),
    or k >= 1: a candidate that ends with k 1m pods.  A candidate with k >= 2 is given k + 1 pods
    and loses its first, so its list starts with its highest id."""
    n = len(kinds)
    nodes = utilgen._nodes(n)
    cpu, where, removed, nxt = [], [], [], 0
    for x, k in enumerate(kinds):
        if k == HOT:
            cpu.append(3000); where.append(x); nxt += 1
            continue
        extra = 1 if k >= 2 else 0
        if extra:
            removed.append(nxt)
        cpu += [1] * (k + extra)
        where += [x] * (k + extra)
        nxt += k + extra
    if not removed and nxt:                      # (every case carries removals: a hot node's twin, added last)
        hot = next((x for x, k in enumerate(kinds) if k == HOT), None)
        if hot is not None:
            cpu.append(1); where.append(hot); removed.append(nxt); nxt += 1
    c = Case(name, nodes, utilgen._pods(cpu, MI), np.array(where, np.int32), removed=removed)
    if pod_over_fn is not None:
        c.pod_over = pod_over_fn(c)
    cand = [x for x, k in enumerate(kinds) if k >= 1]
    c.claims = dict(cand=cand, cand_counts=[kinds[x] for x in cand], table_total=sum(kinds[x] for x in cand),
                    unordered=next((x for x in cand if kinds[x] >= 2), None))
    c.claims.update(claims)
    return c


def _split(total: int, per: int = 256) -> list:
    """Candidate sizes adding up to `total`, `per` each and the rest on the last."""
    out = [per] * (total // per)
    if total % per:
        out.append(total % per)
    return out


def _blocking_or_ds(c: Case):
    """Node 1's pods all blocking or DaemonSet (its move list is empty, its table span is not);
    node 2 keeps a movable pod between two blocking ones."""
    lists = c.node_lists()
    ids, rows = [], []
    for k, pid in enumerate(lists[1]):
        ids.append(pid)
        rows.append(utilgen._upod(1, MI * 1000, flags=abi.CA_UPOD_BLOCKING if k % 2 == 0 else abi.CA_UPOD_DAEMONSET))
    for pid in (lists[2][0], lists[2][-1]):
        ids.append(pid)
        rows.append(utilgen._upod(1, MI * 1000, flags=abi.CA_UPOD_BLOCKING))
    order = np.argsort(ids)
    return np.array(ids, np.int32)[order], np.concatenate(rows)[order]


def _with_removals(c: Case, every: int) -> Case:
    """utilgen's random clusters with the first pod of every `every`-th node removed."""
    lists = c.node_lists()
    c.removed = list(c.removed) + [l[0] for l in lists[::every] if len(l) >= 3 and l[0] not in c.removed]
    c.claims = dict(unordered_any=True)
    return c


def _build() -> dict:
    cases = []
    # the candidates' pod counts around a wave and a workgroup; hot nodes before the first and after the last
    cases.append(_cluster("cand_counts", [HOT, 1, 63, HOT, 64, 65, IDLE, 255, 256, 257, HOT]))
    for total in (0, 1, 2047, 2048, 2049, 4097):                 # the slot table around one and two tiles
        kinds = [HOT] + _split(total) + [HOT, IDLE]
        cases.append(_cluster(f"table_{total}", kinds))
    for k in (0, 1, 1023, 1024, 1025):                           # the offset scan's workgroup
        cases.append(_cluster(f"cands_{k}", [HOT] + [2] * k + [HOT]))
    cases.append(_cluster("blocking_or_ds", [HOT, 5, 4, 3, HOT], _blocking_or_ds, empty_list=1, unordered=3))
    for P in (65535, 65536, 65537):                              # a chunk of the host records; ids past 2^16
        counts = np.full(300, P // 300)
        counts[:P - counts.sum()] += 1
        cases.append(_with_removals(utilgen._random(f"ids_{P}", P + 1, 300, counts), 2))
    c = _with_removals(utilgen._random("rows_first_last", 21, 70, np.full(70, 5)), 1)
    c.pod_over = utilgen._over_rows(c, [0, len(c.pods) - 1])
    cases.append(c)
    c = _with_removals(utilgen._random("rows_all", 22, 200, np.full(200, 4)), 1)
    c.pod_over = utilgen._over_rows(c, np.arange(len(c.pods)))
    cases.append(c)
    c = _with_removals(utilgen._random("rows_detached", 23, 40, np.full(40, 4)), 1)
    c.removed += [i for i in (5, 77) if i not in c.removed]
    c.pod_over = utilgen._over_rows(c, [5, 6, 77])
    c.claims["detached_rows"] = [5, 77]
    cases.append(c)
    return {c.name: c for c in cases}


@lru_cache(maxsize=None)
def all_cases() -> dict:
    return _build()


CASE_NAMES = (["cand_counts"] + [f"table_{t}" for t in (0, 1, 2047, 2048, 2049, 4097)] +
              [f"cands_{k}" for k in (0, 1, 1023, 1024, 1025)] + ["blocking_or_ds"] +
              [f"ids_{p}" for p in (65535, 65536, 65537)] + ["rows_first_last", "rows_all", "rows_detached"])


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
    return info, utilgen.drain_of(off, up)


def split_overrides(c: Case):
    """The case's overrides sent three ways: [(resident rows, per-call rows)], each (ids, rows)
    or None — all resident, all per call, and split, where the resident side also holds a
    conflicting row for every per-call id (the per-call row has to win)."""
    po = c.pod_over
    if po is None or not len(po[0]):
        return [(None, None)]
    ids, rows = po
    half = np.arange(len(ids)) % 2 == 0
    wrong = rows.copy()
    wrong["req_milli"][:, 0] += 13
    wrong["flags"] = np.where(rows["flags"] & abi.CA_UPOD_MOVABLE, abi.CA_UPOD_BLOCKING, abi.CA_UPOD_MOVABLE)
    resident = rows.copy()
    resident[~half] = wrong[~half]
    return [((ids, rows), None), (None, (ids, rows)), ((ids, resident), (ids[~half], rows[~half]))]
