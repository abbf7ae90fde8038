"""The reference for ca_try_schedule_pods: HintingSimulator.TrySchedulePods
(hinting_simulator.go:58-125) written over the three primitives that pyoracle.OracleState
and native.Mirror expose with the same signatures (check_predicates, fits_any_node with a
match, add_pods), with the similar-pods cache and its cap per owner the way
or_filter_out_schedulable applies it; plus the masks and cases the tests share."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from autoscaler_amd import abi

MAX_PODS_PER_OWNER = 10                      # similar_pods.go:53


@dataclass
class TryRef:
    node: np.ndarray
    pod_id: np.ndarray
    hints: np.ndarray
    hint_ok: np.ndarray
    last_index: int
    evals: int
    n_overflowing: int
    placed: int
    tried: int


def match_pos(match, pos: int) -> bool:
    """nodeMatches as data (oracle match_pos): `exclude` applies to every kind."""
    if match is None:
        return True
    kind, lo, hi, exclude, mask = match
    if pos == exclude:
        return False
    if kind == abi.CA_MATCH_RANGE:
        return lo <= pos < hi
    if kind == abi.CA_MATCH_MASK:
        return bool(mask[pos])
    return True


def try_schedule_ref(backend, table, order, match, brk, class_owner, hints, L) -> TryRef:
    order = np.arange(len(table.pods), dtype=np.int32) if order is None else np.asarray(order, np.int32)
    n = len(order)
    n_nodes = backend.node_count()
    cls, flags = table.pods["similar_class"], table.pods["flags"]
    node = np.full(n, -1, np.int32)
    pod_id = np.full(n, -1, np.int32)
    hout = np.full(n, -1, np.int32) if hints is None else np.array(hints, np.int32, copy=True)
    hok = np.zeros(n, np.uint8)
    marked, over, owner_cnt = set(), set(), {}
    evals = placed = tried = 0
    for k in range(n):
        i = int(order[k])
        tried = k + 1
        nd = -1
        h = int(hout[k])
        if h >= 0:                                                   # findNodeWithHints (:91-108)
            typ = backend.check_predicates(table, i, h)[0]
            if h < n_nodes and not (int(flags[i]) & abi.CA_POD_PREFILTER_FAIL):
                evals += 1                                           # the filters ran (oracle check_pred)
            if typ == abi.CA_PRED_OK:
                hok[k] = 1                                           # Hints.Set (:95)
                if match_pos(match, h):                              # isNodeAcceptable (:102)
                    nd = h
        if nd < 0:                                                   # findNode (:110-125)
            c = int(cls[i])
            if not (c >= 0 and c in marked):                         # IsSimilarUnschedulable
                got, l2, _, ev = backend.fits_any_node(table, i, match, L)
                evals += ev
                if got >= 0:
                    nd, L = got, l2
                elif c >= 0 and not (int(flags[i]) & abi.CA_POD_DAEMONSET):   # SetUnschedulable
                    o = int(class_owner[c]) if class_owner is not None else -1
                    if o < 0:
                        marked.add(c)
                    elif owner_cnt.get(o, 0) >= MAX_PODS_PER_OWNER:
                        over.add(o)
                    else:
                        marked.add(c)
                        owner_cnt[o] = owner_cnt.get(o, 0) + 1
        if nd >= 0:                                                  # AddPod (:77-82), Hints.Set (:123)
            pod_id[k] = int(backend.add_pods(table, [i], [nd])[0])
            node[k] = nd
            hout[k] = nd
            placed += 1
        elif brk:                                                    # :83-85
            break
    return TryRef(node, pod_id, hout, hok, int(L), int(evals), len(over), placed, tried)


def eq_try(got, ref: TryRef, what="") -> None:
    """Every output of Mirror.try_schedule_pods against the reference."""
    assert np.array_equal(got.node, ref.node), (what, np.nonzero(got.node != ref.node)[0][:10])
    assert np.array_equal(got.pod_id, ref.pod_id), what
    assert np.array_equal(got.hints, ref.hints), (what, np.nonzero(got.hints != ref.hints)[0][:10])
    assert np.array_equal(got.hint_ok, ref.hint_ok), (what, np.nonzero(got.hint_ok != ref.hint_ok)[0][:10])
    assert (got.placed, got.tried, got.last_index, got.evals, got.n_overflowing) == \
           (ref.placed, ref.tried, ref.last_index, ref.evals, ref.n_overflowing), what


# ---- the masks of the GPU cases (n = node count, w = the FilterWorkload, L = lastIndex) ----
def hot_hint(w) -> int:
    """The node most pods are hinted to."""
    h = w.hints[w.hints >= 0]
    return int(np.bincount(h).argmax()) if len(h) else 0


def _mask(n, on):
    m = np.zeros(n, np.uint8)
    m[[p for p in on if 0 <= p < n]] = 1
    return m


def make_match(name: str, w, L: int):
    n = len(w.nodes)
    M = abi.CA_MATCH_MASK
    if name == "all":                       # plain ALL: no acc words
        return None
    if name == "ones":
        return (M, 0, 0, -1, np.ones(n, np.uint8))
    if name == "zeros":
        return (M, 0, 0, -1, np.zeros(n, np.uint8))
    if name == "one":                       # the node with the most free cpu (so that pods land on it)
        used = np.bincount(w.pod_node, weights=w.table.pods["req_milli_cpu"], minlength=n)
        return (M, 0, 0, -1, _mask(n, [int(np.argmax(w.nodes["alloc_milli_cpu"] - used))]))
    if name == "altwords":                  # whole words alternately off
        return (M, 0, 0, -1, (((np.arange(n) >> 6) & 1) == 0).astype(np.uint8))
    if name == "edges":                     # positions 63, 64 and the last node
        return (M, 0, 0, -1, _mask(n, [63, 64, n - 1]))
    if name == "range":                     # straddles the first word boundary that exists
        return (abi.CA_MATCH_RANGE, min(50, n // 3), min(max(n - 3, 1), 150), -1, None)
    if name == "excl_last":
        return (abi.CA_MATCH_ALL, 0, 0, L % n, None)
    if name == "excl_hot":
        return (abi.CA_MATCH_ALL, 0, 0, hot_hint(w), None)
    if name == "half":                      # every other node
        return (M, 0, 0, -1, (np.arange(n) & 1).astype(np.uint8))
    raise KeyError(name)


MASKS = ["ones", "zeros", "one", "altwords", "edges", "range", "excl_last", "excl_hot"]


# ---- the shared cases ----------------------------------------------------------------------
L0 = 3                                      # lastIndex the cases start from

WORKLOADS = {
    # a ring shorter than one word; the word edges; a tight cluster (pods fail early, static
    # classes from the taint universe); a loose large one (long runs, many placements)
    "n37": dict(n_nodes=37, pods_per_node=10, n_pending=600, hint_frac=0.4, util_low=(0.1, 0.3), util_high=(0.3, 0.5)),
    "n64": dict(n_nodes=64, pods_per_node=20, n_pending=800, hint_frac=1.0, util_low=(0.3, 0.5), util_high=(0.5, 0.7)),
    "n65": dict(n_nodes=65, pods_per_node=20, n_pending=800, hint_frac=0.0, util_low=(0.3, 0.5), util_high=(0.5, 0.7)),
    "n300": dict(n_nodes=300, pods_per_node=20, n_pending=3000, hint_frac=0.4, taints=True, util_low=(0.3, 0.5),
                 util_high=(0.5, 0.7)),
    "n2000": dict(n_nodes=2000, pods_per_node=20, n_pending=6000, hint_frac=0.4, util_low=(0.7, 0.85),
                  util_high=(0.85, 0.95)),
}

# every mask on every workload, but for the one-word rings, where "altwords" is "ones" again
CASES = [(wn, mn) for wn in WORKLOADS for mn in MASKS if not (mn == "altwords" and wn in ("n37", "n64"))]

_W, _REF = {}, {}


def workload(name: str):
    from autoscaler_amd import workloads as W
    if name == "special":
        return special_workload()
    if name not in _W:
        _W[name] = W.c5_filter(**WORKLOADS[name])
    return _W[name]


def special_workload():
    """A loose 300-node C5 cluster with what c5_filter never generates: Unschedulable nodes
    (every 7th), pods that tolerate them (every 3rd pending record), hints onto Unschedulable
    nodes for both kinds of pod, and PreFilter failures (the break's second stop) at three
    positions of the walk."""
    from autoscaler_amd import workloads as W
    if "special" not in _W:
        w = W.c5_filter(n_nodes=300, pods_per_node=20, n_pending=1200, hint_frac=0.3, util_low=(0.2, 0.4),
                        util_high=(0.4, 0.6))
        n, P = len(w.nodes), len(w.order)
        unsched = np.arange(n) % 7 == 2
        w.nodes["flags"][unsched] |= abi.CA_NODE_UNSCHEDULABLE
        w.pending.pods["flags"][np.arange(len(w.pending.pods)) % 3 == 0] |= abi.CA_POD_TOLERATES_UNSCHED
        k = np.arange(P)
        onto = k % 4 == 1                                    # every 4th position: hinted onto an Unschedulable node
        w.hints[onto] = np.nonzero(unsched)[0][(k[onto] * 5) % int(unsched.sum())]
        for pos in (150, 151, 700):
            w.pending.pods["flags"][w.order[pos]] |= abi.CA_POD_PREFILTER_FAIL
        _W["special"] = w
    return _W["special"]


def ref_case(oracle_cls, wname: str, mname: str, brk: bool) -> TryRef:
    """The reference of one case, computed once per session (read-only for the tests)."""
    from autoscaler_amd import workloads as W
    key = (wname, mname, bool(brk))
    if key not in _REF:
        w = workload(wname)
        o = oracle_cls()
        W.load_filter(o, w)
        _REF[key] = try_schedule_ref(o, w.pending, w.order, make_match(mname, w, L0), brk, w.class_owner, w.hints, L0)
        o.close()
    return _REF[key]
