"""Cases for ca_estimate_plan_groups_missing_pods (filterNodeGroupsByPods on the resident
Estimate lists): every case is ONE pod table shared by all its groups, so a pod has one id in
every group; groups differ in their pod_idx slices and templates.

Most cases use "ranked" pods: pod i requests (top - i) milli cpu and the same memory, so the
Estimate score sort puts it at list position i of any group that holds ranks 0..i, and a missing
pod's list position is known by construction (tests/test_similar_cases.py checks the
construction against the CPU restatement's lists).  Filler groups of one to three pods in front
of a group move its offset to a wanted residue mod 4.

Shared by the CPU test of the cases and the GPU test of the kernels.
"""
import copy
from dataclasses import dataclass, field

import numpy as np

from autoscaler_amd import abi, k8s, native
from estgen import _encode_estimate

GI, MI = 1 << 30, 1 << 20
TILE = native.MISSING_PODS_TILE
RANK_TOP = 4500

T_WIDE = ("wide", 64000, 256 * GI, 110)         # pod-count bound: 110 ranked pods always fit
T_TEN = ("ten", 64000, 256 * GI, 10)
T_MID = ("mid", 8000, 16 * GI, 110)
T_SMALL = ("small", 4000, 8 * GI, 10)


@dataclass
class SimCase:
    name: str
    pods: list
    templates: list                  # [(Node, [])] per group
    groups: list                     # [[Pod]] per group
    index: dict                      # group name -> group index
    required: str
    candidates: list                 # group names, in the order the test passes them
    limits: tuple = (0,)             # max_nodes of the runs, in order; the last one is checked
    built: dict = field(default_factory=dict)        # what the generator claims: name -> missing positions

    def encode(self):
        """(table, templates, group_off, pod_idx)."""
        table, _, tm, off, idx = _encode_estimate([], self.pods, self.templates, self.groups)
        return table, tm, off, idx

    def g(self, name) -> int:
        return self.index[name]


def ranked(n, first=0, prefix="r", top=RANK_TOP):
    """Pods of ranks first .. first + n - 1 (rank 0 requests `top` milli cpu)."""
    return [k8s.build_test_pod(f"{prefix}{first + i}", top - first - i, 64 * MI) for i in range(n)]


def layout(named, fill):
    """named: [(name, pods, template, wanted offset residue mod 4 or None)].  Returns (groups,
    templates, index) with filler groups of pods from `fill` where an offset must move."""
    groups, templates, index, at = [], [], {}, 0
    for name, pods, tmpl, res in named:
        if res is not None and at % 4 != res:
            k = (res - at) % 4
            groups.append(list(fill[:k]))
            templates.append((k8s.build_test_node(*T_WIDE), []))
            at += k
        index[name] = len(groups)
        groups.append(list(pods))
        templates.append((k8s.build_test_node(*tmpl), []))
        at += len(pods)
    return groups, templates, index


def _drop(pods, positions):
    gone = set(positions)
    return [p for i, p in enumerate(pods) if i not in gone]


def tile_case(n, res):
    """A required list of n ids at an offset = res mod 4: its first tile ends after list position
    TILE - res - 1, the b-th after b * TILE - res - 1.  One candidate per single missing position
    (0, the last of a tile, the first of the next, the very last), one missing two positions, a
    superset in another order, and one that shares no pod."""
    req = ranked(n)
    extra = ranked(8, first=n, prefix="x")
    b = max(1, (n + res - 1) // TILE)                                  # the last tile boundary inside the list
    drops = sorted({0, b * TILE - res - 1, b * TILE - res, n - 1} & set(range(n)))
    named = [("req", req, T_WIDE, res)]
    built = {}
    for k, d in enumerate(drops):
        named.append((f"drop{d}", _drop(req, [d]) + extra[:2], T_WIDE, (res + 1 + k) % 4))
        built[f"drop{d}"] = [d]
    named.append(("two", _drop(req, [3, n - 2]), T_WIDE, 3))
    built["two"] = [3, n - 2]
    named.append(("full", extra[:3] + req[::-1], T_WIDE, 2))
    built["full"] = []
    named.append(("none", extra, T_WIDE, 1))
    built["none"] = list(range(n))
    groups, templates, index = layout(named, extra)
    return SimCase(f"tile-{n}-{res}", req + extra, templates, groups, index, "req", [c[0] for c in named[1:]],
                   built=built)


def word_case(n_pods):
    """A pod set of n_pods pods; the required list is all of them but ids 5 and 40.  Candidates
    miss the pod of id 0, 31, 32 or n_pods - 1 (and hold the other three), all, or everything."""
    pods = ranked(n_pods)
    others = {5, 40}
    req = [p for i, p in enumerate(pods) if i not in others]
    pos = {id(p): i for i, p in enumerate(req)}                        # (ranked: list position = order in req)
    named = [("req", req, T_WIDE, 1)]
    built = {}
    for k, m in enumerate((0, 31, 32, n_pods - 1)):
        named.append((f"id{m}", [p for p in req if p is not pods[m]], T_WIDE, (2 + k) % 4))
        built[f"id{m}"] = [pos[id(pods[m])]]
    named.append(("full", pods, T_WIDE, None))
    built["full"] = []
    named.append(("none", [pods[i] for i in sorted(others)], T_WIDE, None))
    built["none"] = list(range(len(req)))
    groups, templates, index = layout(named, [pods[5], pods[40], pods[1]])
    return SimCase(f"word-{n_pods}", pods, templates, groups, index, "req", [c[0] for c in named[1:]], built=built)


STALE_LIMIT = 2


def stale_case():
    """Run unlimited, then with max_nodes = STALE_LIMIT.  `req` and `ten` hold the same 300 ranked
    pods; req's template takes 110 pods a node, ten's takes 10: after the limited run ten's list is
    ranks 0..19, and behind it the buffer still holds ranks 20..299 of the unlimited run — the
    pods req's list has and ten's lacks."""
    pods = ranked(300, top=400)                      # (110 of them fit one 64000m node: the pod count binds)
    extra = ranked(6, first=300, prefix="x", top=400)
    named = [("req", pods, T_WIDE, 3), ("ten", pods, T_TEN, 1), ("same", pods[::-1], T_WIDE, 2),
             ("minus0", pods[1:], T_WIDE, 3), ("none", extra, T_WIDE, None)]
    n_req, n_ten = 110 * STALE_LIMIT, 10 * STALE_LIMIT
    built = {"ten": list(range(n_ten, n_req)), "same": [], "minus0": [0], "none": list(range(n_req))}
    groups, templates, index = layout(named, extra)
    return SimCase("stale", pods + extra, templates, groups, index, "req", [c[0] for c in named[1:]],
                   limits=(0, STALE_LIMIT), built=built)


def slots_case():
    """The slot rules: the required group among the candidates, a group listed twice, a group
    without pods, a group whose pods fit no node (n_scheduled 0)."""
    req = ranked(40)
    extra = ranked(5, first=40, prefix="x")
    huge = [k8s.build_test_pod(f"huge{i}", 900000, 64 * MI) for i in range(2)]
    named = [("req", req, T_WIDE, 1), ("sub", _drop(req, [7]), T_WIDE, 2), ("empty", [], T_WIDE, None),
             ("huge", huge, T_WIDE, None), ("full", req + extra, T_WIDE, 3), ("none", extra, T_WIDE, None)]
    built = {"req": [], "sub": [7], "empty": list(range(40)), "huge": list(range(40)), "full": [],
             "none": list(range(40))}
    groups, templates, index = layout(named, extra)
    return SimCase("slots", req + extra + huge, templates, groups, index, "req",
                   ["req", "sub", "sub", "empty", "huge", "full", "none", "req", "sub"], built=built)


def prefix_case():
    """The prefix protocol: `cut` holds a pod the kernels do not cover (a DoNotSchedule spread
    constraint): CA_EUNSUPPORTED, and `after` is CA_ENOTRUN — both count as n_scheduled 0."""
    req = ranked(10)
    extra = ranked(4, first=10, prefix="x")
    bad = k8s.build_test_pod("spread", 300, 64 * MI)
    bad.topology_spread.append(k8s.TopologySpreadConstraint(1, "kubernetes.io/hostname", "DoNotSchedule", {"app": "x"}))
    named = [("req", req, T_WIDE, 2), ("full", req + extra, T_WIDE, None), ("one", req[1:], T_WIDE, None),
             ("none", extra, T_WIDE, None), ("cut", [req[0], bad], T_WIDE, None), ("after", req, T_WIDE, None)]
    built = {"full": [], "one": [0], "none": list(range(10)), "cut": list(range(10)), "after": list(range(10))}
    groups, templates, index = layout(named, extra)
    return SimCase("prefix", req + extra + [bad], templates, groups, index, "req", [c[0] for c in named[1:]],
                   built=built)


def many_case(n_groups=300):
    """More candidate groups than a block has lanes: subsets of 12 ranked pods by bit mask."""
    pods = ranked(12)
    req = pods[:4]
    named, built = [("req", req, T_WIDE, 1)], {}
    for g in range(n_groups):
        mask = (g * 37 + 1) & 0xFFF
        named.append((f"c{g}", [p for i, p in enumerate(pods) if mask >> i & 1], T_WIDE, None))
        built[f"c{g}"] = [i for i in range(4) if not mask >> i & 1]
    groups, templates, index = layout(named, pods)
    return SimCase("many", pods, templates, groups, index, "req", [c[0] for c in named[1:]], built=built)


SHAPES = {"s2": k8s.build_test_pod("s2", 500, 1 * GI), "s3": k8s.build_test_pod("s3", 250, 512 * MI),
          "s1": k8s.build_test_pod("s1", 1000, 2 * GI)}


def shapes_case():
    """Pods of three shapes, deep-copied (uniform score classes: the run may take the decoupled
    Go order); the list order among equal pods is Go's, so nothing is claimed by construction."""
    by = {}
    for s, n in (("s2", 120), ("s3", 60), ("s1", 30)):
        by[s] = []
        for r in range(n):
            q = copy.deepcopy(SHAPES[s])
            q.name = q.uid = f"{s}-{r}"
            by[s].append(q)
    pods = [p for s in by for p in by[s]]
    req = by["s2"][:80] + by["s3"][:40]
    named = [("req", req, T_MID, 1), ("full", by["s3"] + by["s2"], T_MID, 2),
             ("one", [p for p in req if p is not by["s2"][11]], T_MID, 3),
             ("few", by["s2"][40:] + by["s3"][::2], T_SMALL, None), ("none", by["s1"], T_MID, None)]
    groups, templates, index = layout(named, by["s1"])
    return SimCase("shapes", pods, templates, groups, index, "req", [c[0] for c in named[1:]])


TILE_CASES = [(TILE - 1, 1), (TILE, 2), (TILE + 1, 3), (2 * TILE + 3, 1)]
WORD_SIZES = [64, 65, 95]


def all_cases():
    return ([tile_case(n, r) for n, r in TILE_CASES] + [word_case(n) for n in WORD_SIZES] +
            [stale_case(), slots_case(), prefix_case(), many_case(), shapes_case()])


# -- the expected values, from the CPU restatement's lists ------------------------------------
def oracle_lists(oracle_state, enc, max_nodes):
    """(results, per-group scheduled lists; a group whose status is not CA_OK has an empty one)."""
    table, tm, off, idx = enc
    ro = oracle_state.estimate(table, off, idx, tm, max_nodes, 0)
    lists = []
    for g in range(len(tm)):
        ok = int(ro.results[g]["status"]) == abi.CA_OK
        a, n = int(off[g]), int(ro.results[g]["n_scheduled"]) if ok else 0
        lists.append(ro.sched_pod[a:a + n].tolist())
    return ro, lists


def missing_positions(lists, req, cand):
    have = set(lists[cand])
    return [i for i, p in enumerate(lists[req]) if p not in have]


def expected(lists, req, cands):
    """(n_missing, first_missing) per candidate slot."""
    miss = [missing_positions(lists, req, c) for c in cands]
    return np.array([len(m) for m in miss], np.int32), np.array([m[0] if m else -1 for m in miss], np.int32)
