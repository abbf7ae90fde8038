"""Shared Go-order sorts (decoupled Estimate): groups with element-wise equal pod lists whose
templates rank the podset's score classes alike get their ids from one k_pdq_sort workgroup,
the first such group's.  Checked against the CPU restatement and against one sort per group
(CASIM_SORT_SHARE=0, byte for byte) in every output mode, over consecutive runs of a plan
(the ready flags' epochs) and a second plan on the same mirror.

The podsets are test_gpu_table_chain's: uniform, a few deep-copied shapes with no score tie
across shapes on any template used here, so every plan stays decoupled.
"""
import copy

import numpy as np
import pytest

from autoscaler_amd import k8s, native
from estgen import _encode_estimate
import test_gpu_table_chain as tc

pytestmark = pytest.mark.gpu

GI = tc.GI
T_MID, T_SMALL, T_WIDE = tc.T_MID, tc.T_SMALL, tc.T_WIDE    # MID and SMALL rank alike (1 : 2); WIDE is 1 : 4
T_DOUBLE = ("double", 16000, 32 * GI, 110)                   # both allocatables of T_MID doubled
T_RENAMED = ("another-name", 8000, 16 * GI, 110)

# port (400m, 768 Mi) ranks below mb on the 1 : 2 templates and above it on T_WIDE
BASE = [("s1", 30), ("mb", 25), ("port", 6), ("s3", 40), ("bottom", 21)]
OTHER = [("top", 7), ("s2", 33), ("s3", 18)]
THIRD = [("s2", 33), ("bottom", 50), ("ma", 11)]


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


class Pods:
    """Deep copies of tc.SHAPES, two more of each than the longest list asks for."""

    def __init__(self, *specs):
        need = {}
        for grp in specs:
            for s, n in grp:
                need[s] = max(need.get(s, 0), n)
        self.all, self.by_shape = [], {}
        for s, n in need.items():
            self.by_shape[s] = []
            for r in range(n + 2):
                q = copy.deepcopy(tc.SHAPES[s])
                q.name = q.uid = f"{s}-{r}"
                self.by_shape[s].append(q)
                self.all.append(q)

    def interleaved(self, spec):
        lists = [self.by_shape[s][:n] for s, n in spec]
        out = []
        for i in range(max(len(x) for x in lists)):
            out.extend(x[i] for x in lists if i < len(x))
        return out


def _tmpl(t, daemonset=()):
    node, _ = tc._template(*t)
    return (node, list(daemonset))


def _run_plan(plan, max_nodes, L0):
    """Three consecutive runs of every output mode; each run's outputs."""
    outs = []
    for _ in range(3):
        g = plan.run(max_nodes, L0, want_nodes=True)
        st = plan.stats()
        p = plan.run(max_nodes, L0, want_nodes=False)                  # 32-bit ids, published
        d = plan.run(max_nodes, L0, device_results=True)               # left in device memory
        d.sched_pod = plan.fetch()
        h = plan.run_u16(max_nodes, L0)                                # 16-bit ids, published
        outs.append((st, {"nodes": g, "host32": p, "device": d, "u16": h}))
    return outs


def _check(oracle, monkeypatch, pods, templates, groups, sorts, max_nodes=0, L0=0):
    table, node_recs, tm, off, pod_idx = _encode_estimate([], pods, templates, groups)
    o, m = oracle.OracleState(), native.Mirror(0)
    for b in (o, m):
        b.clear()
    ro = o.estimate(table, off, pod_idx, tm, max_nodes, L0)
    G = len(groups)
    raw = {}
    for share in ("1", "0"):
        monkeypatch.setenv("CASIM_SORT_SHARE", share)                  # (read when the plan is created)
        with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
            runs = _run_plan(plan, max_nodes, L0)
            with native.EstimatePlan(m, table, off, pod_idx, tm) as second:   # a second plan, same mirror
                runs += _run_plan(second, max_nodes, L0)[:1]
                runs += _run_plan(plan, max_nodes, L0)[:1]             # ... and the first one again
        for r, (st, modes) in enumerate(runs):
            what = (share, r, max_nodes)
            assert st["decoupled"], what
            assert st["sorts"] == (sorts if share == "1" else G), (what, st)
            for mode, g in modes.items():
                tc._same(ro, g, off, G, what + (mode,), nodes=mode == "nodes", u16=mode == "u16")
                key = (r, mode)
                blob = (g.results.tobytes(), np.asarray(g.sched_pod).tobytes(),
                        g.sched_node.tobytes() if mode == "nodes" else b"", g.last_index)
                if share == "1":
                    raw[key] = blob
                else:
                    assert raw[key] == blob, what + (mode, "share off differs")
    m.close()
    return ro


LIMITS = [0, 3]


@pytest.mark.parametrize("variant", ["last_pod", "swapped"])
@pytest.mark.parametrize("max_nodes", LIMITS)
def test_equal_lists_share_others_do_not(max_nodes, variant, oracle, monkeypatch):
    """Groups 0 and 2 (not adjacent): same list, same template — one sort.  Group 1: the same
    list on the 1 : 4 template, where `port` and `mb` swap ranks — its own sort.  Group 3: a
    list of the same length that differs in its last pod only, or by two swapped positions
    holding pods of one shape (the same rank sequence, other ids) — its own sort."""
    ps = Pods(BASE)
    base = ps.interleaved(BASE)
    other = list(base)
    if variant == "last_pod":
        shape = other[-1].name.rsplit("-", 1)[0]
        spare = ps.by_shape[shape][-1]
        assert all(q is not spare for q in base)
        other[-1] = spare
    else:
        i, j = [k for k, q in enumerate(other) if q.name.startswith("s3-")][3:20:16]
        other[i], other[j] = other[j], other[i]
    assert len(other) == len(base) and other != base
    tm = [_tmpl(T_MID), _tmpl(T_WIDE), _tmpl(T_MID), _tmpl(T_MID)]
    _check(oracle, monkeypatch, ps.all, tm, [base, base, base, other], 3, max_nodes)


@pytest.mark.parametrize("max_nodes", LIMITS)
def test_templates_that_sort_alike(max_nodes, oracle, monkeypatch):
    """One list on four templates that rank every class alike: DaemonSet pods on one (used_*
    only), another name, both allocatables doubled.  One sort; the chains stay per group and
    the group with less free space needs more nodes."""
    ps = Pods(BASE)
    base = ps.interleaved(BASE)
    ds = k8s.build_test_pod("ds", 4000, 6 * GI)
    tm = [_tmpl(T_MID), _tmpl(T_MID, [ds]), _tmpl(T_RENAMED), _tmpl(T_DOUBLE)]
    ro = _check(oracle, monkeypatch, ps.all, tm, [base] * 4, 1, max_nodes)
    if max_nodes == 0:
        n = [int(r["node_count"]) for r in ro.results]
        assert n[1] > n[0] == n[2] > n[3], n


@pytest.mark.parametrize("max_nodes", LIMITS)
def test_class_of_one_between_classes(max_nodes, oracle, monkeypatch):
    """Nine groups (the heavy-first split) in three sort classes: a group that shares with
    nobody between two classes whose members interleave; 64-output publisher chunks."""
    monkeypatch.setenv("CASIM_PUB_CHUNK", "64")
    ps = Pods(BASE, OTHER, THIRD)
    a, b, c = ps.interleaved(BASE), ps.interleaved(THIRD), ps.interleaved(OTHER)
    groups = [a, a, c, a, b, c, c, a, c]
    tm = [_tmpl((T_MID, T_SMALL)[i % 2]) for i in range(9)]
    _check(oracle, monkeypatch, ps.all, tm, groups, 3, max_nodes, L0=2)


@pytest.mark.parametrize("size", [0, 1, 2, 12, 13])
def test_shared_group_sizes(size, oracle, monkeypatch):
    """Shared lists of 0, 1, 2, 12 and 13 pods (pdqsort's insertion-sort edge is 12)."""
    ps = Pods(BASE, OTHER)
    a, c = ps.interleaved(BASE)[:size], ps.interleaved(OTHER)
    for max_nodes in LIMITS:
        _check(oracle, monkeypatch, ps.all, [_tmpl(T_MID), _tmpl(T_SMALL), _tmpl(T_SMALL)], [a, c, a], 2, max_nodes)
