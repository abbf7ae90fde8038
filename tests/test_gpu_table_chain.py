"""The run-table chain (decoupled Estimate: the chains walk k_run_table's per-class table in
LDS instead of an emitted stream) against the CPU restatement, and against the stream path
(CASIM_TABLE_CHAIN=0) on the same inputs: bit-exact results, scheduled pods up to
n_scheduled, node ordinals and lastIndex.

Every podset is uniform: a few pod shapes, each deep-copied.  The shapes are chosen so that
no two of them tie on their score against a template below (the plan stays decoupled), and
so that the table walk meets what it can get wrong: absent classes, merged and unmerged
neighbours, single pods, non-batchable classes, the limiter inside a run.
"""
import copy

import numpy as np
import pytest

from autoscaler_amd import k8s, native
from autoscaler_amd.k8s import Container, ContainerPort, Quantity
from estgen import _encode_estimate

pytestmark = pytest.mark.gpu

GI = 1 << 30
MI = 1 << 20
FPGA = "example.com/fpga"


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


def _pod(name, cpu, mem, init_cpu=0, port=0, fpga=0):
    p = k8s.build_test_pod(name, cpu, mem)
    if init_cpu:
        p.init_containers.append(Container(requests={"cpu": Quantity.milli(init_cpu)}))
    if port:
        p.containers[0].ports.append(ContainerPort(host_port=port))
    if fpga:
        p.containers[0].requests[FPGA] = Quantity(fpga)
    return p


# Score order on every template below (cpu : memory allocatable of 1 : 2 GiB per core, and
# 1 : 4): top > s1 > s2 > mb > mc > ma > (port, fpga) > s3 > bottom, with `port` above mb on
# the 1 : 4 template.  ma and mb request the same (their init container's 1500m, 1 GiB) with
# distinct scores (300m and 320m of containers): adjacent ranks unless mc (310m) is present.
SHAPES = {
    "top": _pod("top", 2000, 4 * GI),
    "s1": _pod("s1", 1000, 2 * GI),
    "s2": _pod("s2", 500, 1 * GI),
    "ma": _pod("ma", 300, 1 * GI, init_cpu=1500),
    "mb": _pod("mb", 320, 1 * GI, init_cpu=1500),
    "mc": _pod("mc", 310, 1 * GI),
    "port": _pod("port", 400, 768 * MI, port=8080),          # non-batchable: one per node
    "fpga": _pod("fpga", 350, 640 * MI, fpga=1),             # non-batchable: two per node
    "s3": _pod("s3", 250, 512 * MI),
    "bottom": _pod("bottom", 100, 128 * MI),
}


def _template(name, cpu, mem, pods):
    t = k8s.build_test_node(name, cpu, mem, pods)
    t.allocatable[FPGA] = Quantity(2)
    return (t, [])


T_MID = ("mid", 8000, 16 * GI, 110)
T_SMALL = ("small", 4000, 8 * GI, 10)
T_WIDE = ("wide", 16000, 64 * GI, 110)
T_ONE = ("one", 3000, 6 * GI, 110)          # one `top` pod per node


def _inputs(groups, templates, n_existing=0):
    """groups: per group a list of (shape, count), interleaved round-robin in the group's
    list so the classes are not in rank order there."""
    need = {}
    for grp in groups:
        for s, n in grp:
            need[s] = max(need.get(s, 0), n)
    pods, by_shape = [], {}
    for s, n in need.items():
        by_shape[s] = []
        for r in range(n):
            q = copy.deepcopy(SHAPES[s])
            q.name = q.uid = f"{s}-{r}"
            by_shape[s].append(q)
            pods.append(q)
    sel = []
    for grp in groups:
        lists = [by_shape[s][:n] for s, n in grp]
        out = []
        for i in range(max(len(x) for x in lists)):
            out.extend(x[i] for x in lists if i < len(x))
        sel.append(out)
    nodes = [k8s.build_test_node(f"e{i}", 2000, 4 * GI, 110) for i in range(n_existing)]
    return nodes, pods, [_template(*t) for t in templates], sel


def _same(ro, g, off, n_groups, what, nodes=True, u16=False):
    assert np.array_equal(ro.results, g.results), (what, ro.results, g.results)
    assert ro.last_index == g.last_index, what
    for k in range(n_groups):
        if int(ro.results[k]["status"]) != 0:
            continue
        a, n = int(off[k]), int(ro.results[k]["n_scheduled"])
        got = g.sched_pod[a:a + n]
        if u16:
            got = np.where(got == 0xFFFF, -1, got.astype(np.int32))
        assert np.array_equal(ro.sched_pod[a:a + n], got), (what, k)
        if nodes:
            assert np.array_equal(ro.sched_node[a:a + n], g.sched_node[a:a + n]), (what, k)


def _check(oracle, monkeypatch, inputs, max_nodes, L0=0, expect_table=True, all_modes=False, min_rounds=1):
    nodes, pods, templates, groups = inputs
    table, node_recs, tm, off, pod_idx = _encode_estimate(nodes, pods, templates, groups)
    o, m = oracle.OracleState(), native.Mirror(0)
    for b in (o, m):
        b.clear()
        if len(node_recs):
            b.add_nodes(node_recs)
    ro = o.estimate(table, off, pod_idx, tm, max_nodes, L0)
    G = len(groups)
    if min_rounds > 1:      # (the input's own premise: round 1's guess for group 1 is wrong)
        assert int(ro.results[0]["last_index_out"]) != L0
    with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
        for knob in ("1", "0"):
            monkeypatch.setenv("CASIM_TABLE_CHAIN", knob)
            what = (knob, max_nodes, L0)
            g = plan.run(max_nodes, L0, want_nodes=True)
            st = plan.stats()
            assert st["table_chain"] == (knob == "1" and expect_table), (what, st)
            assert st["decoupled"], what
            assert st["rounds"] >= min_rounds, (what, st["rounds"])
            _same(ro, g, off, G, what)
            if not all_modes:
                continue
            p = plan.run(max_nodes, L0, want_nodes=False)                  # 32-bit ids, published
            assert plan.stats()["table_chain"] == (knob == "1" and expect_table)
            _same(ro, p, off, G, what + ("host32",), nodes=False)
            d = plan.run(max_nodes, L0, device_results=True)               # left in device memory
            assert np.array_equal(ro.results, d.results) and ro.last_index == d.last_index
            d.sched_pod = plan.fetch()
            _same(ro, d, off, G, what + ("device",), nodes=False)
            h = plan.run_u16(max_nodes, L0)                                # 16-bit ids, published
            assert plan.stats()["table_chain"] == (knob == "1" and expect_table)
            _same(ro, h, off, G, what + ("u16",), nodes=False, u16=True)
    m.close()


LIMITS = [0, 1, 2, 40]


@pytest.mark.parametrize("max_nodes", LIMITS)
def test_absent_classes(max_nodes, oracle, monkeypatch):
    """Groups that lack the top-ranked class, the bottom-ranked class, classes in the middle,
    and all classes but one (top / middle / bottom): absent ranks are skipped, their records
    never read."""
    groups = [
        [("s1", 30), ("s2", 25), ("s3", 40), ("bottom", 20)],          # no top
        [("top", 12), ("s1", 30), ("s3", 40)],                          # no bottom, no s2
        [("top", 9), ("bottom", 70)],                                   # the two ends only
        [("top", 17)], [("s2", 33)], [("bottom", 90)],                  # one class
        [("top", 5), ("s1", 5), ("s2", 5), ("s3", 5), ("bottom", 5)],   # every plain class
    ]
    tm = [T_MID, T_SMALL, T_WIDE, T_SMALL, T_MID, T_SMALL, T_MID]
    _check(oracle, monkeypatch, _inputs(groups, tm), max_nodes)


@pytest.mark.parametrize("max_nodes", LIMITS)
def test_merge_rule(max_nodes, oracle, monkeypatch):
    """ma and mb: distinct scores, identical requests.  Adjacent ranks are one run (40 + 30
    pods placed in closed form across the class boundary); with mc ranked between them they
    are two runs; a group with the pair alone, and with the pair at the end of its order."""
    groups = [
        [("s2", 20), ("ma", 40), ("mb", 30), ("s3", 25)],
        [("s2", 20), ("ma", 40), ("mc", 7), ("mb", 30), ("s3", 25)],
        [("ma", 40), ("mb", 30)],
        [("top", 6), ("mb", 3), ("ma", 50)],
    ]
    _check(oracle, monkeypatch, _inputs(groups, [T_MID, T_MID, T_SMALL, T_WIDE]), max_nodes)


@pytest.mark.parametrize("max_nodes", LIMITS)
def test_single_pod_between_runs(max_nodes, oracle, monkeypatch):
    """A class of one pod (the single-pod path) between two long runs, and first / last."""
    groups = [
        [("s1", 80), ("s2", 1), ("s3", 80)],
        [("top", 1), ("s2", 60), ("bottom", 1)],
        [("s1", 1), ("s2", 1), ("s3", 1)],
    ]
    _check(oracle, monkeypatch, _inputs(groups, [T_MID, T_SMALL, T_MID]), max_nodes)


@pytest.mark.parametrize("max_nodes", LIMITS)
def test_non_batchable_classes(max_nodes, oracle, monkeypatch):
    """A host-port class and an extended-resource class between batchable ones (the PS
    instantiation): `count` single pods of one record each, the ports / scalars looked up
    through the rank's representative pod."""
    groups = [
        [("s2", 30), ("port", 9), ("s3", 30)],
        [("s2", 30), ("fpga", 11), ("s3", 30)],
        [("ma", 10), ("port", 5), ("fpga", 6), ("bottom", 40)],
        [("port", 4)], [("fpga", 70), ("top", 3)],
    ]
    _check(oracle, monkeypatch, _inputs(groups, [T_MID, T_MID, T_WIDE, T_SMALL, T_MID]), max_nodes)


@pytest.mark.parametrize("size", [1, 63, 64, 65, 200])
def test_group_sizes(size, oracle, monkeypatch):
    """Groups of 1, 63, 64, 65 and 200 pods (the 64-position window of the pending single
    placements), in three classes where the size allows, limited and not."""
    a = max(size // 3, 1)
    grp = [("s1", a)] + ([("port", min(2, size - a))] if size - a > 0 else []) + \
          ([("s3", size - a - 2)] if size - a - 2 > 0 else [])
    assert sum(n for _, n in grp) == size
    for max_nodes in (0, 2):
        _check(oracle, monkeypatch, _inputs([grp, [("bottom", size)]], [T_SMALL, T_SMALL]), max_nodes)


def test_last_index_and_speculation_rounds(oracle, monkeypatch):
    """A nonzero input lastIndex over existing nodes, and a batch whose first round guesses
    the groups' input lastIndex wrong: the later rounds reuse round 1's table.  Each `top`
    pod fills a T_ONE node alone, so a group's first FitsAnyNode success comes with several
    new nodes — its outcome depends on its input lastIndex — and group 0 leaves another
    lastIndex than the batch's input, which round 1 guessed for every group."""
    groups = [[("top", 9), ("s2", 50), ("bottom", 45)], [("top", 5), ("s1", 33), ("s3", 20)],
              [("top", 7), ("ma", 25), ("mb", 25), ("port", 6)], [("s1", 33), ("bottom", 80)]]
    inputs = _inputs(groups, [T_ONE, T_ONE, T_ONE, T_MID], n_existing=5)
    _check(oracle, monkeypatch, inputs, 40, L0=3, min_rounds=2)
    _check(oracle, monkeypatch, inputs, 0, L0=123, min_rounds=2)


def test_hbm_slab_rows(oracle, monkeypatch):
    """CASIM_CHAIN_GLOBAL=1: rows in the groups' HBM slabs, the table alone in LDS."""
    monkeypatch.setenv("CASIM_CHAIN_GLOBAL", "1")
    groups = [[("s1", 30), ("ma", 20), ("mb", 20), ("port", 5), ("s3", 70)], [("top", 4), ("fpga", 9), ("bottom", 130)]]
    for max_nodes in (0, 2):
        _check(oracle, monkeypatch, _inputs(groups, [T_SMALL, T_MID]), max_nodes, L0=1)


def test_more_classes_than_the_lds_bound(oracle, monkeypatch):
    """4090 score classes: the table (44 B per class) does not fit the 160 KB of LDS, so the
    plan keeps the stream path (table_chain False) and matches."""
    n = 4090
    pods = [k8s.build_test_pod(f"c{i}", 10 + i, 64 * MI) for i in range(n)]
    groups = [pods[::2], pods[1::3]]
    inputs = ([], pods, [_template(*T_MID), _template(*T_WIDE)], groups)
    _check(oracle, monkeypatch, inputs, 2, expect_table=False)


@pytest.mark.parametrize("max_nodes", [0, 3])
def test_output_modes_multi_group(max_nodes, oracle, monkeypatch):
    """Nine groups (the heavy-first split: two streams) through every output mode: node
    ordinals, 32-bit and 16-bit ids published into page-locked memory, device-resident."""
    monkeypatch.setenv("CASIM_PUB_CHUNK", "64")
    base = [("top", 7), ("s1", 40), ("s2", 33), ("ma", 21), ("mb", 19), ("port", 3), ("fpga", 4), ("s3", 90), ("bottom", 66)]
    groups = [base[i % 4:i % 4 + 3 + i % 5] for i in range(8)] + [base]
    tm = [(T_MID, T_SMALL, T_WIDE)[i % 3] for i in range(9)]
    _check(oracle, monkeypatch, _inputs(groups, tm, n_existing=2), max_nodes, L0=2, all_modes=True)
