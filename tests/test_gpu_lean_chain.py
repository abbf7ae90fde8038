"""The lean run-table chain (k_ffd_chain<.., TB, LEAN>: rows in LDS, no ports or extended
resources, no node ordinals, groups of at most 2^20 pods, every quantity below 2^53) and the
generic kernel (CASIM_LEAN_CHAIN=0) against the CPU restatement on the same inputs: bit-exact
results, lastIndex and scheduled pods up to n_scheduled, with the ids published as 32-bit and
16-bit words and left in device memory.  stats()["lean_chain"] says which kernel ran.

The batches are built like test_gpu_table_chain's (a few pod shapes, deep-copied, no two of
them tying on their score against a template used here), at most 3 groups and ~400 pods, at the
edges the run loop has: block and wave boundaries of the row pass, blocks whose summary admits
a pod no row fits, a block emptied and opened again, the run endings and copy levels, the
rotation start, the limiter, the per-pod path between runs, the table's float64 constants of
zero requests, the fallbacks and a second speculation round.

The lean kernel's per-pod path is reached by classes of one pod only: a class fails
batchable() through host ports, extended resources, an unsupported record (the whole group
is then refused) or a negative request, and the first two make the plan one with port or
scalar columns, which the generic kernel runs.
"""
import copy

import numpy as np
import pytest

from autoscaler_amd import k8s, native
from estgen import _encode_estimate
import test_gpu_table_chain as tc

pytestmark = pytest.mark.gpu

GI, MI = tc.GI, tc.MI

# tc.SHAPES and: `half` (two fill a T_ONE node and none fits beside a `top`), a cpu-heavy and a
# memory-heavy pair whose leftovers on T_MID admit `mid` per dimension but in no single row,
# a cpu-only pod (no memory request: reciprocal +inf), a pod with no request at all, and one
# whose memory request is not below 2^53.
# T_ONE scores: top 1.33 > half 1.0 > s1 0.67 > s2 > s3 > bottom.  T_MID / T_SMALL scores:
# cpuh 1.06 > memh 1.0 > mid 0.5 > s1 0.25 > s2 > s3 > conly (150m: 0.019 / 0.038) > bottom's
# 0.02 only on T_MID, so `conly` and `bottom` are never in one batch on T_SMALL; zero 0.
SHAPES = dict(tc.SHAPES)
SHAPES.update({
    "half": tc._pod("half", 1500, 3 * GI),
    "cpuh": tc._pod("cpuh", 7000, 3 * GI),
    "memh": tc._pod("memh", 1000, 14 * GI),
    "mid": tc._pod("mid", 2000, 4 * GI),
    "conly": k8s.build_test_pod("conly", 150, -1),
    "zero": k8s.build_test_pod("zero", -1, -1),
    "huge": k8s.build_test_pod("huge", 100, (1 << 53) + 4096),
})
T_ONE, T_MID, T_SMALL = tc.T_ONE, tc.T_MID, tc.T_SMALL


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


def _inputs(groups, templates, n_existing=0):
    """tc._inputs over this file's shapes, on templates without an extended resource."""
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
    # (no extended resource on the templates: tc._template's FPGA column makes a plan PS)
    return nodes, pods, [(k8s.build_test_node(*t), []) for t in templates], sel


def _check(oracle, monkeypatch, inputs, max_nodes, L0=0, expect_lean=True, min_rounds=1):
    """Every output mode with CASIM_LEAN_CHAIN 1 and 0 against the oracle; with node ordinals
    wanted the generic kernel runs whatever the switch says."""
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
            monkeypatch.setenv("CASIM_LEAN_CHAIN", knob)
            what = (knob, max_nodes, L0)
            lean = knob == "1" and expect_lean

            def ran(mode, want=lean):
                st = plan.stats()
                assert st["decoupled"] and st["table_chain"], (what, mode, st)
                assert st["lean_chain"] == want, (what, mode, st)
                assert st["rounds"] >= min_rounds, (what, mode, st["rounds"])

            p = plan.run(max_nodes, L0, want_nodes=False)                  # 32-bit ids, published
            ran("host32")
            tc._same(ro, p, off, G, what + ("host32",), nodes=False)
            d = plan.run(max_nodes, L0, device_results=True)               # left in device memory
            ran("device")
            assert np.array_equal(ro.results, d.results) and ro.last_index == d.last_index, what
            d.sched_pod = plan.fetch()
            tc._same(ro, d, off, G, what + ("device",), nodes=False)
            h = plan.run_u16(max_nodes, L0)                                # 16-bit ids, published
            ran("u16")
            tc._same(ro, h, off, G, what + ("u16",), nodes=False, u16=True)
            g = plan.run(max_nodes, L0, want_nodes=True)                   # node ordinals: generic
            ran("nodes", want=False)
            tc._same(ro, g, off, G, what + ("nodes",))
    m.close()


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 257])
def test_block_and_wave_boundaries(n, oracle, monkeypatch):
    """One `top` per T_ONE node: n rows with 1000m / 2 GiB left, so k sits on, before and
    after a 64-row block bound and a wave's range bound (1, 2, 3 and 5 blocks over 4 waves,
    the last block partial); 100 `s3` (four fit a leftover) go round the rows with room and
    30 `bottom` meet several copy counts.  Chunks of 64 outputs."""
    monkeypatch.setenv("CASIM_PUB_CHUNK", "64")
    groups = [[("top", n), ("s3", 100), ("bottom", 30)]]
    _check(oracle, monkeypatch, _inputs(groups, [T_ONE]), 0)


def test_false_admission_and_reopened_block(oracle, monkeypatch):
    """Group 0: three rows with cpu left (1000m, 13 GiB) and three with memory left (7000m,
    2 GiB): their block's summary admits `mid` (2000m, 4 GiB), no row fits it — the summary is
    tightened, `mid` opens a node, and the next runs (`s2`, `bottom`) see the tightened
    summary and find room.  Group 1: a block admitted (`s1` fills the leftovers), emptied for
    `s2` (stale summary, then exact: nothing left), opened again by `s2`'s new node and
    admitted for `s3`.  Group 2: both with the limiter."""
    g0 = [("cpuh", 3), ("memh", 3), ("mid", 4), ("s2", 10), ("bottom", 25)]
    g1 = [("top", 4), ("s1", 4), ("s2", 7), ("s3", 5)]
    inputs = _inputs([g0, g1, g0], [T_MID, T_ONE, T_MID])
    for max_nodes in (0, 7):
        _check(oracle, monkeypatch, inputs, max_nodes)


def test_run_endings_and_levels(oracle, monkeypatch):
    """Four leftovers of 1000m / 2 GiB hold eight `s2`: a run of 8 uses the capacity exactly
    (S = RN), a run of 11 is short of it (an opening follows); `s2` x 3 and `s3` x 2 leave
    rows of at least three distinct `bottom` copy counts for a run in excess of its 12 pods
    (several levels); and two of three leftovers filled by `s1` leave exactly one row with
    room for `s2` x 2."""
    groups = [
        [("top", 4), ("s2", 8), ("s3", 6)],
        [("top", 4), ("s2", 11), ("s3", 6)],
        [("top", 4), ("s2", 3), ("s3", 2), ("bottom", 12)],
    ]
    _check(oracle, monkeypatch, _inputs(groups, [T_ONE] * 3), 0)
    one_row = [[("top", 3), ("s1", 2), ("s2", 2), ("s3", 3)]]
    _check(oracle, monkeypatch, _inputs(one_row, [T_ONE]), 0)


@pytest.mark.parametrize("L0", [0, 3, 6, 8, 10, 123])
def test_rotation_start(L0, oracle, monkeypatch):
    """Five existing nodes and input lastIndex values before, among and past the new rows (the
    modulo of a caller-supplied value included).  Group 0: `half` pairs fill the last rows,
    `s1` x 3 and one `s2` leave the rotation start past the only row with room for `s3` x 2.
    Group 1: the start between two rows with room."""
    groups = [
        [("top", 4), ("half", 4), ("s1", 3), ("s2", 1), ("s3", 2), ("bottom", 9)],
        [("top", 5), ("s1", 3), ("s2", 1), ("s3", 3), ("bottom", 9)],
    ]
    _check(oracle, monkeypatch, _inputs(groups, [T_ONE, T_ONE], n_existing=5), 0, L0=L0)


@pytest.mark.parametrize("max_nodes", [1, 2, 9, 10, 12])
def test_limiter(max_nodes, oracle, monkeypatch):
    """Nine `top` open nine rows: max_nodes 9 equals the rows already open when `s2` (18 fit
    the leftovers, 50 asked) wants its first new node; 10 and 12 stop inside its closed-form
    opening; 1 and 2 stop inside `top`'s."""
    groups = [[("top", 9), ("s2", 50), ("bottom", 45)]]
    _check(oracle, monkeypatch, _inputs(groups, [T_ONE]), max_nodes)


def test_record_kinds(oracle, monkeypatch):
    """A class of one pod between runs (the per-pod path and back), a cpu-only class (zero
    memory request), a class with no request at all on a template of 10 pod slots; and a
    host-port class between batchable ones, whose plan has port columns: the generic kernel."""
    plain = [
        [("s1", 30), ("s2", 1), ("conly", 12), ("s3", 1), ("bottom", 20), ("zero", 7)],
        [("s1", 9), ("s3", 1), ("zero", 25)],
        [("top", 1), ("conly", 40), ("zero", 1)],
    ]
    for max_nodes in (0, 3):
        _check(oracle, monkeypatch, _inputs(plain, [T_MID, T_SMALL, T_MID]), max_nodes)
    port = [[("s2", 30), ("port", 9), ("s3", 30)]]
    _check(oracle, monkeypatch, _inputs(port, [T_MID]), 0, expect_lean=False)


def test_request_not_below_2p53(oracle, monkeypatch):
    """A podset with a memory request of 2^53 + 4096: float64 copy counts are not exact for
    every run of its plans, which keep the generic kernel."""
    groups = [[("huge", 3), ("s1", 20), ("s3", 30)], [("s2", 40)]]
    _check(oracle, monkeypatch, _inputs(groups, [T_MID, T_MID]), 0, expect_lean=False)


def test_speculation_rounds(oracle, monkeypatch):
    """Round 1 guesses the batch's input lastIndex for group 1, group 0 leaves another one and
    group 1's outcome depends on it (several new nodes before its first FitsAnyNode success):
    the lean kernel runs again from the corrected value."""
    groups = [[("top", 9), ("s2", 50), ("bottom", 45)], [("top", 5), ("s1", 33), ("s3", 20)]]
    inputs = _inputs(groups, [T_ONE, T_ONE], n_existing=5)
    _check(oracle, monkeypatch, inputs, 40, L0=3, min_rounds=2)
    _check(oracle, monkeypatch, inputs, 0, L0=123, min_rounds=2)
