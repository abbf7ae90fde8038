"""The parts of the Go-order sort a publisher ticket waits for (k_publish): a pure chunk its own
slice, a segment ticket the positions its first and last overlapping segments bound, every
part once the group's chain has stepped a pod alone.  Results against the CPU restatement,
16-bit and 32-bit ids:

* CASIM_SORT_FAN_MIN=0 with 2 and 8 sort parts, chunks of 64 and 512 outputs: tickets
  straddle part bounds;
* two publisher blocks (far more tickets than blocks), an empty group, a count that is a
  multiple of the chunk, a group the limiter stops (a -1 tail, segment boundaries),
  non-batchable pods (single steps: every part), a second speculation round, and the
  serialised give-up.

What these runs can and cannot see: a ticket that waited for too few parts reads ids the sort
has not written yet, which shows only where the ids buffer does not already hold the same ids
from an earlier run — the first run of a plan and the first after max_nodes changes (every
test here creates its plan and changes max_nodes once), and then only if the read wins the
race.  The rule itself — the range covers every position a chunk reads — is checked
exhaustively on the CPU in tests/test_publish_ranges.py, which restates k_publish's two
searches and its range by hand; these GPU runs tie that restatement to the kernel.
"""
import time

import numpy as np
import pytest

from autoscaler_amd import native
from estgen import _encode_estimate
import test_gpu_sort_share as ts
import test_gpu_table_chain as tc

pytestmark = pytest.mark.gpu

# three lists (sort classes) of 1,500 to 3,000 pods; four groups share each
LA = [("s1", 400), ("mb", 300), ("s3", 500), ("bottom", 300)]                 # 1,500
LB = [("top", 300), ("s2", 800), ("s3", 600), ("bottom", 500)]                # 2,200
LC = [("s1", 900), ("s2", 700), ("mc", 400), ("s3", 600), ("bottom", 400)]    # 3,000
RANK_ALIKE = (ts.T_MID, ts.T_SMALL, ts.T_DOUBLE, ts.T_RENAMED)
# edges: an empty group, 1,536 = 3 x 512 = 24 x 64 outputs, host-port and extended-resource pods
EDGE = [[], [("s1", 512), ("s3", 512), ("bottom", 512)], [("s2", 700), ("port", 9), ("s3", 800)],
        [("fpga", 11), ("s2", 900), ("bottom", 700)]]


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


def _reference(oracle, table, off, pod_idx, tm, limits, L0=0):
    want = {}
    for max_nodes in limits:
        o = oracle.OracleState()
        o.clear()
        want[max_nodes] = o.estimate(table, off, pod_idx, tm, max_nodes, L0)
    return want


@pytest.fixture(scope="module")
def batch(oracle):
    """12 groups in 3 sort classes, encoded once; the oracle's result without a limit and with
    max_nodes 3 (every group stops early: a -1 tail, chunks cut by segment boundaries)."""
    ps = ts.Pods(LA, LB, LC)
    lists = [ps.interleaved(x) for x in (LA, LB, LC)]
    groups = [lists[i % 3] for i in range(12)]
    tm = [ts._tmpl(RANK_ALIKE[i // 3]) for i in range(12)]
    table, _, tmr, off, pod_idx = _encode_estimate([], ps.all, tm, groups)
    return table, tmr, off, pod_idx, len(groups), _reference(oracle, table, off, pod_idx, tmr, (0, 3))


@pytest.fixture(scope="module")
def edge_batch(oracle):
    ps = ts.Pods(*[g for g in EDGE if g])
    groups = [ps.interleaved(g) if g else [] for g in EDGE]
    tm = [ts._tmpl(ts.T_MID)] * len(groups)
    table, _, tmr, off, pod_idx = _encode_estimate([], ps.all, tm, groups)
    assert off[1] == off[0] and (off[2] - off[1]) % 512 == 0
    return table, tmr, off, pod_idx, len(groups), _reference(oracle, table, off, pod_idx, tmr, (0, 3))


def _knobs(monkeypatch, chunk="64", parts="8", blocks=None):
    monkeypatch.setenv("CASIM_SORT_FAN_MIN", "0")
    monkeypatch.setenv("CASIM_SORT_FAN_PARTS", parts)
    monkeypatch.setenv("CASIM_PUB_CHUNK", chunk)
    if blocks:
        monkeypatch.setenv("CASIM_PUB_BLOCKS", blocks)


def _published(plan, max_nodes, L0, ro, off, G, what, min_rounds=1):
    """One 16-bit and one 32-bit published run against the oracle's result."""
    for u16 in (True, False):
        g = plan.run_u16(max_nodes, L0) if u16 else plan.run(max_nodes, L0, want_nodes=False)
        st = plan.stats()
        w = what + ("u16" if u16 else "i32",)
        assert st["decoupled"] and st["results_path"] == "published", (w, st)
        assert st["rounds"] >= min_rounds, (w, st)
        tc._same(ro, g, off, G, w, nodes=False, u16=u16)
        a = np.asarray(g.sched_pod)
        for k in range(G):                                   # past n_scheduled: "not scheduled"
            if int(ro.results[k]["status"]) == 0:
                tail = a[int(off[k]) + int(ro.results[k]["n_scheduled"]):int(off[k + 1])]
                assert (tail == (0xFFFF if u16 else -1)).all(), (w, k)


@pytest.mark.parametrize("chunk", ["64", "512"])
@pytest.mark.parametrize("parts", ["2", "8"])
def test_tickets_across_part_bounds(parts, chunk, batch, monkeypatch):
    table, tm, off, pod_idx, G, want = batch
    _knobs(monkeypatch, chunk, parts)
    m = native.Mirror(0)
    m.clear()
    with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
        for max_nodes in (0, 3):
            for r in range(2):                               # (a second run: the flags' epochs)
                _published(plan, max_nodes, 0, want[max_nodes], off, G, (parts, chunk, max_nodes, r))
            assert plan.stats()["sorts"] == 3 and plan.stats()["sort_parts"] > 3
    m.close()


def test_two_publisher_blocks(batch, monkeypatch):
    """Far more tickets than blocks: every block serves many tickets in turn."""
    table, tm, off, pod_idx, G, want = batch
    _knobs(monkeypatch, blocks="2")
    m = native.Mirror(0)
    m.clear()
    with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
        for max_nodes in (0, 3):
            _published(plan, max_nodes, 0, want[max_nodes], off, G, ("two-blocks", max_nodes))
    m.close()


@pytest.mark.parametrize("chunk", ["64", "512"])
def test_edge_groups(chunk, edge_batch, monkeypatch):
    """An empty group, a count that is a multiple of the chunk, and groups with non-batchable
    pods (their chains step pods alone, so their tickets wait for every part)."""
    table, tm, off, pod_idx, G, want = edge_batch
    _knobs(monkeypatch, chunk)
    m = native.Mirror(0)
    m.clear()
    with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
        for max_nodes in (0, 3):
            _published(plan, max_nodes, 0, want[max_nodes], off, G, ("edge", chunk, max_nodes))
    m.close()


def test_second_speculation_round(oracle, monkeypatch):
    """test_gpu_table_chain's batch whose first round guesses the input lastIndex of the later
    groups wrong: the second round's publisher has tickets of the re-run groups alone."""
    groups = [[("top", 9), ("s2", 50), ("bottom", 45)], [("top", 5), ("s1", 33), ("s3", 20)],
              [("top", 7), ("ma", 25), ("mb", 25), ("port", 6)], [("s1", 33), ("bottom", 80)]]
    nodes, pods, templates, sel = tc._inputs(groups, [tc.T_ONE, tc.T_ONE, tc.T_ONE, tc.T_MID], n_existing=5)
    table, node_recs, tm, off, pod_idx = _encode_estimate(nodes, pods, templates, sel)
    _knobs(monkeypatch, chunk="16")
    o, m = oracle.OracleState(), native.Mirror(0)
    for b in (o, m):
        b.clear()
        b.add_nodes(node_recs)
    ro = o.estimate(table, off, pod_idx, tm, 40, 3)
    assert int(ro.results[0]["last_index_out"]) != 3         # the premise: round 1's guess is wrong
    with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
        _published(plan, 40, 3, ro, off, len(groups), ("rounds",), min_rounds=2)
    m.close()


def test_serialised_publisher_gives_up(oracle, monkeypatch):
    """CASIM_PUB_SERIAL=1: the publisher runs before the chains on their stream, gives up at
    its start deadline, and the stream-ordered copy delivers the
    results — in bounded time (2 ms deadline + the copy, never the 200 ms guard).  The batch
    is test_estimate_publisher_bounded's: flat, so no heavy / light split (the light groups'
    chains of a split batch run on a stream of their own beside the serialised publisher,
    which then rightly waits for the heavy groups' tickets until the dead-chain guard)."""
    from autoscaler_amd import workloads as W
    w = W.c2(n_pods=8000, n_groups=20, n_existing=50)
    o = oracle.OracleState()
    W.load_estimate(o, w)
    ro = o.estimate(w.table, w.group_off, w.pod_idx, w.templates, w.max_nodes, 0)
    _knobs(monkeypatch)
    monkeypatch.setenv("CASIM_PUB_SERIAL", "1")
    m = native.Mirror(0)
    W.load_estimate(m, w)
    walls = []
    with native.EstimatePlan(m, w.table, w.group_off, w.pod_idx, w.templates) as plan:
        for r in range(3):
            for u16 in (True, False):
                t = time.perf_counter()
                g = plan.run_u16(w.max_nodes, 0) if u16 else plan.run(w.max_nodes, 0, want_nodes=False)
                walls.append(time.perf_counter() - t)
                assert plan.stats()["results_path"] == "publisher_gave_up", (r, u16)
                assert np.array_equal(ro.results, g.results) and ro.last_index == g.last_index
                sp = np.where(g.sched_pod == 0xFFFF, -1, g.sched_pod.astype(np.int32)) if u16 else g.sched_pod
                assert np.array_equal(ro.sched_pod, sp), (r, u16)
    m.close()
    assert min(walls) < 0.05, walls
