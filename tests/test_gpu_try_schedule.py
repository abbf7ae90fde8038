"""ca_try_schedule_pods on the HIP path (filter.hip: k_fb_acc, k_fb_walk<true>, k_filter_out)
vs the reference loop composed over the CPU restatement (tspgen.try_schedule_ref): exact
equality of node, mirror pod id, hints, hint_ok, lastIndex, evaluations, overflowing
controllers, placed and tried, for both kernels, every mask, with and without the break."""
import numpy as np
import pytest

from autoscaler_amd import abi, native
from autoscaler_amd import workloads as W
from autoscaler_amd.clustersnapshot import ClusterSnapshot
from autoscaler_amd.podlistprocessor import PodPriority
from autoscaler_amd.predicatechecker import SchedulerBasedPredicateChecker
from autoscaler_amd.simulator import HintingSimulator
from fosgen import rand_filter_case
import tspgen as T

pytestmark = pytest.mark.gpu

PATHS = ["bitmap", "window"]


def _force(path, monkeypatch):
    if path == "window":
        monkeypatch.setenv("CASIM_FO_WINDOW", "1")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("brk", [False, True], ids=["all", "break"])
@pytest.mark.parametrize("wn,mn", T.CASES, ids=[f"{a}-{b}" for a, b in T.CASES])
def test_try_schedule_masks(wn, mn, brk, path, oracle_lib, monkeypatch):
    _force(path, monkeypatch)
    w = T.workload(wn)
    ref = T.ref_case(oracle_lib.OracleState, wn, mn, brk)
    g = native.Mirror(0)
    W.load_filter(g, w)
    got = g.try_schedule_pods(w.pending, w.order, T.make_match(mn, w, T.L0), brk, w.class_owner, w.hints, T.L0)
    st = g.filter_stats()
    assert st["path"] == path
    T.eq_try(got, ref, (wn, mn, brk, path))
    if mn == "ones" and not brk:
        # an all-ones mask is FilterOutSchedulable: byte for byte, on the same kernel
        f = native.Mirror(0)
        W.load_filter(f, w)
        fo = f.filter_out_schedulable(w.pending, w.order, w.class_owner, w.hints, T.L0)
        assert f.filter_stats()["path"] == path
        for a in ("node", "pod_id", "hints"):
            assert getattr(got, a).tobytes() == getattr(fo, a).tobytes(), a
        assert (got.placed, got.last_index, got.evals, got.n_overflowing) == \
               (fo.placed, fo.last_index, fo.evals, fo.n_overflowing)
        assert got.tried == len(w.order)
        f.close()
    g.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("brk", [False, True], ids=["all", "break"])
def test_try_schedule_plain_all(brk, path, oracle_lib, monkeypatch):
    """match NULL (no acc words): the general kernel with the scan words aliasing vis."""
    _force(path, monkeypatch)
    w = T.workload("n300")
    ref = T.ref_case(oracle_lib.OracleState, "n300", "all", brk)
    g = native.Mirror(0)
    W.load_filter(g, w)
    got = g.try_schedule_pods(w.pending, w.order, None, brk, w.class_owner, w.hints, T.L0)
    assert g.filter_stats()["path"] == path
    T.eq_try(got, ref, ("plain", brk, path))
    g.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("brk", [False, True], ids=["all", "break"])
@pytest.mark.parametrize("mn", ["all", "half", "altwords", "range"])
def test_try_schedule_unschedulable_and_prefilter(mn, brk, path, oracle_lib, monkeypatch):
    """Unschedulable nodes in and outside the mask, tolerating pods hinted onto them (the hint
    check reads the true visibility, the scans the masked one) and a break that stops at a
    PreFilter failure."""
    _force(path, monkeypatch)
    w = T.workload("special")
    ref = T.ref_case(oracle_lib.OracleState, "special", mn, brk)
    g = native.Mirror(0)
    W.load_filter(g, w)
    got = g.try_schedule_pods(w.pending, w.order, T.make_match(mn, w, T.L0), brk, w.class_owner, w.hints, T.L0)
    assert g.filter_stats()["path"] == path
    T.eq_try(got, ref, ("special", mn, brk, path))
    g.close()


def test_try_schedule_arguments():
    w = T.workload("n65")
    g = native.Mirror(0)
    W.load_filter(g, w)
    with pytest.raises(native.CasimError) as e:              # ca_fits_any_node's rule: a MASK needs its bytes
        g.try_schedule_pods(w.pending, w.order, (abi.CA_MATCH_MASK, 0, 0, -1, None), False, w.class_owner, w.hints, 0)
    assert e.value.status == abi.CA_EINVAL
    r = g.try_schedule_pods(w.pending, np.zeros(0, np.int32), T.make_match("edges", w, 0), True, None, None, 5)
    assert (r.placed, r.tried, r.last_index, r.evals, len(r.node), len(r.hint_ok)) == (0, 0, 5, 0, 0, 0)
    g.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("brk", [False, True], ids=["all", "break"])
@pytest.mark.parametrize("wn,mn", [("n300", "altwords"), ("n2000", "half"), ("n65", "edges")])
def test_second_call_and_fork_revert(wn, mn, brk, path, oracle_lib, monkeypatch):
    """The state left behind: fork -> call -> revert -> call again, then a second call fed
    the first call's hints and lastIndex, each against the oracle doing the same."""
    _force(path, monkeypatch)
    w = T.workload(wn)
    match = T.make_match(mn, w, T.L0)
    g, o = native.Mirror(0), oracle_lib.OracleState()
    W.load_filter(g, w)
    W.load_filter(o, w)
    g.fork()
    o.fork()
    r1 = T.try_schedule_ref(o, w.pending, w.order, match, brk, w.class_owner, w.hints, T.L0)
    g1 = g.try_schedule_pods(w.pending, w.order, match, brk, w.class_owner, w.hints, T.L0)
    T.eq_try(g1, r1, "forked")
    g.revert()
    o.revert()
    r2 = T.try_schedule_ref(o, w.pending, w.order, match, brk, w.class_owner, w.hints, T.L0)
    g2 = g.try_schedule_pods(w.pending, w.order, match, brk, w.class_owner, w.hints, T.L0)
    T.eq_try(g2, r2, "after revert")
    assert np.array_equal(r2.node, r1.node)
    # everything again on what the call left: its hints, its lastIndex, no break
    r3 = T.try_schedule_ref(o, w.pending, w.order, match, False, w.class_owner, r2.hints, r2.last_index)
    g3 = g.try_schedule_pods(w.pending, w.order, match, False, w.class_owner, g2.hints, g2.last_index)
    assert g.filter_stats()["path"] == path
    T.eq_try(g3, r3, "second call")
    g.close()


def _snapshot(backend, nodes, scheduled):
    s = ClusterSnapshot(backend)
    s.AddNodes(nodes)
    for p, n in scheduled:
        s.AddPod(p, n)
    return s


@pytest.mark.parametrize("brk", [False, True], ids=["all", "break"])
@pytest.mark.parametrize("seed,n_nodes,n_pending", [(0, 10, 60), (5, 10, 60), (7, 70, 300), (10, 130, 300)])
def test_facade_equals_per_pod(seed, n_nodes, n_pending, brk):
    """HintingSimulator.TrySchedulePods (one device call) == TrySchedulePodsPerPod (two device
    calls per pod) with a callable predicate: statuses, lastIndex, evals, overflowing and both
    Hints generations after a DropOldHints between two calls."""
    nodes, scheduled, pending, hints = rand_filter_case(seed, n_nodes, n_pending)
    pending.sort(key=lambda p: -PodPriority(p))
    half = len(pending) // 2

    def acceptable(info):                                    # a property of the node alone
        return sum(map(ord, info.node.name)) % 3 != 0

    out = []
    for batched in (False, True):
        snap = _snapshot(native.Mirror(0), nodes, scheduled)
        pc = SchedulerBasedPredicateChecker()
        pc.last_index = seed % 7
        sim = HintingSimulator(pc)
        sim.hints.current = dict(hints)
        run = sim.TrySchedulePods if batched else sim.TrySchedulePodsPerPod
        res = []
        for part in (pending[:half], pending[half:]):
            st, ov, err = run(snap, list(part), acceptable, brk)
            assert err is None
            res.append(([(s.pod.name, s.node_name) for s in st], ov, pc.last_index, pc.evals,
                        dict(sim.hints.current), dict(sim.hints.old)))
            sim.DropOldHints()
        out.append({"calls": res, "current": dict(sim.hints.current), "old": dict(sim.hints.old),
                    "pods": sorted((p.name, n.node.name) for n in snap.List() for p in n.pods)})
        snap.backend.close()
    assert out[1] == out[0]
    assert any(c[0] for c in out[0]["calls"])
