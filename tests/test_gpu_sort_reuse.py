"""The Go-order ids of the decoupled path belong to the plan: they are sorted once, queued when
the plan is created, and a run whose settings match the record of the stored ids launches no
sort (`stats()["sort_reused"]`); any other decoupled run sorts again under a new epoch, and a
run that is not decoupled or failed invalidates the record.  CASIM_SORT_REUSE=0 sorts in every
run.

The plan is test_gpu_sort_fan's: lists of 2,100 / 5,000 / 9,000 / 120 pods, five groups in four
sort classes, CASIM_SORT_FAN_MIN=0 so the sorts fan.  The reference is the oracle's estimate,
exact; every run with the ids reused is also byte-equal to the same run of a plan that sorts in
every run.
"""
import numpy as np
import pytest

from autoscaler_amd import native
import test_gpu_sort_fan as sf
import test_gpu_table_chain as tc

pytestmark = pytest.mark.gpu

MODES = sf.MODES
L_NONZERO = 2


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


@pytest.fixture(scope="module")
def inputs(oracle):
    """test_gpu_sort_fan's plan, encoded once, and the oracle's result per (max_nodes, last_index)."""
    return _inputs(oracle)


def _inputs(oracle):
    ps = sf.ts.Pods(sf.L2100, sf.L5000, sf.L9000, sf.L120)
    lists = [ps.interleaved(x) for x in (sf.L2100, sf.L5000, sf.L9000, sf.L120)]
    groups = lists + [lists[1]]
    tm = [sf.ts._tmpl(tc.T_MID)] * 4 + [sf.ts._tmpl(tc.T_SMALL)]
    table, node_recs, tmr, off, pod_idx = sf._encode_estimate([], ps.all, tm, groups)
    want = {}
    for max_nodes in (0, 3):
        for L0 in (0, L_NONZERO):
            o = oracle.OracleState()
            o.clear()
            want[max_nodes, L0] = o.estimate(table, off, pod_idx, tmr, max_nodes, L0)
    return table, tmr, off, pod_idx, len(groups), want


def _knobs(monkeypatch, chunk=None, reuse=None):
    monkeypatch.setenv("CASIM_SORT_FAN_MIN", "0")
    if chunk:
        monkeypatch.setenv("CASIM_PUB_CHUNK", chunk)             # tickets straddle part bounds
    if reuse is None:
        monkeypatch.delenv("CASIM_SORT_REUSE", raising=False)
    else:
        monkeypatch.setenv("CASIM_SORT_REUSE", reuse)            # (read in every run)


def _run(plan, mode, max_nodes, L0):
    if mode == "nodes":
        g = plan.run(max_nodes, L0, want_nodes=True)
    elif mode == "host32":
        g = plan.run(max_nodes, L0, want_nodes=False)
    elif mode == "device":
        g = plan.run(max_nodes, L0, device_results=True)
        g.sched_pod = plan.fetch()
    else:
        g = plan.run_u16(max_nodes, L0)
    return g, plan.stats()


def _blob(g, mode):
    return (g.results.tobytes(), np.asarray(g.sched_pod).tobytes(),
            g.sched_node.tobytes() if mode == "nodes" else b"", g.last_index)


def _exact(ro, g, off, G, mode, what):
    tc._same(ro, g, off, G, what, nodes=mode == "nodes", u16=mode == "u16")


def _consecutive(m, inputs, mode, max_nodes, L0, sync_first):
    """Four runs of a fresh plan: each run's blob and stats."""
    table, tm, off, pod_idx, G, want = inputs
    out = []
    with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
        if sync_first:
            # (dlsym through the library's handle reaches the HIP runtime it is linked against)
            assert m.lib.hipDeviceSynchronize() == 0
        for r in range(4):
            g, st = _run(plan, mode, max_nodes, L0)
            _exact(want[max_nodes, L0], g, off, G, mode, (mode, max_nodes, L0, sync_first, r))
            out.append((_blob(g, mode), st))
    return out


@pytest.mark.parametrize("chunk", ["512", None])
@pytest.mark.parametrize("max_nodes,L0", [(0, 0), (3, 0), (3, L_NONZERO), (0, L_NONZERO)])
def test_consecutive_runs(max_nodes, L0, chunk, inputs, monkeypatch):
    m = native.Mirror(0)
    m.clear()
    for mode in MODES:
        for sync_first in (False, True):         # right after creation (sort maybe in flight) / after a device sync
            _knobs(monkeypatch, chunk, reuse="0")
            every = _consecutive(m, inputs, mode, max_nodes, L0, sync_first)
            _knobs(monkeypatch, chunk)
            kept = _consecutive(m, inputs, mode, max_nodes, L0, sync_first)
            for r in range(4):
                what = (mode, max_nodes, L0, chunk, sync_first, r)
                assert kept[r][0] == every[r][0], what + ("differs from a run that sorts",)
                se, sk = every[r][1], kept[r][1]
                assert not se["sort_reused"], what             # CASIM_SORT_REUSE=0: a sort in every run
                assert sk["sort_reused"], what                  # sorted at creation: no run sorts
                assert sk["sort_ms"] == 0, what
                for st in (se, sk):
                    assert st["decoupled"] and st["sorts"] == 4 and st["sort_parts"] > 4, what + (st,)
                assert sk["sort_parts"] == se["sort_parts"], what
                if mode in ("host32", "u16"):
                    assert sk["results_path"] == se["results_path"] == "published", what
    m.close()


def test_reuse_switched_on_within_a_plan(inputs, monkeypatch):
    """A plan created with reuse off sorts nothing at creation: its first run with reuse on
    finds the previous run's ids; with reuse off again every run sorts."""
    table, tm, off, pod_idx, G, want = inputs
    m = native.Mirror(0)
    m.clear()
    _knobs(monkeypatch, reuse="0")
    with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
        seen = []
        for reuse in ("0", None, None, "0", None):
            _knobs(monkeypatch, reuse=reuse)
            g, st = _run(plan, "u16", 3, 0)
            _exact(want[3, 0], g, off, G, "u16", (reuse, len(seen)))
            assert st["sorts"] == 4 and st["sort_parts"] > 4, st
            seen.append(st["sort_reused"])
        assert seen == [False, True, True, False, True], seen
    m.close()


FLIPS = [("CASIM_GO_DECOUPLE", "0"), ("CASIM_TABLE_CHAIN", "0"), ("CASIM_RUNS_STREAM", "0"),
         ("CASIM_NO_RANK_FOLD", "1")]


@pytest.mark.parametrize("mode", MODES)
def test_knob_flips_within_one_plan(mode, inputs, monkeypatch):
    """A run each: default, flipped, default.  The coupled path (its Go sort shares the sort's
    scratch) and another rank fold (other settings) make the next run sort; the chain and
    stream knobs do not reach the sort."""
    table, tm, off, pod_idx, G, want = inputs
    m = native.Mirror(0)
    m.clear()
    _knobs(monkeypatch)
    with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
        for knob, value in FLIPS:
            flags = []
            for step in ("before", "flipped", "after", "again"):
                if step == "flipped":
                    monkeypatch.setenv(knob, value)
                g, st = _run(plan, mode, 3, L_NONZERO)
                if step == "flipped":
                    monkeypatch.delenv(knob)
                _exact(want[3, L_NONZERO], g, off, G, mode, (knob, step))
                flags.append(st["sort_reused"])
                if knob == "CASIM_GO_DECOUPLE" and step == "flipped":
                    assert not st["decoupled"], (knob, st)
                else:
                    assert st["decoupled"] and st["sorts"] == 4 and st["sort_parts"] > 4, (knob, step, st)
            sorts_again = knob in ("CASIM_GO_DECOUPLE", "CASIM_NO_RANK_FOLD")
            assert flags == [True, not sorts_again, not sorts_again, True], (knob, flags)
    m.close()


@pytest.mark.parametrize("mode", ["device", "u16"])
def test_two_plans_on_one_mirror(mode, inputs, monkeypatch):
    table, tm, off, pod_idx, G, want = inputs
    m = native.Mirror(0)
    m.clear()
    _knobs(monkeypatch)
    with native.EstimatePlan(m, table, off, pod_idx, tm) as a:
        g, st = _run(a, mode, 3, 0)
        _exact(want[3, 0], g, off, G, mode, "a0")
        with native.EstimatePlan(m, table, off, pod_idx, tm) as b:       # created between two runs of a
            for r in range(3):
                for name, plan in (("a", a), ("b", b)):
                    g, st = _run(plan, mode, 3 if r != 1 else 0, 0)
                    _exact(want[3 if r != 1 else 0, 0], g, off, G, mode, (name, r))
                    assert st["sort_reused"] and st["sorts"] == 4, (name, r, st)
    m.close()


def test_publisher_give_up_then_a_normal_run(inputs, monkeypatch):
    table, tm, off, pod_idx, G, want = inputs
    m = native.Mirror(0)
    m.clear()
    _knobs(monkeypatch)
    with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
        monkeypatch.setenv("CASIM_PUB_SERIAL", "1")
        g, st = _run(plan, "u16", 3, 0)
        _exact(want[3, 0], g, off, G, "u16", "serial")
        assert st["results_path"] == "publisher_gave_up", st
        monkeypatch.delenv("CASIM_PUB_SERIAL")
        g, st = _run(plan, "u16", 3, 0)
        _exact(want[3, 0], g, off, G, "u16", "normal")
        assert st["results_path"] == "published" and st["sort_reused"], st
    m.close()


def test_option_and_multi_constructors(inputs, monkeypatch):
    """EstimatePlan.from_options (the sort queued behind the kernel that builds the lists) and
    a MultiEstimatePlan over two mirrors on device 0: two runs each, exact and byte-equal."""
    table, tm, off, pod_idx, G, want = inputs
    _knobs(monkeypatch)
    # equivalence groups: the four distinct lists; group 4 takes list 1
    eg_off = np.array([off[0], off[1], off[2], off[3], off[4]], np.int32)
    eg_pod = pod_idx[: off[4]]
    ok = np.zeros((G, 4), np.uint8)
    for g, e in enumerate((0, 1, 2, 3, 1)):
        ok[g, e] = 1
    ms = [native.Mirror(0) for _ in range(2)]
    for m in ms:
        m.clear()
    with native.EstimatePlan.from_options(ms[0], table, eg_off, eg_pod, ok, tm) as plan:
        assert plan.group_off.tobytes() == np.asarray(off, np.int32).tobytes()
        for mode in MODES:
            blobs = []
            for r in range(2):
                g, st = _run(plan, mode, 3, 0)
                _exact(want[3, 0], g, off, G, mode, ("options", mode, r))
                assert st["sort_reused"] and st["sorts"] == 4, (mode, r, st)
                blobs.append(_blob(g, mode))
            assert blobs[0] == blobs[1], mode
    with native.Multi(ms) as mm, native.MultiEstimatePlan(mm, table, off, pod_idx, tm) as plan:
        blobs = []
        for r in range(2):
            g = plan.run(3, 0)
            tc._same(want[3, 0], g, off, G, ("multi", r))
            blobs.append((g.results.tobytes(), g.sched_pod.tobytes(), g.sched_node.tobytes(), g.last_index))
        assert blobs[0] == blobs[1]
    for m in ms:
        m.close()


def test_destroy_without_and_after_a_run(inputs, monkeypatch):
    table, tm, off, pod_idx, G, want = inputs
    m = native.Mirror(0)
    m.clear()
    _knobs(monkeypatch)
    native.EstimatePlan(m, table, off, pod_idx, tm).close()              # its sort may still be queued
    plan = native.EstimatePlan(m, table, off, pod_idx, tm)
    g, st = _run(plan, "host32", 0, 0)
    plan.close()
    _exact(want[0, 0], g, off, G, "host32", "destroyed after one run")
    with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:        # the pooled streams serve the next plan
        g, st = _run(plan, "u16", 0, 0)
        _exact(want[0, 0], g, off, G, "u16", "next plan")
    m.close()


@pytest.mark.parametrize("reuse", ["0", None])
def test_epoch_wrap(reuse, inputs, monkeypatch):
    """The plan's epochs start at INT32_MAX - 1 (test hook): the sort of the creation, or of the
    first run with reuse off, takes INT32_MAX and the next one clears the table and starts
    over.  With reuse on the rank fold is flipped so that runs 2 and 3 sort."""
    table, tm, off, pod_idx, G, want = inputs
    m = native.Mirror(0)
    m.clear()
    _knobs(monkeypatch, reuse=reuse)
    monkeypatch.setenv("CASIM_IDS_EPOCH_NEAR_WRAP", "1")
    for mode in ("u16", "device"):
        with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
            flags = []
            for r in range(3):
                if reuse is None and r == 1:
                    monkeypatch.setenv("CASIM_NO_RANK_FOLD", "1")
                if reuse is None and r == 2:
                    monkeypatch.delenv("CASIM_NO_RANK_FOLD")
                g, st = _run(plan, mode, 3, L_NONZERO)
                _exact(want[3, L_NONZERO], g, off, G, mode, (reuse, mode, r))
                assert st["sorts"] == 4 and st["sort_parts"] > 4, (reuse, mode, r, st)
                flags.append(st["sort_reused"])
            assert flags == ([False] * 3 if reuse == "0" else [True, False, False]), (reuse, mode, flags)
    m.close()
