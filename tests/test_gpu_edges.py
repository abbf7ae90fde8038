"""HIP path vs the CPU restatement at the numeric edges the kernels are built around
(tests/quantgen.py): quotients on a boundary, values at and above 2^53, zero and negative
free values, pod-slot limits, score edges, and one run longer than 2^20 pods.  Exact
equality of every output, through every chain mode the knobs select.  The same node
shapes then go through the kernels that apply AddPod arithmetic to mirror rows."""
import random

import numpy as np
import pytest

import quantgen as Q
from autoscaler_amd import abi, native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


_REF = {}


def _ref(oracle, name, build, limits=None):
    """The case and the oracle's outputs under each (max_nodes, L0): computed once.  By
    default the case's own limiter and a cut (5 nodes per group, another lastIndex)."""
    if name not in _REF:
        case = build()
        limits = limits or [(case.max_nodes, case.L0), (5, 123)]
        o = oracle.OracleState()
        case.load(o)
        _REF[name] = (case, {lim: o.estimate(case.table, case.group_off, case.pod_idx, case.templates, *lim)
                             for lim in limits})
        o.close()
    return _REF[name]


def _same(case, ro, g, what, nodes=True, u16=False):
    assert np.array_equal(ro.results, g.results), (what, ro.results, g.results)
    assert ro.last_index == g.last_index, what
    sp = np.where(g.sched_pod == 0xFFFF, -1, g.sched_pod.astype(np.int32)) if u16 else g.sched_pod
    for k in range(len(case.templates)):
        a, b, n = int(case.group_off[k]), int(case.group_off[k + 1]), int(ro.results[k]["n_scheduled"])
        assert np.array_equal(ro.sched_pod[a:a + n], sp[a:a + n]), (what, k)
        assert (sp[a + n:b] == -1).all(), (what, k)
        if nodes:
            assert np.array_equal(ro.sched_node[a:a + n], g.sched_node[a:a + n]), (what, k)


KNOBS = {                # CASIM_RUN_BATCH, new-node rows (CASIM_CHAIN_GLOBAL), CASIM_SORT
    "default": ("1", "lds", "bucket"),
    "per-pod": ("0", "lds", "bucket"),
    "hbm": ("1", "hbm", "bucket"),
    "hbm-per-pod": ("0", "hbm", "bucket"),
    "merge": ("1", "lds", "merge"),
    "merge-per-pod": ("0", "lds", "merge"),
}


def _set_rows(monkeypatch, rows):
    """CASIM_CHAIN_GLOBAL is read by presence (any value selects the HBM-slab rows): set for
    "hbm", absent for the LDS rows these shapes get by default."""
    if rows == "hbm":
        monkeypatch.setenv("CASIM_CHAIN_GLOBAL", "1")
    else:
        monkeypatch.delenv("CASIM_CHAIN_GLOBAL", raising=False)


def _set_knobs(monkeypatch, knobs):
    batch, rows, sort = KNOBS[knobs]
    monkeypatch.setenv("CASIM_RUN_BATCH", batch)
    _set_rows(monkeypatch, rows)
    monkeypatch.setenv("CASIM_SORT", sort)
    return batch


@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("name", list(Q.small_cases()))
def test_estimate_quantity_edges(name, knobs, oracle, monkeypatch):
    """Every case under its own limiter and under a cut (5 nodes per group, another
    lastIndex), through ca_estimate_batch with and without node ordinals, a plan, and its
    16-bit output."""
    batch = _set_knobs(monkeypatch, knobs)
    case, refs = _ref(oracle, name, Q.small_cases()[name])
    m = native.Mirror(0)
    case.load(m)
    for lim, ro in refs.items():
        g = m.estimate(case.table, case.group_off, case.pod_idx, case.templates, *lim, want_nodes=True)
        _same(case, ro, g, (name, knobs, lim, "batch"))
        if batch == "1":                 # (per-pod chain: ordinals do not change the path)
            g = m.estimate(case.table, case.group_off, case.pod_idx, case.templates, *lim, want_nodes=False)
            _same(case, ro, g, (name, knobs, lim, "batch, no ordinals"), nodes=False)
    with native.EstimatePlan(m, case.table, case.group_off, case.pod_idx, case.templates) as plan:
        for lim, ro in refs.items():
            _same(case, ro, plan.run(*lim, want_nodes=True), (name, knobs, lim, "plan"))
            _same(case, ro, plan.run(*lim, want_nodes=False), (name, knobs, lim, "plan, no ordinals"), nodes=False)
            if name == "score-tie":
                # two classes of one float64 score: groups_tie_free sends the batch down the
                # coupled path (ca_estimate_plan_timings[8])
                assert not plan.stats()["decoupled"]
            if len(case.table) <= 65535:
                _same(case, ro, plan.run_u16(*lim), (name, knobs, lim, "u16"), nodes=False, u16=True)
                if name == "score-tie":
                    assert not plan.stats()["decoupled"]
                elif name == "score-ulp" and KNOBS[knobs][2] == "bucket":
                    # scores one ulp apart are no tie: the same kind of podset does run decoupled
                    assert plan.stats()["decoupled"]
    m.close()


def _long(oracle, name, build, limits, m):
    """One long-run case through a plan, with and without node ordinals."""
    case, refs = _ref(oracle, name, build, limits)
    case.load(m)
    with native.EstimatePlan(m, case.table, case.group_off, case.pod_idx, case.templates) as plan:
        for lim, ro in refs.items():
            _same(case, ro, plan.run(*lim, want_nodes=True), (name, lim, "plan"))
            _same(case, ro, plan.run(*lim, want_nodes=False), (name, lim, "no ordinals"), nodes=False)
    return refs


@pytest.mark.parametrize("rows", ["lds", "hbm"])
def test_estimate_long_run(rows, oracle, monkeypatch):
    """Runs longer than 2^20 pods (k_ffd_chain's `<= (1 << 20)` tests; tests/test_edges_oracle.py
    checks the placements that put each case there).
    long-run: one run of 2^20 + 77 pods that starts with no node open: the closed-form opening
    takes the template's copy count by the integer rec_copies (rem2 > 2^20) and the group
    is longer than 2^20 (k_pdq_sort's mode 3); unlimited (two nodes) and cut at one.
    long-run-rows, limiter 4: a run of 2^20 + 777 that starts with three rows open (the
    scan's integer copy counts and 64-bit sum, three rows alive), and the same run on a
    50-pod template, where four nodes open at once and the `exhausted` check of the last
    row runs with more than 2^20 pods left."""
    _set_rows(monkeypatch, rows)
    m = native.Mirror(0)
    for max_nodes in (0, 1):
        refs = _long(oracle, f"long-run-{max_nodes}", lambda: Q.long_run(max_nodes), [(max_nodes, 1)], m)
        assert int(refs[(max_nodes, 1)].results[0]["n_scheduled"]) == (Q.LONG_RUN_PODS if max_nodes == 0 else 600000)
    refs = _long(oracle, "long-run-rows", Q.long_run_rows, [(Q.LONG_ROWS_MAX_NODES, 1)], m)
    assert refs[(Q.LONG_ROWS_MAX_NODES, 1)].results["n_scheduled"].tolist() == [Q.LONG_ROWS_PODS + 3, 200]
    m.close()


# --------------------------------------------------------------------------
# the same node shapes as mirror rows
# --------------------------------------------------------------------------
def _pair(oracle, rc):
    o, m = oracle.OracleState(), native.Mirror(0)
    for b in (o, m):
        rc.load(b)
    return o, m


def test_rows_check_predicates_and_matrix(oracle):
    rc = Q.row_cluster()
    o, m = _pair(oracle, rc)
    n = len(rc.nodes)
    mat = m.fits_matrix(rc.table)
    seen = set()
    for i in rc.pending.tolist():
        key = rc.table.pods[i].tobytes()
        for pos in range(n):
            if key not in seen:            # verdict and reasons once per distinct record
                assert o.check_predicates(rc.table, i, pos) == m.check_predicates(rc.table, i, pos), (i, pos)
        seen.add(key)
    ref = np.array([[o.check_predicates(rc.table, i, pos)[0] == abi.CA_PRED_OK for pos in range(n)]
                    for i in range(len(rc.table))], np.uint8)
    assert np.array_equal(mat, ref)
    m.close()


@pytest.mark.parametrize("seed", range(2))
def test_rows_fits_any_node_with_placement(seed, oracle):
    """FitsAnyNode for every pending pod, each success placed: rows fill up to the boundary
    and the next pod of the run meets free = req - 1, req, req + 1."""
    rc = Q.row_cluster(seed)
    o, m = _pair(oracle, rc)
    rng = random.Random(f"edges/fits/{seed}")
    n = len(rc.nodes)
    L = seed * 7
    placed = 0
    for i in rc.pending.tolist():
        kind = rng.choice([abi.CA_MATCH_ALL, abi.CA_MATCH_ALL, abi.CA_MATCH_RANGE, abi.CA_MATCH_MASK])
        lo, hi = sorted(rng.sample(range(n + 1), 2))
        mask = np.array([rng.random() < 0.8 for _ in range(n)], np.uint8)
        match = (kind, lo, hi, -1, mask if kind == abi.CA_MATCH_MASK else None)
        ro = o.fits_any_node(rc.table, i, match, L)
        rg = m.fits_any_node(rc.table, i, match, L)
        assert ro == rg, (seed, i, ro, rg)
        L = ro[1]
        if ro[0] >= 0:
            placed += 1
            for b in (o, m):
                b.add_pods(rc.table, [i], [ro[0]])
    assert placed > 50
    m.close()


def _eq_filter(rg, ro, what):
    assert rg.placed == ro.placed, what
    assert np.array_equal(rg.node, ro.node), (what, np.nonzero(rg.node != ro.node)[0][:10])
    assert np.array_equal(rg.pod_id, ro.pod_id), what
    assert np.array_equal(rg.hints, ro.hints), what
    assert (rg.last_index, rg.evals, rg.n_overflowing) == (ro.last_index, ro.evals, ro.n_overflowing), what


@pytest.mark.parametrize("path", ["bitmap", "window"])
def test_rows_filter_out_schedulable(path, oracle, monkeypatch):
    if path == "window":
        monkeypatch.setenv("CASIM_FO_WINDOW", "1")
    rc = Q.row_cluster()
    o, m = _pair(oracle, rc)
    order = rc.pending
    rg = m.filter_out_schedulable(rc.table, order, None, None, 3)
    assert m.filter_stats()["path"] == path
    ro = o.filter_out_schedulable(rc.table, order, None, None, 3)
    _eq_filter(rg, ro, path)
    assert 50 < ro.placed < len(order)
    rg2 = m.filter_out_schedulable(rc.table, order, None, rg.hints, rg.last_index)       # the state left behind
    ro2 = o.filter_out_schedulable(rc.table, order, None, ro.hints, ro.last_index)
    _eq_filter(rg2, ro2, path + " second pass")
    m.close()


def _sweep_args(rc, rng):
    n, P = len(rc.nodes), rc.n_resident
    cands = np.array(rng.sample(range(n), n), np.int32)
    off, moves = [0], []
    for c in cands.tolist():
        moves.extend(np.nonzero(rc.node_of == c)[0].tolist())
        off.append(len(moves))
    hints = np.array([rng.choice([-1, -1, rng.randrange(n)]) for _ in range(P)], np.int32)
    return (cands, np.ones(n, np.uint8), np.zeros(n, np.int32), np.array(off, np.int32),
            np.array(moves, np.int32)), hints


@pytest.mark.parametrize("mode", ["pipeline", "serial"])
@pytest.mark.parametrize("seed", range(2))
def test_rows_find_nodes_to_remove(seed, mode, oracle, monkeypatch):
    if mode == "serial":
        monkeypatch.setenv("CASIM_SWEEP_SERIAL", "1")
    rc = Q.filled_rows(seed)
    o, m = _pair(oracle, rc)
    args, hints = _sweep_args(rc, random.Random(f"edges/sweep/{seed}"))
    ro = o.find_nodes_to_remove(*args, hints, 5)
    rg = m.find_nodes_to_remove(*args, hints, 5)
    assert np.array_equal(ro.results, rg.results), (ro.results, rg.results)
    assert np.array_equal(ro.dest, rg.dest) and np.array_equal(ro.hints, rg.hints)
    assert ro.last_index == rg.last_index
    assert 0 < int(ro.results["removable"].sum()) < len(rc.nodes)
    m.close()


@pytest.mark.parametrize("path", ["chain", "speculative"])
@pytest.mark.parametrize("seed", range(2))
def test_rows_plan_removals(seed, path, oracle, monkeypatch):
    if path == "speculative":
        monkeypatch.setenv("CASIM_PLAN_SPECULATIVE", "1")
    else:
        monkeypatch.delenv("CASIM_PLAN_SPECULATIVE", raising=False)
    rc = Q.filled_rows(seed)
    o, m = _pair(oracle, rc)
    args, hints = _sweep_args(rc, random.Random(f"edges/plan/{seed}"))
    ro = o.plan_removals(*args, hints, 2, 0)
    rg = m.plan_removals(*args, hints, 2, 0)
    assert m.plan_stats()["path"] == path
    assert np.array_equal(ro.results, rg.results), (ro.results, rg.results)
    assert np.array_equal(ro.moves, rg.moves) and np.array_equal(ro.hints, rg.hints)
    assert ro.last_index == rg.last_index
    assert int(ro.results["removable"].sum()) > 0
    n = len(rc.nodes)                     # the committed rows: pod lists and a further FitsAnyNode per pod
    assert [o.node_pods(i) for i in range(n)] == [m.node_pods(i) for i in range(n)]
    L = ro.last_index
    for i in rc.pending.tolist()[:60]:
        a, b = o.fits_any_node(rc.table, i, None, L), m.fits_any_node(rc.table, i, None, L)
        assert a == b, (i, a, b)
        L = a[1]
    m.close()


def test_rows_check_templates(oracle):
    rc = Q.row_cluster()
    o, m = _pair(oracle, rc)
    p = rc.table.pods
    _, first = np.unique(np.array([p[i].tobytes() for i in range(len(p))]), return_index=True)
    samples = np.sort(first).astype(np.int32)
    ro = o.check_templates(rc.table, samples, rc.templates)
    rg = m.check_templates(rc.table, samples, rc.templates)
    assert ro.tobytes() == rg.tobytes()
    v = m.check_templates(rc.table, samples, rc.templates, verdict_only=True)
    assert np.array_equal(v, (ro["type"] == abi.CA_PRED_OK).astype(np.uint8))
    assert 0 < int(v.sum()) < v.size
    m.close()
