"""HIP path vs the CPU restatement on clusters whose interned ids reach the last position
of every fixed width (tests/widegen.py): label pairs up to 255 (four words), Exists keys up
to 63, taint classes up to 62 and the overflow bit 63, host ports up to 127 (two words),
scalar slots up to 7, Gt/Lt keys up to 3.  A kernel, an LDS staging loop or a host row
builder that dropped or mis-indexed an upper word would change these verdicts
(tests/test_edges_oracle.py checks on the CPU that each upper part decides some).  Exact
equality, compared as the random-cluster tests compare."""
import random

import numpy as np
import pytest

import widegen as WG
from autoscaler_amd import abi, native

pytestmark = pytest.mark.gpu

CASES = [(s, n, sc, pe, False) for s, n, sc, pe in WG.SIZES] + [(s, n, sc, pe, True) for s, n, sc, pe in WG.SIZES[:2]]
IDS = [f"n{n}-p{sc + pe}" + ("-taint63" if x else "") for _, n, sc, pe, x in CASES]


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


_ENC = {}


def _enc(case) -> WG.Encoded:
    if case not in _ENC:
        seed, n, sc, pe, extra = case
        e = WG.encode(WG.wide_case(seed, n, sc, pe, extra_taint=extra))
        it = e.it
        over = {u.what: u.overflow for u in (it.taints, it.pairs, it.keys, it.int_keys, it.ports, it.scalars)}
        if extra:
            assert over.pop("taint classes") == {WG.OVER_TAINT}
            assert int(e.node_recs["taints"][-1]) >> 63 == 1
        assert not any(over.values()) and not it.port_groups_over, over
        assert not (e.table.pods["flags"] & abi.CA_POD_OUT_OF_SCOPE).any()
        _ENC[case] = e
    return _ENC[case]


def _pair(oracle, e):
    o, m = oracle.OracleState(), native.Mirror(0)
    for b in (o, m):
        e.load(b)
    return o, m


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_check_predicates(case, oracle):
    e = _enc(case)
    o, m = _pair(oracle, e)
    n = len(e.node_recs)
    ref = np.zeros((len(e.table), n), np.uint8)
    terms, reqs = e.table.terms, e.table.reqs
    seen = set()
    for i in range(len(e.table)):                   # every pod, scheduled ones too, against every node
        p = e.table.pods[i].copy()
        p["similar_class"] = 0
        tf, tc = int(p["aff_term_first"]), max(int(p["aff_term_count"]), 0)
        rows = b"".join(reqs[int(t["first"]):int(t["first"]) + int(t["count"])].tobytes() for t in terms[tf:tf + tc])
        p["aff_term_first"] = 0
        key = (p.tobytes(), tc, rows)               # the record and the requirement rows it points to
        for pos in range(n):
            ro = o.check_predicates(e.table, i, pos)
            ref[i, pos] = ro[0] == abi.CA_PRED_OK
            if key not in seen:                     # all four fields, once per distinct pod
                assert ro == m.check_predicates(e.table, i, pos), (i, pos)
        seen.add(key)
    assert np.array_equal(m.fits_matrix(e.table), ref)
    if case[4]:                                     # the node with a taint past the width: tolerate-all pods only
        last = n - 1
        tol_all = (e.table.pods["tolerated_taints"] >> np.uint64(63)).astype(bool)
        assert tol_all.any() and not tol_all.all()
        assert not ref[~tol_all, last].any()
    m.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_fits_any_node(case, oracle):
    e = _enc(case)
    o, m = _pair(oracle, e)
    rng = random.Random(f"wide/fits/{case}")
    n = len(e.node_recs)
    L = 0
    for i in e.pending.tolist()[:150]:
        kind = rng.choice([abi.CA_MATCH_ALL, abi.CA_MATCH_RANGE, abi.CA_MATCH_MASK])
        mask = np.array([rng.random() < 0.7 for _ in range(n)], np.uint8)
        lo, hi = sorted(rng.sample(range(n + 1), 2))
        match = (kind, lo, hi, rng.choice([-1, rng.randrange(n)]), mask if kind == abi.CA_MATCH_MASK else None)
        if rng.random() < 0.2:
            L = rng.randrange(0, 1000)
        ro = o.fits_any_node(e.table, i, match, L)
        rg = m.fits_any_node(e.table, i, match, L)
        assert ro == rg, (i, ro, rg)
        L = ro[1]
        if ro[0] >= 0 and rng.random() < 0.5:       # place it: ports and scalars of the row move on
            for b in (o, m):
                b.add_pods(e.table, [i], [ro[0]])
    m.close()


@pytest.mark.parametrize("knobs", ["default", "per-pod", "hbm", "merge"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_estimate(case, knobs, oracle, monkeypatch):
    """Templates with wide labels, taints, used ports and scalars: ca_estimate_batch and a
    plan in every output mode."""
    monkeypatch.setenv("CASIM_RUN_BATCH", "0" if knobs == "per-pod" else "1")
    if knobs == "hbm":                              # read by presence: any value selects the HBM-slab rows
        monkeypatch.setenv("CASIM_CHAIN_GLOBAL", "1")
    else:
        monkeypatch.delenv("CASIM_CHAIN_GLOBAL", raising=False)
    monkeypatch.setenv("CASIM_SORT", "merge" if knobs == "merge" else "bucket")
    e = _enc(case)
    o, m = _pair(oracle, e)
    args = (e.table, e.group_off, e.pod_idx, e.templates)
    with native.EstimatePlan(m, *args) as plan:
        for max_nodes, L0 in ((0, 3), (2, 77)):
            ro = o.estimate(*args, max_nodes, L0)
            assert (ro.results["status"] == abi.CA_OK).all()
            outs = [(m.estimate(*args, max_nodes, L0), True), (plan.run(max_nodes, L0, want_nodes=True), True),
                    (plan.run(max_nodes, L0, want_nodes=False), False)]
            h = plan.run_u16(max_nodes, L0)
            h.sched_pod = np.where(h.sched_pod == 0xFFFF, -1, h.sched_pod.astype(np.int32))
            outs.append((h, False))
            for g, nodes in outs:
                assert np.array_equal(ro.results, g.results), (max_nodes, ro.results, g.results)
                assert ro.last_index == g.last_index
                for k in range(len(e.templates)):
                    a, cnt = int(e.group_off[k]), int(ro.results[k]["n_scheduled"])
                    assert np.array_equal(ro.sched_pod[a:a + cnt], g.sched_pod[a:a + cnt]), k
                    if nodes:
                        assert np.array_equal(ro.sched_node[a:a + cnt], g.sched_node[a:a + cnt]), k
    m.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_check_templates(case, oracle):
    e = _enc(case)
    o, m = _pair(oracle, e)
    ro = o.check_templates(e.table, e.pending, e.templates)
    rg = m.check_templates(e.table, e.pending, e.templates)
    assert ro.tobytes() == rg.tobytes()
    v = m.check_templates(e.table, e.pending, e.templates, verdict_only=True)
    assert np.array_equal(v, (ro["type"] == abi.CA_PRED_OK).astype(np.uint8))
    m.close()


def _eq_filter(rg, ro, what):
    assert rg.placed == ro.placed, what
    assert np.array_equal(rg.node, ro.node), (what, np.nonzero(rg.node != ro.node)[0][:10])
    assert np.array_equal(rg.pod_id, ro.pod_id), what
    assert np.array_equal(rg.hints, ro.hints), what
    assert (rg.last_index, rg.evals, rg.n_overflowing) == (ro.last_index, ro.evals, ro.n_overflowing), what


@pytest.mark.parametrize("path", ["bitmap", "window", "window-all"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_filter_out_schedulable(case, path, oracle, monkeypatch):
    """bitmap: the pending records without their host ports and extended resources (the
    feasibility-bitmap walk's scope: labels, keys, taints and Gt/Lt in its static classes);
    window: the same records through the window sequencer; window-all: the pending pods as
    they are (ports and scalars against the rows).  The rows carry the scheduled pods' ports
    and scalars in all three."""
    if path == "window":
        monkeypatch.setenv("CASIM_FO_WINDOW", "1")
    e = _enc(case)
    o, m = _pair(oracle, e)
    table, order, owners, hints = WG.filter_args(e, plain=path != "window-all")
    rg = m.filter_out_schedulable(table, order, owners, hints, 3)
    assert m.filter_stats()["path"] == path.split("-")[0]
    ro = o.filter_out_schedulable(table, order, owners, hints, 3)
    _eq_filter(rg, ro, path)
    assert 0 < ro.placed < len(order)
    rg2 = m.filter_out_schedulable(table, order, owners, rg.hints, rg.last_index)      # the state left behind
    ro2 = o.filter_out_schedulable(table, order, owners, ro.hints, ro.last_index)
    _eq_filter(rg2, ro2, path + " second pass")
    m.close()


@pytest.mark.parametrize("mode", ["pipeline", "serial"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_find_nodes_to_remove(case, mode, oracle, monkeypatch):
    if mode == "serial":
        monkeypatch.setenv("CASIM_SWEEP_SERIAL", "1")
    e = _enc(case)
    o, m = _pair(oracle, e)
    args, hints = WG.sweep_args(e, case[0])
    ro = o.find_nodes_to_remove(*args, hints, 2)
    rg = m.find_nodes_to_remove(*args, hints, 2)
    assert np.array_equal(ro.results, rg.results), (ro.results, rg.results)
    assert np.array_equal(ro.dest, rg.dest) and np.array_equal(ro.hints, rg.hints)
    assert ro.last_index == rg.last_index
    assert int(ro.results["removable"].sum()) > 0
    m.close()


@pytest.mark.parametrize("path", ["chain", "speculative"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_plan_removals(case, path, oracle, monkeypatch):
    """speculative: the pods as they are (those with host ports or extended resources are
    outside the device chain's scope).  chain: every pod stripped of ports and extended
    resources, so the device chain runs, over the wide labels, keys, taints and Gt/Lt."""
    e = _enc(case)
    if path == "speculative":
        monkeypatch.setenv("CASIM_PLAN_SPECULATIVE", "1")
    else:
        monkeypatch.delenv("CASIM_PLAN_SPECULATIVE", raising=False)
        e = WG.plain_encoded(e)
    o, m = _pair(oracle, e)
    args, hints = WG.sweep_args(e, case[0])
    ro = o.plan_removals(*args, hints, 2, 0)
    rg = m.plan_removals(*args, hints, 2, 0)
    assert m.plan_stats()["path"] == path
    assert np.array_equal(ro.results, rg.results), (ro.results, rg.results)
    assert np.array_equal(ro.moves, rg.moves) and np.array_equal(ro.hints, rg.hints)
    assert ro.last_index == rg.last_index
    assert int(ro.results["removable"].sum()) > 0
    n = len(e.node_recs)                  # the committed snapshot: pod lists, then a FitsAnyNode per pending pod
    assert [o.node_pods(i) for i in range(n)] == [m.node_pods(i) for i in range(n)]
    L = ro.last_index
    for i in e.pending.tolist()[:60]:
        a, b = o.fits_any_node(e.table, i, None, L), m.fits_any_node(e.table, i, None, L)
        assert a == b, (i, a, b)
        L = a[1]
    m.close()
