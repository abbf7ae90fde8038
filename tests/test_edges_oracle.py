"""CPU guards for the edge-case GPU tests (test_gpu_edges.py, test_gpu_wide.py): against
the oracle alone, the generated inputs really sit where those tests claim, so the GPU
comparisons cannot pass vacuously.

  quantities  every case packs runs of identical pods onto several nodes (or is a stated
              rejection), the boundary cases hold q - 1, q, q pods per node, the tie case
              ties in float64
  wide        the encoded records use the last position of every fixed width, each upper
              part decides verdicts, and both interners agree on the objects
"""
import numpy as np
import pytest

import quantgen as Q
import widegen as WG
from autoscaler_amd import abi


def _estimate(oracle_lib, case):
    o = oracle_lib.OracleState()
    case.load(o)
    r = o.estimate(*case.args())
    o.close()
    return r


def _longest_run(case, r, k):
    """Longest stretch of consecutive scheduled pods of group k with one shape (identical
    records but for their position: what the chain batches as a run)."""
    a, n = int(case.group_off[k]), int(r.results[k]["n_scheduled"])
    sh = case.shape_of[r.sched_pod[a:a + n]]
    best = cur = 1 if n else 0
    for i in range(1, n):
        cur = cur + 1 if sh[i] == sh[i - 1] else 1
        best = max(best, cur)
    return best


@pytest.mark.parametrize("name", list(Q.small_cases()))
def test_quantity_cases_are_not_degenerate(name, oracle_lib):
    case = Q.small_cases()[name]()
    r = _estimate(oracle_lib, case)
    assert (r.results["status"] == abi.CA_OK).all()
    for k, g in enumerate(case.groups):
        n_pods = int(case.group_off[k + 1] - case.group_off[k])
        assert 200 <= n_pods <= 3000, (name, g.tag)
        res = r.results[k]
        if g.reject:        # every pod fails on a fresh node: one empty node, nothing scheduled
            assert (int(res["n_scheduled"]), int(res["nodes_added"]), int(res["node_count"])) == (0, 1, 0), g.tag
            continue
        assert int(res["nodes_added"]) >= 2 and int(res["node_count"]) >= 2, (name, g.tag, res)
        assert _longest_run(case, r, k) >= 2, (name, g.tag)


def test_quotients_need_their_corrections():
    """The float64 closed form (reciprocal, multiply, floor) is one short at free = q * r for
    LOW_REQS and one over at free = q * R - 1 for HIGH_R3 / HIGH_R5, so these cases pass
    only through its correction steps; all values are below 2^53 (exact in float64)."""
    import math
    for r in Q.LOW_REQS.values():
        for q in Q.QS:
            assert math.floor(float(q * r) * (1.0 / float(r))) == q - 1, (r, q)
    for q, r in ((3, Q.HIGH_R3), (5, Q.HIGH_R5)):
        assert q * r - 1 < Q.E53 and math.floor(float(q * r - 1) * (1.0 / float(r))) == q, (r, q)


@pytest.mark.parametrize("req", [Q.EXAMPLE_REQS, Q.LOW_REQS], ids=["example", "low"])
@pytest.mark.parametrize("dim", Q.DIMS)
@pytest.mark.parametrize("q", Q.QS)
def test_quot_boundary_counts(q, dim, req, oracle_lib):
    """free = q * req - 1, q * req, q * req + 1: every node that holds boundary-shape pods
    holds exactly q - 1, q, q of them (but the last one opened), and none when q - 1 == 0."""
    case = Q.quot_boundary(q, dim, req)
    r = _estimate(oracle_lib, case)
    for k, want in enumerate((q - 1, q, q)):
        a, n = int(case.group_off[k]), int(r.results[k]["n_scheduled"])
        big = case.shape_of[r.sched_pod[a:a + n]] == 3 * k          # shape 0 of group k
        per_node = np.bincount(r.sched_node[a:a + n][big], minlength=1)
        per_node = per_node[per_node > 0]
        if want == 0:
            assert len(per_node) == 0
            continue
        assert len(per_node) >= 2
        assert (per_node[:-1] == want).all() and per_node[-1] <= want, (q, dim, k, per_node)


def _scores(case, k):
    """float64 score of every shape of group k on its template (binpacking_estimator.go:164-193)."""
    t = case.templates[k]["node"]
    out = {}
    for s in sorted(set(case.shape_of[case.group_off[k]:case.group_off[k + 1]].tolist())):
        sh = case.shapes[s]
        sc = 0.0
        c = sh.cpu if sh.score_cpu is None else sh.score_cpu
        m = sh.mem if sh.score_mem is None else sh.score_mem
        if int(t["alloc_milli_cpu"]) > 0:
            sc += float(c) / float(int(t["alloc_milli_cpu"]))
        if int(t["alloc_memory"]) > 0:
            sc += float(m) / float(int(t["alloc_memory"]))
        out[s] = (sc, (c, m))
    return out


def test_score_edges_tie_and_ulp():
    tie = Q.score_tie()
    for k in range(len(tie.groups)):
        sc = sorted(_scores(tie, k).values())
        equal = [(a, b) for a, b in zip(sc, sc[1:]) if a[0] == b[0]]
        assert equal and all(a[1] != b[1] for a, b in equal), sc      # one float64, different integers
    ulp = Q.score_ulp()
    sc = sorted(v[0] for v in _scores(ulp, 0).values())
    assert any(b == np.nextafter(a, np.inf) for a, b in zip(sc, sc[1:])), sc
    assert len(set(sc)) == len(sc)
    skip = Q.score_skip()
    assert int(skip.templates[0]["node"]["alloc_milli_cpu"]) == 0 and int(skip.templates[1]["node"]["alloc_memory"]) == 0


def test_near_2_53_groups_straddle_the_float64_path():
    """Group 0 keeps every free value and request below 2^53 (run_div's f64 flag holds for
    all its runs); every later group has a free value or requests at or above it."""
    case = Q.near_2_53()
    p = case.table.pods

    def bound(k):
        t = case.templates[k]
        return max(int(t["node"]["alloc_milli_cpu"]) - int(t["used_milli_cpu"]),
                   int(t["node"]["alloc_memory"]) - int(t["used_memory"]),
                   int(t["node"]["alloc_ephemeral"]) - int(t["used_ephemeral"]))

    def max_req(k):
        sl = slice(int(case.group_off[k]), int(case.group_off[k + 1]))
        return int(max(p["req_milli_cpu"][sl].max(), p["req_memory"][sl].max(), p["req_ephemeral"][sl].max()))

    assert bound(0) == Q.E53 - 1 and max_req(0) == Q.E53 - 1
    assert bound(1) == Q.E53 and bound(2) == Q.E53 + 1
    assert bound(3) == Q.E53 - 1 and max_req(3) == Q.E53 + 1
    assert {max_req(1), max_req(2)} == {Q.E53, Q.E53 + 1}
    huge = Q.huge()
    ph = huge.table.pods
    assert all(bound_ >= 1 << 59 for bound_ in
               (int(t["node"]["alloc_milli_cpu"]) - int(t["used_milli_cpu"]) for t in huge.templates))
    assert int(ph["req_milli_cpu"].max()) > Q.E53 and int(ph["req_milli_cpu"][ph["req_milli_cpu"] > 0].min()) > 1 << 40
    # no sum the oracle forms reaches 2^62: a node's requests never exceed its allocatable
    for t in huge.templates:
        assert max(int(t["node"][f]) for f in ("alloc_milli_cpu", "alloc_memory", "alloc_ephemeral")) < 1 << 62


def test_long_run_crosses_2_20(oracle_lib):
    """long-run: the group is one run longer than 2^20 with no node open when it starts, so
    the template's copy count (600000) is taken with all 2^20 + 77 pods left; two nodes hold
    the run, one under max_nodes 1.  (When the second node opens only 448653 are left: the
    row scan never runs with more than 2^20 here; long-run-rows below is for that.)"""
    case = Q.long_run(0)
    assert len(case.table) == Q.LONG_RUN_PODS > 1 << 20
    r = _estimate(oracle_lib, case)
    res = r.results[0]
    assert (int(res["n_scheduled"]), int(res["nodes_added"])) == (Q.LONG_RUN_PODS, 2)
    per_node = np.bincount(r.sched_node[:Q.LONG_RUN_PODS])
    assert per_node.tolist() == [600000, Q.LONG_RUN_PODS - 600000]
    r1 = _estimate(oracle_lib, Q.long_run(1))
    assert (int(r1.results[0]["n_scheduled"]), int(r1.results[0]["nodes_added"])) == (600000, 1)


def test_long_run_rows_meets_open_rows_and_the_limiter(oracle_lib):
    """long-run-rows under its limiter of 4.  Group 0: the three big pods come first, one per
    node, so the run of 2^20 + 777 starts with three rows open and nothing of it placed; it
    fills them in rotation (300001 copies each: the scan ran over rows with room while more
    than 2^20 were left) and the fourth grant takes the rest.  Group 1: four 50-pod nodes,
    then the limiter ends the group with more than 2^20 pods of the run left."""
    case = Q.long_run_rows()
    n = Q.LONG_ROWS_PODS
    assert n > 1 << 20 and case.max_nodes == 4
    r = _estimate(oracle_lib, case)
    g0, g1 = r.results
    assert (int(g0["n_scheduled"]), int(g0["nodes_added"])) == (n + 3, 4)
    sp, sn = r.sched_pod[:n + 3], r.sched_node[:n + 3]
    assert case.shape_of[sp[:3]].tolist() == [0, 0, 0] and sn[:3].tolist() == [0, 1, 2]
    assert (case.shape_of[sp[3:]] == 1).all()
    assert sn[3:9].tolist() == [0, 1, 2, 0, 1, 2]                        # placed on the open rows, in rotation
    first_on_3 = int(np.argmax(sn == 3))
    assert first_on_3 == 3 + 3 * 300001 and np.bincount(sn).tolist() == [300002, 300002, 300002, n - 3 * 300001]
    a = int(case.group_off[1])
    assert (int(g1["n_scheduled"]), int(g1["nodes_added"])) == (200, 4)
    assert np.bincount(r.sched_node[a:a + 200]).tolist() == [50, 50, 50, 50]
    assert n - 200 > 1 << 20                                            # left when the limiter cuts the run


def test_row_clusters_fit_the_small_drivers(oracle_lib):
    for seed in range(2):
        for rc in (Q.row_cluster(seed), Q.filled_rows(seed)):
            assert len(rc.nodes) <= 64 and len(rc.table) <= 400
        rc = Q.filled_rows(seed)
        assert rc.n_resident > len(rc.nodes) + 50
        # every resident was placed by NodeResourcesFit's rule: no row is overcommitted
        # beyond what its shape states (negative free values come from the node shapes)
        o = oracle_lib.OracleState()
        rc.load(o)
        base = Q.row_cluster(seed)
        ob = oracle_lib.OracleState()
        base.load(ob)
        for i in range(len(rc.nodes)):
            assert all(a <= b for a, b in zip(o.node_state(i), ob.node_state(i)))
            if ob.node_state(i)[0] >= 0 and ob.node_state(i)[1] >= 0 and ob.node_state(i)[2] >= 0:
                assert min(o.node_state(i)[:3]) >= 0


# --------------------------------------------------------------------------
# wide vocabulary
# --------------------------------------------------------------------------
_WIDE = {}


def _wide(size, extra=False):
    key = (size, extra)
    if key not in _WIDE:
        seed, n, sc, pe = size
        case = WG.wide_case(seed, n, sc, pe, extra_taint=extra)
        _WIDE[key] = (case, WG.encode(case))
    return _WIDE[key]


def _wide_outputs(oracle_lib, e, seed):
    """check_predicates of every (pending pod, node), and the batched calls."""
    o = oracle_lib.OracleState()
    e.load(o)
    n = len(e.node_recs)
    cp = np.array([[o.check_predicates(e.table, int(i), pos) for pos in range(n)] for i in e.pending])
    est = o.estimate(e.table, e.group_off, e.pod_idx, e.templates, 0, 3)
    args, hints = WG.sweep_args(e, seed)
    sw = o.find_nodes_to_remove(*args, hints, 2)
    o.close()
    o = oracle_lib.OracleState()
    e.load(o)
    table, order, owners, fh = WG.filter_args(e, plain=False)
    fo = o.filter_out_schedulable(table, order, owners, fh, 3)
    o.close()
    return cp, est, sw, fo


@pytest.mark.parametrize("size", WG.SIZES, ids=[f"n{s[1]}" for s in WG.SIZES])
def test_wide_cases_reach_the_last_positions(size):
    case, e = _wide(size)
    assert 12 <= len(case.nodes) <= 64 and 40 <= len(case.pods) <= 400
    it = e.it
    assert (len(it.pairs), len(it.keys), len(it.int_keys), len(it.taints), len(it.ports), len(it.scalars)) == \
        (256, 64, 4, 63, 128, 8)
    for u in (it.taints, it.pairs, it.keys, it.int_keys, it.ports, it.scalars):
        assert not u.overflow, u.what
    assert not it.port_groups_over
    assert not (e.table.pods["flags"] & (abi.CA_POD_OUT_OF_SCOPE | abi.CA_POD_HOSTNAME_DEPENDENT)).any()
    for part, uses in WG.upper_bits(e).items():
        assert all(uses.values()), (part, uses)
    # the last position of each width, on a live object
    n, p, r = e.node_recs, e.table.pods, e.table.reqs
    top = np.uint64(1) << np.uint64(63)
    assert (n["label_pairs"][:, 3] & top).any() or (p["node_selector"][:, 3] & top).any() or (r["pairs"][:, 3] & top).any()
    assert any("0.0.0.0" == ip for ip, _, _ in it.ports.ids)              # wildcard groups


@pytest.mark.parametrize("part", WG.UPPER_PARTS)
@pytest.mark.parametrize("size", WG.SIZES, ids=[f"n{s[1]}" for s in WG.SIZES])
def test_wide_upper_parts_decide_verdicts(size, part, oracle_lib):
    """With only that upper part cleared the oracle answers differently: in
    CheckPredicates, and in at least one of Estimate, FilterOutSchedulable and the sweep.
    So a device path that lost the part could not pass test_gpu_wide.py."""
    _, e = _wide(size)
    if ("outputs", size) not in _WIDE:
        _WIDE[("outputs", size)] = _wide_outputs(oracle_lib, e, size[0])
    cp, est, sw, fo = _WIDE[("outputs", size)]
    cp2, est2, sw2, fo2 = _wide_outputs(oracle_lib, WG.clear_upper(e, part), size[0])
    assert (cp != cp2).any(), part
    assert (not np.array_equal(est.results, est2.results) or not np.array_equal(fo.node, fo2.node)
            or not (np.array_equal(sw.results, sw2.results) and np.array_equal(sw.dest, sw2.dest))), part


@pytest.mark.parametrize("size", WG.SIZES[:2], ids=[f"n{s[1]}" for s in WG.SIZES[:2]])
def test_wide_taint_past_the_width(size, oracle_lib):
    """One taint class past the 63: the last node carries bit 63, pods that tolerate it
    carry bit 63, nobody is out of scope (intern.py: one overflow taint is tolerated
    entirely or not at all), and only pods with bit 63 pass TaintToleration there."""
    case, e = _wide(size, extra=True)
    assert e.it.taints.overflow == {WG.OVER_TAINT} and len(e.it.taints) == 63
    assert not (e.table.pods["flags"] & abi.CA_POD_OUT_OF_SCOPE).any()
    assert int(e.node_recs["taints"][-1]) >> 63 == 1 and not (e.node_recs["taints"][:-1] >> np.uint64(63)).any()
    tol = (e.table.pods["tolerated_taints"] >> np.uint64(63)).astype(bool)
    assert tol.any() and not tol.all()
    o = oracle_lib.OracleState()
    e.load(o)
    last = len(e.node_recs) - 1
    for i in range(len(e.table)):
        t, plugin, _, taint = o.check_predicates(e.table, i, last)
        if not tol[i] and plugin in (abi.CA_PLUGIN_NONE, abi.CA_PLUGIN_TAINT_TOLERATION) and t != abi.CA_PRED_OK:
            assert plugin == abi.CA_PLUGIN_TAINT_TOLERATION
        if not tol[i]:
            assert t != abi.CA_PRED_OK
    o.close()


@pytest.mark.parametrize("extra", [False, True], ids=["inside", "taint63"])
@pytest.mark.parametrize("size", WG.SIZES[:2], ids=[f"n{s[1]}" for s in WG.SIZES[:2]])
def test_wide_objects_intern_alike_in_c(size, extra):
    """intern.py and csrc/intern.cpp give the wide objects the same universes and fields."""
    from test_intern_c import _compare
    case, _ = _wide(size, extra)
    _compare(case.nodes, case.pods, case.templates)
