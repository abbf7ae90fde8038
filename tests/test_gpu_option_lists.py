"""The Estimate plan built from the option matrix (ca_estimate_plan_create_options, lists made
in device memory by k_option_lists) against the plan built from the same lists made on the
host (optgen.lists_of): the lists byte for byte, every run mode's outputs, the readers of the
resident lists, the error codes, and the facades that choose between the two forms."""
import numpy as np
import pytest

import optgen
from autoscaler_amd import abi, native, runonce, workloads as W

pytestmark = pytest.mark.gpu

LIMITS = [0, 3]
KNOBS = {"default": {}, "coupled": {"CASIM_GO_DECOUPLE": "0"}, "merge": {"CASIM_SORT": "merge"}}


@pytest.fixture(scope="module")
def loaded():
    """One mirror and one resident podset per workload (most cases share optgen.base())."""
    made = {}

    def get(w):
        if id(w) not in made:
            m = native.Mirror(0)
            W.load_estimate(m, w)
            made[id(w)] = (m, m.podset(w.table))
        return made[id(w)]
    yield get
    for m, ps in made.values():
        ps.close()
        m.close()


def _score_classes(table):
    """The podset's score classes: pods of equal (score_milli_cpu, score_memory), numbered in
    first-occurrence order (ca_podset)."""
    sc = np.stack([table.pods["score_milli_cpu"], table.pods["score_memory"]], 1)
    _, first, inv = np.unique(sc, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int32)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first), dtype=np.int32)
    return rank[np.asarray(inv).reshape(-1)]


def _scheduled(results, off, *arrays):
    """The defined part of a run's lists: the first n_scheduled entries of every group that ran
    (what the project's parity tests compare; the tail of a published list is unspecified)."""
    out = []
    for a in arrays:
        out.append(b"".join(a[int(off[k]):int(off[k]) + int(r["n_scheduled"])].tobytes()
                            for k, r in enumerate(results) if int(r["status"]) == 0))
    return tuple(out)


def _modes(plan, max_nodes, L0=1):
    off = plan.group_off
    g = plan.run(max_nodes, L0, want_nodes=True)
    st = plan.stats()
    p = plan.run(max_nodes, L0, want_nodes=False)
    d = plan.run(max_nodes, L0, device_results=True)
    fetched = plan.fetch().copy()
    h = plan.run_u16(max_nodes, L0)
    blob = {"nodes": (g.results.tobytes(), _scheduled(g.results, off, g.sched_pod, g.sched_node), g.last_index),
            "host32": (p.results.tobytes(), _scheduled(p.results, off, p.sched_pod), p.last_index),
            "device": (d.results.tobytes(), _scheduled(d.results, off, fetched), d.last_index),
            "u16": (h.results.tobytes(), _scheduled(h.results, off, h.sched_pod), h.last_index)}
    return blob, (st["sorts"], st["sort_parts"], st["decoupled"]), int(g.results["n_scheduled"].sum())


def _plans(loaded, name):
    _, w, eg_off, eg_pod, ok, tm, _ = optgen.case(name)
    m, ps = loaded(w)
    off, idx = optgen.lists_of(eg_off, eg_pod, ok)
    a = native.EstimatePlan(m, w.table, off, idx, tm, podset=ps)
    b = native.EstimatePlan.from_options(m, ps, eg_off, eg_pod, ok, tm)
    return w, off, idx, a, b


@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("name", optgen.CASE_NAMES)
def test_lists_and_runs_equal_the_host_form(name, knob, loaded, monkeypatch):
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)                       # (read when the plan is created / run)
    w, off, idx, a, b = _plans(loaded, name)
    with a, b:
        assert b.group_off.dtype == np.int32 and b.group_off.tobytes() == off.tobytes()
        assert b.total == len(idx) and b.G == a.G
        got_idx, got_cls = b.fetch_lists()
        assert got_idx.tobytes() == idx.tobytes()
        cls = _score_classes(w.table)
        bucket = knob != "merge" and int(cls.max()) < 4096         # (estimate.hip CLS_MAX score classes)
        assert (got_cls is not None) == (bucket or len(idx) == 0), (name, knob)
        if bucket:
            assert got_cls.tobytes() == cls[idx].tobytes()         # the class column at cls[pod_idx]
        if name == "lengths":
            a_idx, a_cls = a.fetch_lists()
            assert a_idx.tobytes() == idx.tobytes()
            assert bucket == (a_cls is not None) and (not bucket or a_cls.tobytes() == cls[idx].tobytes())
        for max_nodes in LIMITS:
            ra, sa, na = _modes(a, max_nodes)
            rb, sb, _ = _modes(b, max_nodes)
            if max_nodes == 0 and w is optgen.base():
                assert na == len(idx)                              # every pod fits its template: whole lists compared
            for mode in ra:
                assert ra[mode] == rb[mode], (name, knob, max_nodes, mode)
            assert sa == sb, (name, knob, max_nodes, sa, sb)
            if knob == "coupled":
                assert not sb[2]
            elif knob == "default" and w is optgen.base() and len(idx):
                assert sb[2], (name, "the tie-free uniform podset runs decoupled")


def test_shared_sorts_are_found_from_the_rows(loaded):
    """Groups 0, 2 and 3 hold one row on templates that rank the classes alike: one sort; group
    1 (another cpu : memory ratio) and group 4 (another row) sort for themselves."""
    _, _, _, a, b = _plans(loaded, "equal_rows")
    with a, b:
        for plan in (a, b):
            plan.run(0, 0)
            st = plan.stats()
            assert st["decoupled"] and st["sorts"] == 3, st


def test_readers_of_the_resident_lists(loaded):
    w, off, idx, a, b = _plans(loaded, "groups_300")
    price = np.random.default_rng(3).random(len(w.table))
    with a, b:
        outs = []
        for plan in (a, b):
            r = plan.run(2, 0, device_results=True)
            cpu, mem = plan.option_sums()
            groups = [g for g in range(plan.G) if g != 7][:40]
            miss = plan.groups_missing_pods(7, groups)
            outs.append((r.results.tobytes(), cpu.tobytes(), mem.tobytes(), plan.option_price_sums(price).tobytes(),
                         [plan.fetch_group(g).tobytes() for g in (0, 7, 150, 299)],
                         miss[0].tobytes(), miss[1].tobytes(), plan.chain_info(),
                         plan.rebase(r.results.copy(), 5)))
        assert outs[0] == outs[1]
        assert b.stats()["option_lists_ms"] > 0 and a.stats()["option_lists_ms"] == 0


def test_error_codes(loaded):
    w = optgen.base()
    m, ps = loaded(w)
    tm = optgen._templates(2)
    P = len(w.table)

    def status(eg_off, eg_pod, ok, templates=tm):
        try:
            native.EstimatePlan.from_options(m, ps, eg_off, eg_pod, ok, templates).close()
        except native.CasimError as e:
            return e.status
        return abi.CA_OK

    ok = np.ones((2, 2), np.uint8)
    pods = np.arange(6, dtype=np.int32)
    assert status([0, 2, 6], pods, ok) == abi.CA_OK
    assert status([1, 2, 6], pods, ok) == abi.CA_EINVAL                    # eg_off[0] != 0
    assert status([0, 4, 3], pods, ok) == abi.CA_EINVAL                    # decreasing
    for bad in (-1, P, 2**31 - 1):
        q = pods.copy()
        q[3] = bad
        assert status([0, 2, 6], q, ok) == abi.CA_EINVAL                   # outside the pod set
    # an entry outside the pod set is refused even where no row uses its group
    q = pods.copy()
    q[5] = P
    assert status([0, 2, 6], q, np.array([[1, 0], [1, 0]], np.uint8)) == abi.CA_EINVAL
    # 40 000 rows of one group of 70 000 pods: 2.8e9 items do not fit int32
    n, G = 70_000, 40_000
    big = (np.arange(n) % P).astype(np.int32)
    assert status([0, n], big, np.ones((G, 1), np.uint8), np.zeros(G, abi.TEMPLATE_DTYPE)) == abi.CA_EINVAL
    # a podset of another mirror: what the host constructor returns
    other = native.Mirror(0)
    W.load_estimate(other, w)
    off, idx = optgen.lists_of([0, 2, 6], pods, ok)
    try:
        native.EstimatePlan(other, w.table, off, idx, tm, podset=ps).close()
        want = abi.CA_OK
    except native.CasimError as e:
        want = e.status
    try:
        native.EstimatePlan.from_options(other, ps, [0, 2, 6], pods, ok, tm).close()
        got = abi.CA_OK
    except native.CasimError as e:
        got = e.status
    other.close()
    assert got == want


def test_empty_inputs(loaded):
    w = optgen.base()
    m, ps = loaded(w)
    tm = optgen._templates(3)
    with native.EstimatePlan.from_options(m, ps, [0], np.zeros(0, np.int32), np.zeros((3, 0), np.uint8), tm) as b:
        assert b.group_off.tolist() == [0, 0, 0, 0]
        r = b.run(0, 4)
        with native.EstimatePlan(m, w.table, [0, 0, 0, 0], np.zeros(0, np.int32), tm, podset=ps) as a:
            ra = a.run(0, 4)
        assert r.results.tobytes() == ra.results.tobytes() and r.last_index == ra.last_index
    with native.EstimatePlan.from_options(m, ps, [0, 3], [0, 1, 2], np.zeros((0, 1), np.uint8), tm[:0]) as b:
        assert b.group_off.tolist() == [0] and b.G == 0


def test_scope_blocker_behaves_as_with_host_lists():
    """A snapshot that holds a pod with required anti-affinity: both constructors and their runs
    answer alike."""
    _, w, eg_off, eg_pod, ok, tm, _ = optgen.case("long_group")
    m = native.Mirror(0)
    W.load_estimate(m, w)
    blocker = W.resource_pods(np.array([100]), np.array([W.MI]))
    blocker["flags"] |= abi.CA_POD_REQUIRED_ANTI_AFFINITY
    m.add_pods(abi.PodTable(blocker), [0], [0])
    assert m.scope_blockers() == 1
    off, idx = optgen.lists_of(eg_off, eg_pod, ok)
    seen = []
    for make in (lambda: native.EstimatePlan(m, w.table, off, idx, tm),
                 lambda: native.EstimatePlan.from_options(m, w.table, eg_off, eg_pod, ok, tm)):
        try:
            with make() as plan:
                r = plan.run(0, 0)
                seen.append(("ran", r.results.tobytes(), _scheduled(r.results, off, r.sched_pod), r.last_index))
        except native.CasimError as e:
            seen.append(("error", e.status))
    m.close()
    assert seen[0] == seen[1], seen


def test_estimate_options_one_shot(loaded):
    _, w, eg_off, eg_pod, ok, tm, _ = optgen.case("c4")
    m, ps = loaded(w)
    off, idx = optgen.lists_of(eg_off, eg_pod, ok)
    want = m.estimate(w.table, off, idx, tm, w.max_nodes, 2, podset=ps)
    for src in (ps, w.table):
        got, group_off = m.estimate_options(src, eg_off, eg_pod, ok, tm, w.max_nodes, 2)
        assert group_off.tobytes() == off.tobytes()
        assert (got.results.tobytes(), _scheduled(got.results, off, got.sched_pod, got.sched_node), got.last_index) == \
               (want.results.tobytes(), _scheduled(want.results, off, want.sched_pod, want.sched_node), want.last_index)


# -- facades ------------------------------------------------------------------------------

def _facade_inputs():
    import test_gpu_price as tp
    from autoscaler_amd.expander import ChainStrategy, LeastWaste, MostPods

    class _First:
        def BestOption(self, options, node_infos):          # noqa: N802
            return options[0] if options else None
    return tp, lambda seed: ChainStrategy([LeastWaste(), MostPods()], _First())


@pytest.mark.parametrize("chain_kind", ["price", "waste"])
@pytest.mark.parametrize("seed", range(3))
def test_compute_best_expansion_option_either_form(seed, chain_kind):
    from autoscaler_amd.clustersnapshot import ClusterSnapshot
    from autoscaler_amd.estimator import ThresholdBasedEstimationLimiter
    from autoscaler_amd.predicatechecker import SchedulerBasedPredicateChecker
    from autoscaler_amd.scaleup import BuildPodGroups, ComputeBestExpansionOption
    tp, waste = _facade_inputs()
    res = []
    for form in ("host", "device"):
        nodes, pods, infos = tp._options_inputs(seed)
        snap = ClusterSnapshot(native.Mirror(0))
        snap.AddNodes(nodes)
        pc = SchedulerBasedPredicateChecker()
        pc.last_index = seed % 3
        chain = tp._chain(seed) if chain_kind == "price" else waste(seed)
        best, feas = ComputeBestExpansionOption(snap, pc, BuildPodGroups(pods), infos,
                                                ThresholdBasedEstimationLimiter(max_nodes=7), chain, option_lists=form)
        res.append((None if best is None else (best.node_group, best.node_count, [p.name for p in best.pods]),
                    feas.tobytes(), pc.last_index, pc.evals))
        snap.backend.close()
    assert res[0] == res[1]


@pytest.mark.parametrize("chain_kind", ["price", "waste"])
@pytest.mark.parametrize("seed", range(3))
def test_compute_balanced_scale_up_either_form(seed, chain_kind):
    from autoscaler_amd.clustersnapshot import ClusterSnapshot
    from autoscaler_amd.estimator import ThresholdBasedEstimationLimiter
    from autoscaler_amd.nodegroupset import BalancingNodeGroupSetProcessor
    from autoscaler_amd.predicatechecker import SchedulerBasedPredicateChecker
    from autoscaler_amd.scaleup import BuildPodGroups, ComputeBalancedScaleUp
    tp, waste = _facade_inputs()
    res = []
    for form in ("host", "device"):
        nodes, pods, node_groups = tp._balanced_inputs(seed)
        snap = ClusterSnapshot(native.Mirror(0))
        pc = SchedulerBasedPredicateChecker()
        chain = tp._chain(seed) if chain_kind == "price" else waste(seed)
        best, plan, feas = ComputeBalancedScaleUp(snap, pc, BuildPodGroups(pods), node_groups,
                                                  ThresholdBasedEstimationLimiter(max_nodes=0), chain,
                                                  BalancingNodeGroupSetProcessor(), option_lists=form)
        res.append((None if best is None else (best.node_group.Id(), best.node_count, [p.name for p in best.pods]),
                    [(i.Group.Id(), i.CurrentSize, i.NewSize, i.MaxSize) for i in plan], feas.tobytes(),
                    pc.last_index, pc.evals))
        snap.backend.close()
    assert res[0] == res[1]


def test_option_lists_argument_is_checked():
    from autoscaler_amd.scaleup import _check_option_lists
    assert _check_option_lists(None) in ("device", "host")
    with pytest.raises(ValueError):
        _check_option_lists("gpu")


def test_runonce_builds_the_lists_on_the_device(oracle_lib):
    """A reduced C5 loop: step 3 goes through estimate_options on the mirror and through the
    list-building loop on the oracle; every step compares equal."""
    import pyoracle
    w = runonce.c5_runonce(n_nodes=800, n_pending=2000, n_groups=16)
    o = pyoracle.OracleState()
    W.load_filter(o, w.filt)
    ro = runonce.run(o, pyoracle.runonce_cpu_util, w)
    assert not callable(getattr(type(o), "estimate_options", None))
    res = {}
    for form in ("device", "host"):
        m = native.Mirror(0)
        W.load_filter(m, w.filt)
        util = runonce.DeviceUtil(0)
        res[form] = runonce.run(m, util, w, option_lists=form)
        util.close()
        m.close()
        eq = runonce.compare(ro, res[form])
        assert all(eq.values()), (form, eq)
        assert ro.last_index == res[form].last_index
    assert res["device"].sizes == res["host"].sizes and res["device"].sizes["estimate_items"] > 0
