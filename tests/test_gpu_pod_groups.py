"""BuildPodGroups on the device (ca_pod_groups_create) against the reference loop stated on the
records (groupgen.groups_of), byte for byte on every case; the two calls that read the handle
(ca_expansion_plan_run_groups, ca_estimate_plan_create_groups) against their host-array forms
on the fetched groups; and the callers (runonce.run, the Compute* facades)."""
import ctypes as C

import numpy as np
import pytest

import groupgen
import optgen
from groupgen import T, CHUNK
from autoscaler_amd import abi, native, runonce, workloads as W
from autoscaler_amd.abi import ptr

pytestmark = pytest.mark.gpu

LIMITS = [0, 3]


@pytest.fixture(scope="module")
def mirror():
    m = native.Mirror(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def podsets(mirror):
    """One resident podset per distinct pod table of the cases."""
    made = {}

    def get(pods):
        key = pods.tobytes()
        if key not in made:
            made[key] = mirror.podset(abi.PodTable(pods))
        return made[key]
    yield get
    for ps in made.values():
        ps.close()


def _build(mirror, podsets, name):
    _, pods, order, node, owner, _ = groupgen.case(name)
    return mirror.build_pod_groups(podsets(pods), order=order, node=node, class_owner=owner)


@pytest.mark.parametrize("name", groupgen.CASE_NAMES)
def test_fetch_is_groups_of(name, mirror, podsets):
    want_off, want_pod = groupgen.expected(name)
    with _build(mirror, podsets, name) as g:
        assert (g.n_groups, g.n_pods) == (len(want_off) - 1, len(want_pod))
        eg_off, eg_pod = g.fetch()
        assert eg_off.dtype == np.int32 and eg_pod.dtype == np.int32
        assert eg_off.tobytes() == want_off.tobytes()
        assert eg_pod.tobytes() == want_pod.tobytes()
        assert g.samples().tobytes() == want_pod[want_off[:-1]].tobytes()
        t = g.timings()
        assert t["build_ms"] >= 0 and (t["launches"] > 0) == (name != "n_0")      # (n == 0: nothing is launched)
        # a second build gives the same bytes
        with _build(mirror, podsets, name) as h:
            off2, pod2 = h.fetch()
            assert off2.tobytes() == eg_off.tobytes() and pod2.tobytes() == eg_pod.tobytes()
            assert h.timings()["launches"] == t["launches"]


def test_launch_count_does_not_depend_on_the_data(mirror, podsets):
    """Two cases of one size and one form of arguments: the same number of kernels."""
    n = {}
    for name in (f"unsched_{T - 1}", f"unsched_{2 * T + 1}", "unsched_1"):
        with _build(mirror, podsets, name) as g:
            n[name] = g.timings()["launches"]
    assert len(set(n.values())) == 1, n


def test_einval_leaves_no_handle(mirror, podsets):
    _, pods, _, _, _, _ = groupgen.case("owner_25")
    ps = podsets(pods)
    P = len(pods)
    lib = mirror.lib
    n_cls = int(pods["similar_class"].max()) + 1
    owner = np.zeros(n_cls, np.int32)

    def status(order, n, node, class_owner, n_classes):
        h = C.c_void_p(0xDEAD)
        od = None if order is None else np.ascontiguousarray(order, np.int32)
        nd = None if node is None else np.ascontiguousarray(node, np.int32)
        co = None if class_owner is None else np.ascontiguousarray(class_owner, np.int32)
        st = lib.ca_pod_groups_create(mirror.h, ps.h, ptr(od), n, ptr(nd), ptr(co), n_classes, C.byref(h))
        if st == abi.CA_OK:
            assert h.value not in (None, 0xDEAD)
            lib.ca_pod_groups_destroy(h)
        else:
            assert h.value is None, "no handle after an error"
        return st

    assert status(None, P, None, owner, n_cls) == abi.CA_OK
    assert status(None, -1, None, owner, n_cls) == abi.CA_EINVAL                       # n < 0
    assert status(None, P + 1, None, None, 0) == abi.CA_EINVAL                         # table order past the set
    for bad in (-1, P, 2**31 - 1):
        order = np.arange(P, dtype=np.int32)
        order[P // 2] = bad
        assert status(order, P, None, owner, n_cls) == abi.CA_EINVAL                   # outside the pod set
        assert status(order, P, None, None, 0) == abi.CA_EINVAL
    assert status(None, P, None, owner[:-1], n_cls - 1) == abi.CA_EINVAL               # similar_class >= n_classes
    bad_owner = owner.copy()
    bad_owner[3] = -1
    assert status(None, P, None, bad_owner, n_cls) == abi.CA_EINVAL                    # a class_owner entry below 0
    # the class past n_classes belongs to a placed pod only: the list does not hold it
    last = np.nonzero(pods["similar_class"] == n_cls - 1)[0]
    node = np.full(P, -1, np.int32)
    node[last] = 0
    assert status(None, P, node, owner[:-1], n_cls - 1) == abi.CA_OK
    # ... or to a DaemonSet pod, which never shares a group
    _, ds, _, _, _, _ = groupgen.case("daemonset")
    h = C.c_void_p()
    st = lib.ca_pod_groups_create(mirror.h, podsets(ds).h, None, len(ds), None, ptr(np.zeros(1, np.int32)), 1, C.byref(h))
    assert st == abi.CA_OK
    lib.ca_pod_groups_destroy(h)
    # a podset of another mirror
    other = native.Mirror(0)
    h = C.c_void_p(0xDEAD)
    assert lib.ca_pod_groups_create(other.h, ps.h, None, P, None, None, 0, C.byref(h)) == abi.CA_EINVAL
    other.close()


PLAN_CASES = ["n_0", f"unsched_{T + 1}", "interleaved_64", "owner_25", "owners_3000", "shuffled_order",
              f"n_eg_{CHUNK - 1}", f"n_eg_{CHUNK}", f"n_eg_{CHUNK + 1}"]


@pytest.mark.parametrize("name", PLAN_CASES)
def test_expansion_run_reads_the_samples_from_the_handle(name, mirror, podsets):
    _, pods, _, _, _, _ = groupgen.case(name)
    ps = podsets(pods)
    tm = optgen._templates(5)
    tm[1]["node"]["alloc_milli_cpu"] = 600                    # some samples fail on it
    tm[3]["node"]["alloc_memory"] = 2000 * W.MI
    with _build(mirror, podsets, name) as g, native.ExpansionPlan(mirror, tm) as ep:
        samples = g.samples()
        for verdict_only in (False, True):
            want = ep.run(ps, samples, verdict_only=verdict_only)
            got = ep.run(ps, verdict_only=verdict_only, groups=g)
            assert got.shape == want.shape == (5, g.n_groups)
            assert got.tobytes() == want.tobytes()
        if g.n_groups:
            ok = ep.run(ps, verdict_only=True, groups=g)
            assert 0 < int(ok.sum()) < ok.size                 # both verdicts occur


@pytest.mark.parametrize("name", PLAN_CASES)
def test_plans_from_the_handle_equal_plans_from_the_fetched_csr(name, mirror, podsets):
    from test_gpu_option_lists import _modes
    _, pods, _, _, _, _ = groupgen.case(name)
    ps = podsets(pods)
    with _build(mirror, podsets, name) as g:
        eg_off, eg_pod = g.fetch()
        E = g.n_groups
        rng = np.random.default_rng(E)
        ok = optgen._rows(E, rng) if E else np.zeros((6, 0), np.uint8)
        tm = optgen._templates(len(ok))
        with native.EstimatePlan.from_options(mirror, ps, eg_off, eg_pod, ok, tm) as a, \
                native.EstimatePlan.from_groups(mirror, ps, g, ok, tm) as b:
            want_off, want_idx = optgen.lists_of(eg_off, eg_pod, ok)
            assert a.group_off.tobytes() == b.group_off.tobytes() == want_off.tobytes()
            assert (a.total, a.G) == (b.total, b.G)
            a_idx, a_cls = a.fetch_lists()
            b_idx, b_cls = b.fetch_lists()
            assert b_idx.tobytes() == a_idx.tobytes() == want_idx.tobytes()
            assert (a_cls is None) == (b_cls is None) and (a_cls is None or a_cls.tobytes() == b_cls.tobytes())
            for max_nodes in LIMITS:
                ra, sa, _ = _modes(a, max_nodes)
                rb, sb, _ = _modes(b, max_nodes)
                for mode in ra:
                    assert ra[mode] == rb[mode], (name, max_nodes, mode)
                assert sa == sb
            assert E == 0 or b.stats()["option_lists_ms"] > 0


def test_from_groups_wants_the_groups_own_podset(mirror, podsets):
    _, pods, _, _, _, _ = groupgen.case("first_placed")
    other = mirror.podset(abi.PodTable(pods.copy()))
    with _build(mirror, podsets, "first_placed") as g:
        with pytest.raises(ValueError):
            native.EstimatePlan.from_groups(mirror, other, g, np.ones((1, g.n_groups), np.uint8), optgen._templates(1))
        st = mirror.lib.ca_estimate_plan_create_groups(mirror.h, other.h, g.h, None, None, 0,
                                                       ptr(np.zeros(1, np.int32)), C.byref(C.c_void_p()))
        assert st == abi.CA_EINVAL
    other.close()


def test_runonce_with_device_pod_groups():
    """A reduced C5 loop with the grouping on the device against the Python loop: every compared
    output and the sizes are equal (no unschedulable pod of this workload is a DaemonSet pod,
    which runonce._equivalence_groups does not tell apart)."""
    w = runonce.c5_runonce(n_nodes=800, n_pending=2000, n_groups=16)
    res = {}
    for form in ("host", "device"):
        for expand in (False, True):
            m = native.Mirror(0)
            W.load_filter(m, w.filt)
            util = runonce.DeviceUtil(0)
            ex = runonce.DeviceExpansion() if expand else None
            r = res[form, expand] = runonce.run(m, util, w, expand_fn=ex, pod_groups=form)
            r.util = np.copy(r.util)                # (DeviceUtil's rows are views into its page-locked buffers)
            r.options = np.copy(r.options)          # (DeviceExpansion's likewise)
            if ex is not None:
                ex.close()
            util.close()
            m.close()
    base = res["host", False]
    assert base.sizes["equivalence_groups"] > 1 and base.sizes["estimate_items"] > 0
    for key, r in res.items():
        eq = runonce.compare(base, r)
        assert all(eq.values()), (key, eq)
        assert r.sizes == base.sizes and r.last_index == base.last_index, key
    with pytest.raises(ValueError):
        runonce.run(None, None, w, pod_groups="gpu")


# -- facades ------------------------------------------------------------------------------

def _trip_the_cap(pods):
    """The first 45 pods become one controller's pods in 15 label variants (5 past the cap)."""
    from autoscaler_amd.k8s import OwnerReference
    for i, p in enumerate(pods[:45]):
        p.owner_refs = [OwnerReference("ReplicaSet", "big", "big")]
        p.labels = dict(p.labels, variant=str(i % 15))
    return pods


def _names(groups):
    return [[p.name for p in g.pods] for g in groups]


@pytest.mark.parametrize("seed", range(3))
def test_compute_best_expansion_option_on_device_groups(seed):
    import test_gpu_price as tp
    from autoscaler_amd.clustersnapshot import ClusterSnapshot
    from autoscaler_amd.estimator import ThresholdBasedEstimationLimiter
    from autoscaler_amd.predicatechecker import SchedulerBasedPredicateChecker
    from autoscaler_amd.scaleup import BuildPodGroups, BuildPodGroupsOnDevice, ComputeBestExpansionOption
    res = []
    for form in ("host", "device"):
        nodes, pods, infos = tp._options_inputs(seed)
        pods = _trip_the_cap(pods)
        snap = ClusterSnapshot(native.Mirror(0))
        snap.AddNodes(nodes)
        pc = SchedulerBasedPredicateChecker()
        pc.last_index = seed % 3
        snap.ensure(pods=pods)        # both forms intern the pods in input order: feas carries interned ids
        want = BuildPodGroups(pods)
        assert sum(len(g.pods) == 1 for g in want) >= 15 and len(want) < len(pods)
        groups = want if form == "host" else BuildPodGroupsOnDevice(snap, pods)
        assert _names(groups) == _names(want)
        best, feas = ComputeBestExpansionOption(snap, pc, groups, infos, ThresholdBasedEstimationLimiter(max_nodes=7),
                                                tp._chain(seed), option_lists="device")
        if form == "device":
            assert groups.handle is not None and groups.handle.n_groups == len(want)
            groups.close()
        res.append((None if best is None else (best.node_group, best.node_count, [p.name for p in best.pods]),
                    feas.tobytes(), [g.schedulable for g in groups]))
        snap.backend.close()
    assert res[0] == res[1]
    assert seed % 3 == 2 or res[0][0] is not None          # (seed 2: some pods have no price, tp._chain)


@pytest.mark.parametrize("seed", range(3))
def test_compute_balanced_scale_up_on_device_groups(seed):
    import test_gpu_price as tp
    from autoscaler_amd.clustersnapshot import ClusterSnapshot
    from autoscaler_amd.estimator import ThresholdBasedEstimationLimiter
    from autoscaler_amd.nodegroupset import BalancingNodeGroupSetProcessor
    from autoscaler_amd.predicatechecker import SchedulerBasedPredicateChecker
    from autoscaler_amd.scaleup import BuildPodGroups, BuildPodGroupsOnDevice, ComputeBalancedScaleUp
    res = []
    for form in ("host", "device"):
        nodes, pods, node_groups = tp._balanced_inputs(seed)
        pods = _trip_the_cap(pods)
        snap = ClusterSnapshot(native.Mirror(0))
        pc = SchedulerBasedPredicateChecker()
        snap.ensure(pods=pods)        # (as above)
        want = BuildPodGroups(pods)
        assert sum(len(g.pods) == 1 for g in want) >= 5 and len(want) >= 15          # 5 variants past the cap
        groups = want if form == "host" else BuildPodGroupsOnDevice(snap, pods)
        assert _names(groups) == _names(want)
        best, plan, feas = ComputeBalancedScaleUp(snap, pc, groups, node_groups,
                                                  ThresholdBasedEstimationLimiter(max_nodes=0), tp._chain(seed),
                                                  BalancingNodeGroupSetProcessor(), option_lists="device")
        if form == "device":
            groups.close()
        res.append((None if best is None else (best.node_group.Id(), best.node_count, [p.name for p in best.pods]),
                    [(i.Group.Id(), i.CurrentSize, i.NewSize, i.MaxSize) for i in plan], feas.tobytes()))
        snap.backend.close()
    assert res[0] == res[1]
    assert seed % 3 == 2 or res[0][0] is not None
