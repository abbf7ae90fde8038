"""filterNodeGroupsByPods on the Estimate plan's device-resident lists
(csrc/nodegroupset.hip: ca_estimate_plan_groups_missing_pods) against set membership in Python
over the CPU restatement's lists, on the cases of tests/similargen.py (which
tests/test_similar_cases.py checks on the CPU), and ComputeBalancedScaleUp against the same flow
built from host lists.  Every case is a handful of groups of at most three tiles."""
import numpy as np
import pytest

import similargen as S
from autoscaler_amd import abi, k8s, native
from autoscaler_amd.clustersnapshot import ClusterSnapshot, NodeInfo
from autoscaler_amd.estimator import ThresholdBasedEstimationLimiter
from autoscaler_amd.expander import ChainStrategy, LeastWaste, MostPods
from autoscaler_amd.k8s import OwnerReference, Taint, Toleration
from autoscaler_amd.nodegroupset import (BalancingNodeGroupSetProcessor, NodeGroup, filter_node_groups_by_pods,
                                         filter_plan_groups_by_pods)
from autoscaler_amd.predicatechecker import SchedulerBasedPredicateChecker
from autoscaler_amd.scaleup import BuildPodGroups, ComputeBalancedScaleUp, ComputeExpansionOptions

pytestmark = pytest.mark.gpu

KNOB = "CASIM_MISSING_SCRATCH"


@pytest.fixture(scope="module")
def oracle_state(oracle_lib):
    st = oracle_lib.OracleState()
    yield st
    st.close()


class Dev:
    """One case on the device (its plan) with the expected values per max_nodes, computed once
    from the CPU restatement's lists."""

    def __init__(self, case, oracle_state):
        self.c = case
        self.enc = case.encode()
        self.o = oracle_state
        self.m = native.Mirror(0)
        table, tm, off, idx = self.enc
        self.plan = native.EstimatePlan(self.m, table, off, idx, tm)
        self._lists = {}

    def close(self):
        self.plan.close()
        self.m.close()

    def lists(self, max_nodes):
        if max_nodes not in self._lists:
            self._lists[max_nodes] = S.oracle_lists(self.o, self.enc, max_nodes)
        return self._lists[max_nodes]

    def run(self, max_nodes):
        ro, _ = self.lists(max_nodes)
        d = self.plan.run(max_nodes, 0, device_results=True)
        assert np.array_equal(ro.results, d.results)
        return d

    def check(self, max_nodes, required=None, candidates=None):
        """The call on the resident lists against Python set membership."""
        _, lists = self.lists(max_nodes)
        req = self.c.g(required or self.c.required)
        cands = [self.c.g(k) for k in (candidates if candidates is not None else self.c.candidates)]
        want_n, want_first = S.expected(lists, req, cands)
        got_n, got_first = self.plan.groups_missing_pods(req, cands)
        assert got_n.tolist() == want_n.tolist(), (self.c.name, required)
        assert got_first.tolist() == want_first.tolist(), (self.c.name, required)
        kept = filter_plan_groups_by_pods(self.plan, req, cands)
        assert kept == [g for g, n in zip(cands, want_n) if n == 0]
        return got_n, got_first


@pytest.fixture
def dev(oracle_state):
    made = []

    def make(case):
        d = Dev(case, oracle_state)
        made.append(d)
        return d
    yield make
    for d in made:
        d.close()


@pytest.mark.parametrize("n,res", S.TILE_CASES)
def test_tile_edges(n, res, dev):
    """Required lists one below, at, one above a tile and two tiles + 3, required and candidate
    groups at offsets 1, 2, 3 mod 4, the missing pod at position 0, on both sides of a tile
    boundary and at the very end; two missing pods: first_missing is the smaller position."""
    assert S.TILE == native.MISSING_PODS_TILE
    d = dev(S.tile_case(n, res))
    d.run(0)
    got_n, got_first = d.check(0)
    by = dict(zip(d.c.candidates, zip(got_n.tolist(), got_first.tolist())))
    assert by["two"] == (2, 3) and by["full"] == (0, -1) and by["none"] == (n, 0)
    assert by[f"drop{n - 1}"] == (1, n - 1) and by["drop0"] == (1, 0)
    # any group as the required one: every other list against this one
    d.check(0, required="two", candidates=["req", "full", "none", "two"])
    assert d.plan.groups_missing_pods_ms() > 0.0


@pytest.mark.parametrize("n_pods", S.WORD_SIZES)
def test_word_edges(n_pods, dev):
    """Pod sets of 32 k, 32 k + 1 and 32 k + 31 pods; the missing pod (and a present one) has id
    0, 31, 32 and n_pods - 1."""
    d = dev(S.word_case(n_pods))
    d.run(0)
    got_n, _ = d.check(0)
    assert got_n.tolist()[:4] == [1, 1, 1, 1]
    d.check(0, required="full")


def test_stale_tail(dev):
    """An unlimited run, then max_nodes = 2 on the same plan: the candidate's slice still holds
    the first run's ids behind its n_scheduled, among them the very pods it now lacks."""
    d = dev(S.stale_case())
    d.run(0)
    d.check(0)
    d.run(S.STALE_LIMIT)
    got_n, got_first = d.check(S.STALE_LIMIT)
    by = dict(zip(d.c.candidates, zip(got_n.tolist(), got_first.tolist())))
    assert by["ten"] == (200, 20) and by["same"] == (0, -1) and by["minus0"] == (1, 0)
    # the same after a run whose lists did not stay final, followed by an eligible one
    d.plan.run(0, 0, want_nodes=False)
    if d.plan.stats()["results_path"] == "published":
        with pytest.raises(native.CasimError) as e:
            d.plan.groups_missing_pods(d.c.g("req"), [d.c.g("ten")])
        assert e.value.status == abi.CA_ESTATE
    d.run(S.STALE_LIMIT)
    d.check(S.STALE_LIMIT)


def test_slots(dev):
    """The required group among the candidates, a group listed twice, candidates without a list,
    an empty required list, no candidates."""
    d = dev(S.slots_case())
    d.run(0)
    got_n, got_first = d.check(0)
    names = d.c.candidates
    assert [got_n[i] for i, k in enumerate(names) if k == "req"] == [0, 0]
    assert [(got_n[i], got_first[i]) for i, k in enumerate(names) if k == "sub"] == [(1, 7)] * 3
    assert (got_n[names.index("empty")], got_first[names.index("empty")]) == (40, 0)
    assert (got_n[names.index("huge")], got_first[names.index("huge")]) == (40, 0)
    for required in ("empty", "huge"):                      # an empty required list: everything fits
        n, f = d.check(0, required=required)
        assert not n.any() and (f == -1).all()
        assert d.plan.groups_missing_pods_ms() == 0.0       # ... without a launch
    n, f = d.plan.groups_missing_pods(d.c.g("req"), [])
    assert len(n) == 0 and len(f) == 0
    d.check(0, candidates=["empty", "req"])                 # only slots the host answers
    assert d.plan.groups_missing_pods_ms() == 0.0
    import ctypes as C
    one = np.array([d.c.g("sub")], np.int32)
    out = np.zeros(1, np.int32)
    st = d.plan.lib.ca_estimate_plan_groups_missing_pods(d.plan.h, d.c.g("req"), one.ctypes.data, 1, out.ctypes.data, None)
    assert st == abi.CA_OK and out[0] == 1                  # first_missing may be NULL
    st = d.plan.lib.ca_estimate_plan_groups_missing_pods(d.plan.h, d.c.g("req"), one.ctypes.data, 1, None, None)
    assert st == abi.CA_EINVAL
    ms = C.c_float(-1)
    assert d.plan.lib.ca_estimate_plan_groups_missing_pods_ms(d.plan.h, C.byref(ms)) == abi.CA_OK and ms.value >= 0


def test_groups_cut_by_the_prefix_protocol(dev):
    """A group with an out-of-scope pod (CA_EUNSUPPORTED) and the group after it (CA_ENOTRUN)
    have n_scheduled 0: as candidates they miss everything, as the required group everything fits."""
    d = dev(S.prefix_case())
    out = d.run(0)
    st = out.results["status"].tolist()
    assert st[d.c.g("cut")] == abi.CA_EUNSUPPORTED and st[d.c.g("after")] == abi.CA_ENOTRUN
    got_n, got_first = d.check(0)
    by = dict(zip(d.c.candidates, zip(got_n.tolist(), got_first.tolist())))
    assert by["cut"] == (10, 0) and by["after"] == (10, 0) and by["one"] == (1, 0)
    for required in ("cut", "after"):
        n, f = d.check(0, required=required, candidates=["req", "full", "none", "cut", "after"])
        assert not n.any() and (f == -1).all()


def test_more_candidates_than_a_block_has_lanes(dev):
    d = dev(S.many_case())
    d.run(0)
    got_n, _ = d.check(0)
    assert len(got_n) == 300 and len(set(got_n.tolist())) == 5           # 0 .. 4 missing all occur


def test_batches(dev, monkeypatch):
    """The bitmap rows bounded to one row and to two rows a batch: identical results; below one
    row CA_ECAPACITY."""
    d = dev(S.word_case(95))
    d.run(0)
    base = d.check(0)
    row_bytes = 4 * ((95 + 31) // 32)
    for rows in (1, 2):
        monkeypatch.setenv(KNOB, str(rows * row_bytes))
        got = d.check(0)
        assert got[0].tolist() == base[0].tolist() and got[1].tolist() == base[1].tolist()
    monkeypatch.setenv(KNOB, str(row_bytes - 1))
    with pytest.raises(native.CasimError) as e:
        d.plan.groups_missing_pods(d.c.g("req"), [d.c.g("full")])
    assert e.value.status == abi.CA_ECAPACITY
    monkeypatch.delenv(KNOB)
    d.check(0)
    # the many-rows case in batches of seven rows
    m = dev(S.many_case())
    m.run(0)
    monkeypatch.setenv(KNOB, str(7 * 4))
    m.check(0)


def test_codes(dev):
    d = dev(S.word_case(64))
    req, full = d.c.g("req"), d.c.g("full")
    with pytest.raises(native.CasimError) as e:              # before any run
        d.plan.groups_missing_pods(req, [full])
    assert e.value.status == abi.CA_ESTATE
    # a run that published into page-locked memory leaves no final lists
    saw_published = False
    for mode in ("host32", "u16"):
        d.plan.run(0, 0, want_nodes=False) if mode == "host32" else d.plan.run_u16(0, 0)
        if d.plan.stats()["results_path"] == "published":
            saw_published = True
            with pytest.raises(native.CasimError) as e:
                d.plan.groups_missing_pods(req, [full])
            assert e.value.status == abi.CA_ESTATE
        else:
            d.check(0)
    assert saw_published
    d.run(0)
    G = d.plan.G
    for bad_req, bad_groups in ((-1, [full]), (G, [full]), (req, [full, -1]), (req, [G])):
        with pytest.raises(native.CasimError) as e:
            d.plan.groups_missing_pods(bad_req, bad_groups)
        assert e.value.status == abi.CA_EINVAL
    d.check(0)


def test_both_id_paths(dev, monkeypatch):
    """Lists left by the decoupled run-table path and by the coupled path (CASIM_GO_DECOUPLE=0)."""
    d = dev(S.shapes_case())
    for limit in (0, 3):
        d.run(limit)
        assert d.plan.stats()["decoupled"]
        d.check(limit)
    monkeypatch.setenv("CASIM_GO_DECOUPLE", "0")
    for limit in (0, 3):
        d.run(limit)
        assert not d.plan.stats()["decoupled"]
        d.check(limit)


# -- end to end ---------------------------------------------------------------------------------
class _First:
    def BestOption(self, options, node_infos):  # noqa: N802
        return options[0] if options else None


class _Recording(BalancingNodeGroupSetProcessor):
    """Records the groups the scale-up is balanced between ([best] + kept)."""

    def BalanceScaleUpBetweenGroups(self, groups, new_nodes):  # noqa: N802
        self.balanced = ([g.Id() for g in groups], new_nodes)
        return super().BalanceScaleUpBetweenGroups(groups, new_nodes)


def _host_flow(snap, pc, pod_groups, node_groups, lim, chain, proc):
    """ScaleUp's path from the options to the plan on host lists (orchestrator.go:139-313)."""
    infos = {ng.Id(): info for ng, info in node_groups}
    opts, feas = ComputeExpansionOptions(snap, pc, pod_groups, node_groups, lim)
    options = {o.node_group.Id(): o for o in opts if len(o.pods) > 0 and o.node_count > 0}
    if not options:
        return None, [], feas
    best = chain.BestOption(list(options.values()), infos)
    similar = proc.FindSimilarNodeGroups([ng for ng, _ in node_groups], best.node_group, infos)
    kept = filter_node_groups_by_pods(similar, best.pods, options)
    return best, proc.BalanceScaleUpBetweenGroups([best.node_group] + kept, best.node_count), feas


def _both_flows(make_inputs):
    res = []
    for device_form in (False, True):
        nodes, pods, node_groups = make_inputs()
        snap = ClusterSnapshot(native.Mirror(0))
        for node, scheduled in nodes:
            snap.AddNodeWithPods(node, scheduled)
        pc = SchedulerBasedPredicateChecker()
        lim = ThresholdBasedEstimationLimiter(max_nodes=0)
        chain = ChainStrategy([LeastWaste(), MostPods()], _First())
        proc = _Recording()
        flow = ComputeBalancedScaleUp if device_form else _host_flow
        best, plan, feas = flow(snap, pc, BuildPodGroups(pods), node_groups, lim, chain, proc)
        res.append(((best.node_group.Id(), best.node_count, [p.name for p in best.pods]), proc.balanced,
                    [(i.Group.Id(), i.CurrentSize, i.NewSize, i.MaxSize) for i in plan], feas.tobytes(),
                    pc.last_index, pc.evals))
        snap.backend.close()
    assert res[0] == res[1]
    return res[1]


def test_balanced_scale_up_drops_the_zone_a_pod_group_does_not_fit():
    """Three similar zones; zone c's template has a taint the `web` pods do not tolerate, so c's
    option lacks pods of the winner's and c is dropped; the other shape is not similar."""
    def make():
        pods = []
        for i in range(12):
            p = k8s.build_test_pod(f"job{i}", 500, S.GI)
            p.owner_refs = [OwnerReference("ReplicaSet", "job", "job")]
            p.tolerations.append(Toleration(key="dedicated", operator="Exists"))
            pods.append(p)
        for i in range(8):
            p = k8s.build_test_pod(f"web{i}", 300, S.GI)
            p.owner_refs = [OwnerReference("ReplicaSet", "web", "web")]
            pods.append(p)
        groups = []
        for zone, size in (("a", 1), ("b", 3), ("c", 0)):
            n = k8s.build_test_node(f"t-{zone}", 4000, 8 * S.GI, 110)
            n.labels.update({"topology.kubernetes.io/zone": zone, "pool": "std"})
            if zone == "c":
                n.taints.append(Taint("dedicated", "x", "NoSchedule"))
            groups.append((NodeGroup(f"ng-{zone}", size, 10), NodeInfo(n, [])))
        big = k8s.build_test_node("t-big", 32000, 128 * S.GI, 110)
        big.labels.update({"topology.kubernetes.io/zone": "a", "pool": "std"})
        groups.append((NodeGroup("ng-big", 1, 10), NodeInfo(big, [])))
        return [], pods, groups
    best, balanced, plan, *_ = _both_flows(make)
    assert best[0] == "ng-a" and len(best[2]) == 20
    assert balanced[0] == ["ng-a", "ng-b"] and balanced[1] == best[1]
    assert sum(n - c for _, c, n, _ in plan) == best[1] and {g for g, *_ in plan} <= {"ng-a", "ng-b"}


def test_balanced_scale_up_balance_groups_known_answer():
    """TestScaleUpBalanceGroups (orchestrator_test.go:763-837): ng1 is maxed and skipped by the
    caller; the two 80m pods need two 100m nodes, split between ng2 and ng3."""
    cfg = {"ng1": (1, 1, 1), "ng2": (1, 2, 1), "ng3": (1, 5, 1), "ng4": (1, 5, 3)}

    def make():
        nodes, groups = [], []
        for gid, (mn, mx, size) in cfg.items():
            for i in range(size):
                nodes.append((k8s.build_test_node(f"{gid}-node-{i}", 100, 1000),
                              [k8s.build_scheduled_test_pod(f"{gid}-pod-{i}", 80, 0, f"{gid}-node-{i}")]))
            if size < mx:                                   # (ScaleUp skips a group at its maximum)
                groups.append((NodeGroup(gid, size, mx, mn), NodeInfo(k8s.build_test_node(f"{gid}-template", 100, 1000), [])))
        pods = [k8s.build_test_pod(f"test-pod-{i}", 80, 0) for i in range(2)]
        return nodes, pods, groups
    best, balanced, plan, *_ = _both_flows(make)
    assert best[1] == 2 and sorted(balanced[0]) == ["ng2", "ng3", "ng4"]
    assert {g: n for g, _, n, _ in plan} == {"ng2": 2, "ng3": 2}
