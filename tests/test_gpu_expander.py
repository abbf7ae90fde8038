"""The expander on the Estimate plan's device-resident lists (csrc/expander.hip): per-option
request sums (ca_estimate_plan_option_sums), one option's list (ca_estimate_plan_fetch_group)
and the least-waste / most-pods survivors, against numpy sums of the pod table's
containers-only fields over the CPU restatement's scheduled lists, and against the host form
of the filters (autoscaler_amd/expander.py) on the same lists.

The shapes are those of test_gpu_table_chain: a few pod shapes, deep-copied.  Every case is a
handful of groups of at most a few tiles (native.OPTION_SUMS_TILE list positions per block).
"""
import copy
import random

import numpy as np
import pytest

from autoscaler_amd import abi, k8s, native
from autoscaler_amd.clustersnapshot import ClusterSnapshot, NodeInfo
from autoscaler_amd.estimator import ThresholdBasedEstimationLimiter
from autoscaler_amd.expander import ChainStrategy, DeviceOptions, LeastWaste, MostPods, resources_for_node
from autoscaler_amd.k8s import Container, OwnerReference, Quantity
from autoscaler_amd.predicatechecker import SchedulerBasedPredicateChecker
from autoscaler_amd.scaleup import (BuildPodGroups, ComputeBestExpansionOption, ComputeExpansionOptions,
                                    ExpansionOption)
from estgen import _encode_estimate, _estimate_inputs

pytestmark = pytest.mark.gpu

GI = 1 << 30
MI = 1 << 20
TILE = native.OPTION_SUMS_TILE


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


def _pod(name, cpu, mem, init_cpu=0):
    p = k8s.build_test_pod(name, cpu, mem)
    if init_cpu:
        p.init_containers.append(Container(requests={"cpu": Quantity.milli(init_cpu)}))
    return p


# (ma and mb: an init container of 1500m above their containers' 300m / 320m, so their
# requests differ from the containers-only sums the expander adds up)
SHAPES = {
    "top": _pod("top", 2000, 4 * GI),
    "s1": _pod("s1", 1000, 2 * GI),
    "s2": _pod("s2", 500, 1 * GI),
    "ma": _pod("ma", 300, 1 * GI, init_cpu=1500),
    "mb": _pod("mb", 320, 1 * GI, init_cpu=1500),
    "s3": _pod("s3", 250, 512 * MI),
    "bottom": _pod("bottom", 100, 128 * MI),
    "huge": _pod("huge", 64000, 512 * GI),           # fits no template below
}

T_MID = ("mid", 8000, 16 * GI, 110)
T_SMALL = ("small", 4000, 8 * GI, 10)
T_WIDE = ("wide", 16000, 64 * GI, 110)


def _inputs(groups, templates):
    """groups: per group a list of (shape, count), interleaved round-robin in the group's list
    (test_gpu_table_chain._inputs; an empty group is an empty list)."""
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
        for i in range(max((len(x) for x in lists), default=0)):
            out.extend(x[i] for x in lists if i < len(x))
        sel.append(out)
    return pods, [(k8s.build_test_node(*t), []) for t in templates], sel


class _First:
    def BestOption(self, options, node_infos):  # noqa: N802
        return options[0] if options else None


class Case:
    """One Estimate input on both backends: the oracle's lists and the expected sums per
    max_nodes (computed once per limit), the plan on the device."""

    def __init__(self, oracle, pods, templates, groups):
        self.pods, self.templates = pods, templates
        self.table, node_recs, self.tm, self.off, self.pod_idx = _encode_estimate([], pods, templates, groups)
        self.o, self.m = oracle.OracleState(), native.Mirror(0)
        self.G = len(groups)
        self.plan = native.EstimatePlan(self.m, self.table, self.off, self.pod_idx, self.tm)
        caps = [resources_for_node(t) for t, _ in templates]
        self.cap_cpu, self.cap_mem = [c for c, _ in caps], [m for _, m in caps]
        self._want = {}

    def close(self):
        self.plan.close()
        self.m.close()

    def want(self, max_nodes):
        """(oracle output, per-group lists, cpu sums, memory sums)."""
        if max_nodes not in self._want:
            ro = self.o.estimate(self.table, self.off, self.pod_idx, self.tm, max_nodes, 0)
            lists, cpu, mem = [], np.zeros(self.G, np.int64), np.zeros(self.G, np.int64)
            for g in range(self.G):
                ok = int(ro.results[g]["status"]) == abi.CA_OK
                a, n = int(self.off[g]), int(ro.results[g]["n_scheduled"]) if ok else 0
                ids = ro.sched_pod[a:a + n]
                lists.append(ids)
                cpu[g] = self.table.pods["score_milli_cpu"][ids].sum(dtype=np.int64)
                mem[g] = self.table.pods["score_memory"][ids].sum(dtype=np.int64)
            self._want[max_nodes] = (ro, lists, cpu, mem)
        return self._want[max_nodes]

    def host_survivors(self, max_nodes, flt):
        """The host form of a filter over every group as an option, from the oracle's lists."""
        ro, lists, _, _ = self.want(max_nodes)
        infos = {g: NodeInfo(self.templates[g][0]) for g in range(self.G)}
        options = [ExpansionOption(g, int(ro.results[g]["node_count"]), [self.pods[i] for i in lists[g]])
                   for g in range(self.G)]
        return [o.node_group for o in flt.BestOptions(options, infos)]

    def check_resident(self, max_nodes, what=""):
        """After a run that left final lists: sums, every group's list, both filters."""
        ro, lists, cpu, mem = self.want(max_nodes)
        got_cpu, got_mem = self.plan.option_sums()
        assert got_cpu.tolist() == cpu.tolist(), (what, max_nodes)
        assert got_mem.tolist() == mem.tolist(), (what, max_nodes)
        for g in range(self.G):
            assert np.array_equal(self.plan.fetch_group(g), lists[g]), (what, max_nodes, g)
        dev = DeviceOptions(self.plan, ro.results, self.cap_cpu, self.cap_mem)
        every = np.arange(self.G, dtype=np.int32)
        for flt in (LeastWaste(), MostPods()):
            assert flt.best_indices(dev, every).tolist() == self.host_survivors(max_nodes, flt), (what, type(flt))
        return got_cpu, got_mem

    def run_device(self, max_nodes, what=""):
        ro = self.want(max_nodes)[0]
        d = self.plan.run(max_nodes, 0, device_results=True)
        assert np.array_equal(ro.results, d.results) and ro.last_index == d.last_index, what
        return self.check_resident(max_nodes, what)


@pytest.fixture
def make_case(oracle):
    made = []

    def make(groups, templates):
        c = Case(oracle, *_inputs(groups, templates))
        made.append(c)
        return c
    yield make
    for c in made:
        c.close()


def _two(n):
    """n pods in two shapes (so a sum is not a multiple of one record)."""
    return [("s2", n - n // 3), ("s3", n // 3)]


def test_tile_edges(make_case):
    """Lists one below, at and one above the tile length, at aligned and unaligned offsets:
    a TILE-long list at an odd offset spills into a second tile with a masked head; a list that
    ends one position into a tile; a one-pod group behind them."""
    sizes = [5, TILE - 1, 3, TILE, TILE + 1, TILE, 1]
    c = make_case([_two(n) for n in sizes], [T_WIDE] * len(sizes))
    off = c.off.tolist()
    assert off[1] % 4 == 1 and off[3] % 4 == 3 and off[5] % 4 == 0       # odd, odd, aligned starts
    c.run_device(0)
    assert [int(n) for n in c.plan.results["n_scheduled"]] == sizes      # every list is scheduled whole


def test_empty_list_group(make_case):
    """A group without pods between two others: no tile, sums 0, an empty list."""
    c = make_case([_two(40), [], _two(9)], [T_MID, T_MID, T_SMALL])
    cpu, mem = c.run_device(0)
    assert cpu[1] == 0 and mem[1] == 0 and len(c.plan.fetch_group(1)) == 0


def test_unscheduled_group_is_the_nan_option(make_case):
    """A group whose pods fit nowhere: n_scheduled == 0 and node_count == 0, score 0 / 0.  First
    in the option order it wins least-waste; later it is skipped."""
    c = make_case([[("huge", 4)], _two(50), [("s1", 20)]], [T_MID, T_MID, T_SMALL])
    cpu, mem = c.run_device(0)
    r = c.plan.results
    assert int(r[0]["n_scheduled"]) == 0 and int(r[0]["node_count"]) == 0 and cpu[0] == 0 and mem[0] == 0
    dev = DeviceOptions(c.plan, r, c.cap_cpu, c.cap_mem)
    assert LeastWaste().best_indices(dev, [0, 1, 2]).tolist() == [0]
    later = LeastWaste().best_indices(dev, [1, 0, 2]).tolist()
    assert 0 not in later and len(later) >= 1


def test_stale_tail_after_a_limited_run(make_case):
    """An unlimited run, then max_nodes = 3 on the same plan: the slices' tails still hold the
    first run's ids; sums and fetch_group stop at the second run's n_scheduled."""
    c = make_case([_two(300), [("s1", 90), ("bottom", 200)], _two(TILE + 7)], [T_SMALL, T_MID, T_SMALL])
    full_cpu, _ = c.run_device(0)
    cpu, _ = c.run_device(3)
    assert (cpu < full_cpu).all()
    assert (c.plan.results["n_scheduled"] < np.diff(c.off)).all()


def test_class_count_paths(make_case, oracle):
    """More score classes than the LDS table holds (a gather per id) and fewer (counted in
    LDS), on lists of more than one tile."""
    n = native.OPTION_SUMS_LDS_CLASSES + 52
    for n_cls in (n, 300):
        pods = [k8s.build_test_pod(f"c{i}", 10 + i % n_cls, 64 * MI + (i % n_cls) * 4096) for i in range(n)]
        assert len({(10 + i % n_cls) for i in range(n)}) == n_cls
        groups = [pods[::2], pods[1::3], pods]
        c = Case(oracle, pods, [(k8s.build_test_node(*T_WIDE), []) for _ in groups], groups)
        try:
            c.run_device(0, n_cls)
            c.run_device(2, n_cls)
        finally:
            c.close()


def test_containers_only_field(make_case):
    """ma / mb request their init container's 1500m (req_milli_cpu) but their containers sum to
    300m / 320m: the sums follow the containers-only field."""
    c = make_case([[("ma", 40), ("mb", 30), ("s2", 20)], [("mb", 25)]], [T_MID, T_SMALL])
    cpu, _ = c.run_device(0)
    ro, lists, _, _ = c.want(0)
    req = np.array([c.table.pods["req_milli_cpu"][ids].sum() for ids in lists])
    assert (req > cpu).all()
    assert cpu[1] == 320 * int(ro.results[1]["n_scheduled"])


def test_exact_integers(oracle):
    """Three pods of 2^52 + 1 bytes: the sum 3 * 2^52 + 3 has no float64 form."""
    big = (1 << 52) + 1
    pods = [k8s.build_test_pod(f"b{i}", 100, big) for i in range(3)]
    c = Case(oracle, pods, [(k8s.build_test_node("t", 16000, 1 << 56, 110), [])], [pods])
    try:
        _, mem = c.run_device(0)
        assert int(c.plan.results[0]["n_scheduled"]) == 3
        assert int(mem[0]) == 3 * big and int(np.float64(3 * big)) != 3 * big
    finally:
        c.close()


def test_run_modes(make_case):
    """After runs that copy to the host (node ordinals wanted), publish into page-locked memory
    (32-bit and 16-bit ids) the sums are right or the call is CA_ESTATE — CA_ESTATE exactly
    when the publisher wrote the results; after a device-results run always the sums."""
    base = [("top", 7), ("s1", 40), ("s2", 33), ("ma", 21), ("mb", 19), ("s3", 90), ("bottom", 66)]
    groups = [base[i % 4:i % 4 + 3 + i % 4] for i in range(5)]
    c = make_case(groups, [(T_MID, T_SMALL, T_WIDE)[i % 3] for i in range(5)])
    for max_nodes in (0, 3):
        for mode in ("nodes", "host32", "u16", "device"):
            if mode == "nodes":
                c.plan.run(max_nodes, 0, want_nodes=True)
            elif mode == "host32":
                c.plan.run(max_nodes, 0, want_nodes=False)
            elif mode == "u16":
                c.plan.run_u16(max_nodes, 0)
            else:
                c.plan.run(max_nodes, 0, device_results=True)
            path = c.plan.stats()["results_path"]
            try:
                c.check_resident(max_nodes, mode)
            except native.CasimError as e:
                assert e.status == abi.CA_ESTATE and mode in ("host32", "u16") and path == "published", (mode, path)
                with pytest.raises(native.CasimError):
                    c.plan.fetch_group(0)
            else:
                assert path != "published", mode


def test_coupled_and_decoupled_paths(make_case, oracle):
    """A podset whose classes are uniform runs decoupled; one with two pods of equal score but
    different requests (an init container) takes the coupled path: both leave final lists."""
    c = make_case([_two(120), [("s1", 30), ("bottom", 50)]], [T_MID, T_SMALL])
    c.run_device(0)
    assert c.plan.stats()["decoupled"]
    pods, templates, groups = _inputs([_two(120), [("s1", 30), ("bottom", 50)]], [T_MID, T_SMALL])
    pods[0].init_containers.append(Container(requests={"cpu": Quantity.milli(700)}))      # same score, other request
    n = Case(oracle, pods, templates, groups)
    try:
        for max_nodes in (0, 2):
            n.run_device(max_nodes)
            assert not n.plan.stats()["decoupled"]
    finally:
        n.close()


def test_calls_before_any_run_and_bad_arguments(make_case):
    c = make_case([_two(10)], [T_MID])
    for call in (c.plan.option_sums, lambda: c.plan.fetch_group(0)):
        with pytest.raises(native.CasimError) as e:
            call()
        assert e.value.status == abi.CA_ESTATE
    c.plan.run(0, 0, device_results=True)
    with pytest.raises(native.CasimError) as e:
        c.plan.fetch_group(1)
    assert e.value.status == abi.CA_EINVAL
    import ctypes as C
    out, n = np.zeros(4, np.int32), C.c_int32(0)
    st = c.plan.lib.ca_estimate_plan_fetch_group(c.plan.h, 0, out.ctypes.data, 4, C.byref(n))
    assert st == abi.CA_ECAPACITY and n.value == 10
    assert c.plan.option_sums_ms() >= 0.0


# -- end to end ---------------------------------------------------------------------------------
def _options_inputs(seed):
    rng, nodes, pods, templates, _ = _estimate_inputs(seed, n_groups=10, n_pods=90)
    for i, p in enumerate(pods):
        if rng.random() < 0.7:
            p.owner_refs = [OwnerReference("ReplicaSet", f"rs{i % 5}", f"rs{i % 5}")]
    extra = []
    for p in pods[:30]:
        if p.owner_refs:
            q = copy.deepcopy(p)
            q.name = p.name + "-twin"
            extra.append(q)
    pods = pods + extra
    random.Random(seed).shuffle(pods)
    infos = [(f"ng{g}", NodeInfo(t, list(ds))) for g, (t, ds) in enumerate(templates)]
    return nodes, pods, infos


@pytest.mark.parametrize("seed", range(6))
def test_compute_best_expansion_option_matches_host_chain(seed):
    """ComputeBestExpansionOption (lists resident, one list fetched) against ChainStrategy's
    host form over ComputeExpansionOptions' output after the orchestrator's option filter."""
    res = []
    for device_form in (False, True):
        nodes, pods, infos = _options_inputs(seed)
        snap = ClusterSnapshot(native.Mirror(0))
        snap.AddNodes(nodes)
        pc = SchedulerBasedPredicateChecker()
        pc.last_index = seed % 3
        groups = BuildPodGroups(pods)
        lim = ThresholdBasedEstimationLimiter(max_nodes=7)
        chain = ChainStrategy([LeastWaste(), MostPods()], _First())
        if device_form:
            best, feas = ComputeBestExpansionOption(snap, pc, groups, infos, lim, chain)
        else:
            opts, feas = ComputeExpansionOptions(snap, pc, groups, infos, lim)
            valid = [o for o in opts if len(o.pods) > 0 and o.node_count > 0]
            best = chain.BestOption(valid, dict(infos)) if valid else None
        res.append((None if best is None else (best.node_group, best.node_count, [p.name for p in best.pods]),
                    feas, pc.last_index, pc.evals, [g.schedulable for g in groups]))
        snap.backend.close()
    (hb, hf, hl, he, hs), (db, df, dl, de, ds) = res
    assert hb == db
    assert np.array_equal(hf, df) and hl == dl and he == de and hs == ds


def test_compute_best_expansion_option_fetches_every_survivor():
    """Two node groups with equal templates tie on both filters: the chain falls through, the
    lists of both survivors are fetched and the caller's fallback picks (here: the first)."""
    seen = []

    class Fallback:
        def BestOption(self, options, node_infos):  # noqa: N802
            seen.append([(o.node_group, o.node_count, [p.name for p in o.pods]) for o in options])
            return options[0] if options else None

    res = []
    for device_form in (False, True):
        pods = []
        for i in range(24):
            p = k8s.build_test_pod(f"p{i}", 500, GI)
            p.owner_refs = [OwnerReference("ReplicaSet", "rs", "rs")]
            pods.append(p)
        infos = [("worse", NodeInfo(k8s.build_test_node("tw", 16000, 64 * GI, 110), [])),
                 ("a", NodeInfo(k8s.build_test_node("ta", 4000, 8 * GI, 110), [])),
                 ("b", NodeInfo(k8s.build_test_node("tb", 4000, 8 * GI, 110), []))]
        snap = ClusterSnapshot(native.Mirror(0))
        pc = SchedulerBasedPredicateChecker()
        groups = BuildPodGroups(pods)
        lim = ThresholdBasedEstimationLimiter(max_nodes=0)
        chain = ChainStrategy([LeastWaste(), MostPods()], Fallback())
        if device_form:
            best, _ = ComputeBestExpansionOption(snap, pc, groups, infos, lim, chain)
        else:
            opts, _ = ComputeExpansionOptions(snap, pc, groups, infos, lim)
            best = chain.BestOption([o for o in opts if len(o.pods) > 0 and o.node_count > 0], dict(infos))
        res.append((best.node_group, best.node_count, [p.name for p in best.pods], pc.last_index, pc.evals))
        snap.backend.close()
    assert res[0] == res[1] and res[0][0] == "a" and res[0][1] == 3 and len(res[0][2]) == 24
    assert len(seen) == 2 and seen[0] == seen[1] and [o[0] for o in seen[0]] == ["a", "b"]


def test_more_groups_than_a_block_has_lanes(make_case):
    """600 small groups and a two-tile one at the end: a tile's group is found by binary steps
    down to one candidate per lane, then by the lanes."""
    groups = [[("s2", 1 + g % 3)] if g % 7 else [("s3", 2), ("s2", 1)] for g in range(600)] + [_two(TILE + 5)]
    c = make_case(groups, [(T_MID, T_SMALL)[g % 2] for g in range(601)])
    c.run_device(0)
    c.run_device(1)
