"""The price expander's totalPodPrice on the Estimate plan's device-resident lists
(csrc/expander.hip: ca_estimate_plan_option_price_sums) against the in-order Python float sum
over the CPU restatement's lists, byte for byte, on the cases of tests/pricegen.py (which
tests/test_price_cases.py checks on the CPU); and ComputeBestExpansionOption /
ComputeBalancedScaleUp with the price filter in the chain against the host chain on host lists.
Every case is one small plan; the longest list is 4097 pods."""
import copy
import ctypes as C
import math
import random
import zlib

import numpy as np
import pytest

import pricegen as P
from autoscaler_amd import abi, k8s, native
from autoscaler_amd.clustersnapshot import ClusterSnapshot, NodeInfo
from autoscaler_amd.estimator import ThresholdBasedEstimationLimiter
from autoscaler_amd.expander import (ChainStrategy, PriceBased, PricingError, SimpleNodeUnfitness,
                                     SimplePreferredNodeProvider)
from autoscaler_amd.k8s import OwnerReference, Quantity
from autoscaler_amd.nodegroupset import BalancingNodeGroupSetProcessor, NodeGroup, filter_node_groups_by_pods
from autoscaler_amd.predicatechecker import SchedulerBasedPredicateChecker
from autoscaler_amd.scaleup import (BuildPodGroups, ComputeBalancedScaleUp, ComputeBestExpansionOption,
                                    ComputeExpansionOptions)
from estgen import _estimate_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle_state(oracle_lib):
    st = oracle_lib.OracleState()
    yield st
    st.close()


def assert_same_bits(got, want, what=""):
    """Raw bytes; where the reference is NaN only isnan is compared."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, np.flatnonzero(np.isnan(got) != nan)[:8])
    g, w = got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]
    bad = np.flatnonzero(g != w)
    assert len(bad) == 0, (what, len(bad), np.flatnonzero(~nan)[bad][:8], got[~nan][bad][:4], want[~nan][bad][:4])


class Dev:
    """One case on the device (its plan) with the oracle's lists per max_nodes, computed once."""

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
            self._lists[max_nodes] = P.oracle_lists(self.o, self.enc, max_nodes)
        return self._lists[max_nodes]

    def run(self, max_nodes):
        ro, _ = self.lists(max_nodes)
        d = self.plan.run(max_nodes, 0, device_results=True)
        assert np.array_equal(ro.results, d.results)
        return d

    def check(self, max_nodes, price=None):
        price = self.c.price if price is None else price
        _, lists = self.lists(max_nodes)
        got = self.plan.option_price_sums(price)
        assert_same_bits(got, P.expected(price, lists), (self.c.name, max_nodes))
        return got


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


def test_chunk_edges(dev):
    """Lists of 0..130 pods and around every power of two up to 4096, at offsets of every
    residue mod 4 and mod 64, in one run and one call; a second price table on the same run
    reuses the scratch."""
    assert P.CHUNK == native.PRICE_SUMS_CHUNK and P.CHUNK <= 2048
    d = dev(P.edges_case())
    d.run(0)
    got = d.check(0)
    assert len(got) == len(P.EDGE_LENGTHS)
    zero = got[d.c.index["len0"]]
    assert zero == 0.0 and not np.signbit(zero)
    assert d.plan.option_price_sums_ms() > 0.0
    other = P.random_prices(random.Random(7), len(d.c.price))
    assert d.check(0, other).tobytes() != got.tobytes()
    d.check(0)                                                           # and the first table again
    d.check(0, np.zeros(len(d.c.price)))                                 # +0.0 everywhere
    d.check(0, -other)                                                   # negative prices


def test_stale_tail(dev):
    """An unlimited run, then max_nodes = 1 on the same plan: behind n_scheduled the slices keep
    the first run's ids; the sums follow the short lists."""
    d = dev(P.stale_case())
    d.run(0)
    full = d.check(0)
    d.run(P.STALE_LIMIT)
    short = d.check(P.STALE_LIMIT)
    g = d.c.index
    assert [int(d.plan.results[g[k]]["n_scheduled"]) for k in ("a", "ten", "b")] == [110, 10, 110]
    assert all(short[g[k]] < full[g[k]] for k in ("a", "ten", "b"))


def test_groups_without_a_sum(dev):
    """An empty group, one whose pods fit no node, one cut by the prefix protocol and the one
    after it: +0.0 with the sign bit clear; their neighbours are summed."""
    d = dev(P.slots_case())
    out = d.run(0)
    got = d.check(0)
    g = d.c.index
    st = out.results["status"].tolist()
    assert st[g["cut"]] == abi.CA_EUNSUPPORTED and st[g["after"]] == abi.CA_ENOTRUN
    for k in ("empty", "huge", "cut", "after"):
        assert got[g[k]] == 0.0 and not np.signbit(got[g[k]]), k
    assert all(got[g[k]] > 0 for k in ("first", "second", "third"))
    # a NaN price on a pod that only the groups without a sum hold changes nothing
    price = d.c.price.copy()
    price[[i for i, p in enumerate(d.c.pods) if p.name in ("huge0", "huge1", "spread")]] = math.nan
    assert d.check(0, price).tobytes() == got.tobytes()


def test_planted_specials(dev):
    """Subnormals stay subnormal, -0.0 alone sums to +0.0, 1e308 twice overflows to +inf, +inf and
    -inf in one list and a NaN price give NaN."""
    d = dev(P.specials_case())
    d.run(0)
    got = d.check(0)
    g = d.c.index
    tiny = np.finfo(np.float64).tiny
    assert 0.0 < got[g["subnormal"]] < tiny and got[g["subnormal"]] == math.fsum(P.SUBNORMALS)
    assert got[g["negzero"]] == 0.0 and not np.signbit(got[g["negzero"]])
    assert math.isfinite(got[g["big"]]) and got[g["overflow"]] == math.inf and got[g["pinf"]] == math.inf
    assert math.isnan(got[g["infnan"]]) and math.isnan(got[g["nan"]])
    assert math.isfinite(got[g["plain"]])


def test_buffer_shorter_than_one_quad(dev):
    """Three list positions in all: the kernel loads whole 16-byte quads inside the buffer, so a
    buffer without one is summed by the library's host code, in the same order."""
    pods = P.small_pods(3)
    case = P.PriceCase("tiny", pods, [(k8s.build_test_node(*P.T_WIDE), []) for _ in range(3)],
                       [pods[:1], [], pods[1:]], P.random_prices(random.Random(3), 3), {})
    d = dev(case)
    d.run(0)
    got = d.check(0)
    assert got[1] == 0.0 and not np.signbit(got[1]) and got[0] > 0 and got[2] > 0
    assert d.plan.option_price_sums_ms() == 0.0
    d.check(0, np.array([math.nan, 5e-324, -0.0]))
    # and the smallest buffer the kernel takes: one quad, one list ending at the buffer's end
    pods = P.small_pods(5)
    for groups in ([pods[:1], pods[1:4]], [pods[:2], pods[2:5]], [pods[:3], pods[:3]], [pods[:3], pods[1:5]],
                   [[], pods[:4]]):         # 4, 5, 6, 7 and 4 positions: the last quad shifted by 0..3
        case = P.PriceCase("quad", pods, [(k8s.build_test_node(*P.T_WIDE), []) for _ in groups], groups,
                           P.random_prices(random.Random(4), 5), {})
        q = dev(case)
        q.run(0)
        q.check(0)
        assert q.plan.option_price_sums_ms() > 0.0


def test_more_options_than_a_block_holds(dev):
    """300 options, most of one to seven pods, a few of several chunks among them: more waves
    than a block holds and more blocks than one."""
    assert 300 > 8 * native.PRICE_SUMS_WAVES
    d = dev(P.many_case())
    d.run(0)
    got = d.check(0)
    assert len(got) == 300
    d.run(1)
    d.check(1)


def test_both_go_order_paths(dev, monkeypatch):
    """Lists left by the decoupled run-table path and by the coupled path (CASIM_GO_DECOUPLE=0):
    the list order comes from them, and the sum follows it."""
    d = dev(P.uniform_case())
    for limit in d.c.limits:
        d.run(limit)
        assert d.plan.stats()["decoupled"]
        d.check(limit)
    monkeypatch.setenv("CASIM_GO_DECOUPLE", "0")
    for limit in d.c.limits:
        d.run(limit)
        assert not d.plan.stats()["decoupled"]
        d.check(limit)


def test_codes(dev):
    d = dev(P.slots_case())
    price = d.c.price
    with pytest.raises(native.CasimError) as e:              # before any run
        d.plan.option_price_sums(price)
    assert e.value.status == abi.CA_ESTATE
    assert d.plan.option_price_sums_ms() == 0.0
    # a run whose zero-copy publisher delivered leaves no final lists
    saw_published = False
    for mode in ("host32", "u16"):
        d.plan.run(0, 0, want_nodes=False) if mode == "host32" else d.plan.run_u16(0, 0)
        if d.plan.stats()["results_path"] == "published":
            saw_published = True
            with pytest.raises(native.CasimError) as e:
                d.plan.option_price_sums(price)
            assert e.value.status == abi.CA_ESTATE
        else:
            d.check(0)
    assert saw_published
    d.run(0)
    for bad in (price[:-1], np.concatenate([price, [1.0]]), np.zeros(0)):
        with pytest.raises(native.CasimError) as e:
            d.plan.option_price_sums(bad)
        assert e.value.status == abi.CA_EINVAL
    lib, out = d.plan.lib, np.zeros(d.plan.G, np.float64)
    call = lib.ca_estimate_plan_option_price_sums
    assert call(None, price.ctypes.data, len(price), out.ctypes.data) == abi.CA_EINVAL
    assert call(d.plan.h, None, len(price), out.ctypes.data) == abi.CA_EINVAL
    assert call(d.plan.h, price.ctypes.data, len(price), None) == abi.CA_EINVAL
    assert lib.ca_estimate_plan_option_price_sums_ms(d.plan.h, None) == abi.CA_EINVAL
    ms = C.c_float(-1)
    assert lib.ca_estimate_plan_option_price_sums_ms(d.plan.h, C.byref(ms)) == abi.CA_OK and ms.value >= 0
    d.check(0)


# -- end to end ---------------------------------------------------------------------------------
class LinearPricing:
    """A pricing model linear in the requests, with a per-name factor so that sums round; pods
    whose name hashes to `fail_mod` have no price."""

    def __init__(self, fail_mod=0):
        self.fail_mod = fail_mod

    @staticmethod
    def _h(name):
        return zlib.crc32(name.encode())

    def NodePrice(self, node, start, end):  # noqa: N802
        cap = node.get_capacity()
        cpu, mem = Quantity(cap.get("cpu", 0)).milli_value(), Quantity(cap.get("memory", 0)).value()
        return (cpu * 0.031 + mem / (1 << 30) * 0.0042) * (1.0 + (self._h(node.name) % 9) / 64.0)

    def PodPrice(self, pod, start, end):  # noqa: N802
        if self.fail_mod and self._h(pod.name) % self.fail_mod == 0:
            raise PricingError(f"no price for {pod.name}")
        cpu = mem = 0
        for ct in pod.containers:
            cpu += Quantity(ct.requests.get("cpu", 0)).milli_value()
            mem += Quantity(ct.requests.get("memory", 0)).value()
        return (cpu * 0.0317 + mem / (1 << 30) * 0.00425) * (1.0 + (self._h(pod.name) % 1000) / 7919.0)


class _First:
    def BestOption(self, options, node_infos):  # noqa: N802
        return options[0] if options else None


class _Lister:
    def __init__(self, n):
        self.n = n

    def List(self):  # noqa: N802
        return [None] * self.n


def _chain(seed):
    # every third seed: some pods have no price, so their options are skipped
    return ChainStrategy([PriceBased(LinearPricing(fail_mod=29 if seed % 3 == 2 else 0),
                                     SimplePreferredNodeProvider(_Lister(3 * seed)), SimpleNodeUnfitness)], _First())


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
def test_compute_best_expansion_option_with_the_price_filter(seed):
    """ComputeBestExpansionOption (lists resident, totals from the device) against the host chain
    (PriceBased.BestOptions) over ComputeExpansionOptions' lists: same winner, same pods."""
    res = []
    for device_form in (False, True):
        nodes, pods, infos = _options_inputs(seed)
        snap = ClusterSnapshot(native.Mirror(0))
        snap.AddNodes(nodes)
        pc = SchedulerBasedPredicateChecker()
        pc.last_index = seed % 3
        groups = BuildPodGroups(pods)
        lim = ThresholdBasedEstimationLimiter(max_nodes=7)
        chain = _chain(seed)
        if device_form:
            best, feas = ComputeBestExpansionOption(snap, pc, groups, infos, lim, chain)
        else:
            opts, feas = ComputeExpansionOptions(snap, pc, groups, infos, lim)
            valid = [o for o in opts if len(o.pods) > 0 and o.node_count > 0]
            best = chain.BestOption(valid, dict(infos)) if valid else None
        res.append((None if best is None else (best.node_group, best.node_count, [p.name for p in best.pods]),
                    feas.tobytes(), pc.last_index, pc.evals))
        snap.backend.close()
    print(seed, res[1][0] and (res[1][0][0], res[1][0][1], len(res[1][0][2])))
    assert res[0] == res[1]


def _balanced_inputs(seed):
    rng = random.Random(100 + seed)
    pods = []
    for rs, (cpu, mem) in enumerate([(500, 1), (300, 1), (1200, 3), (150, 2)]):
        for i in range(rng.randint(4, 30)):
            p = k8s.build_test_pod(f"rs{rs}-{seed}-{i}", cpu, mem * P.GI)
            p.owner_refs = [OwnerReference("ReplicaSet", f"rs{rs}", f"rs{rs}")]
            pods.append(p)
    rng.shuffle(pods)
    groups = []
    for shape, (cpu, mem) in (("std", (4000, 8)), ("big", (16000, 64)), ("tiny", (1000, 4))):
        for zone in "abc"[: rng.randint(1, 3)]:
            n = k8s.build_test_node(f"t-{shape}-{zone}", cpu, mem * P.GI, 110)
            n.labels.update({"topology.kubernetes.io/zone": zone, "pool": shape})
            groups.append((NodeGroup(f"ng-{shape}-{zone}", rng.randint(0, 3), 40), NodeInfo(n, [])))
    return [], pods, groups


def _host_flow(snap, pc, pod_groups, node_groups, lim, chain, proc):
    """ScaleUp's path from the options to the plan on host lists (orchestrator.go:139-313)."""
    infos = {ng.Id(): info for ng, info in node_groups}
    opts, feas = ComputeExpansionOptions(snap, pc, pod_groups, node_groups, lim)
    options = {o.node_group.Id(): o for o in opts if len(o.pods) > 0 and o.node_count > 0}
    if not options:
        return None, [], feas
    best = chain.BestOption(list(options.values()), infos)
    if best is None:
        return None, [], feas
    similar = proc.FindSimilarNodeGroups([ng for ng, _ in node_groups], best.node_group, infos)
    kept = filter_node_groups_by_pods(similar, best.pods, options)
    return best, proc.BalanceScaleUpBetweenGroups([best.node_group] + kept, best.node_count), feas


@pytest.mark.parametrize("seed", range(6))
def test_compute_balanced_scale_up_with_the_price_filter(seed):
    """ComputeBalancedScaleUp with the price filter in the chain against the same flow on host
    lists: same winner, same pods, same ScaleUpInfos."""
    res = []
    for device_form in (False, True):
        nodes, pods, node_groups = _balanced_inputs(seed)
        snap = ClusterSnapshot(native.Mirror(0))
        pc = SchedulerBasedPredicateChecker()
        lim = ThresholdBasedEstimationLimiter(max_nodes=0)
        flow = ComputeBalancedScaleUp if device_form else _host_flow
        best, plan, feas = flow(snap, pc, BuildPodGroups(pods), node_groups, lim, _chain(seed),
                                BalancingNodeGroupSetProcessor())
        res.append((None if best is None else (best.node_group.Id(), best.node_count, [p.name for p in best.pods]),
                    [(i.Group.Id(), i.CurrentSize, i.NewSize, i.MaxSize) for i in plan], feas.tobytes(),
                    pc.last_index, pc.evals))
        snap.backend.close()
    print(seed, res[1][0] and (res[1][0][0], res[1][0][1], len(res[1][0][2])), res[1][1])
    assert res[0] == res[1]


def test_price_filter_needs_the_api_objects(dev):
    from autoscaler_amd.expander import DeviceOptions
    d = dev(P.slots_case())
    out = d.run(0)
    flt = PriceBased(LinearPricing(), SimplePreferredNodeProvider(_Lister(1)), SimpleNodeUnfitness)
    with pytest.raises(TypeError, match="pods="):
        flt.best_indices(DeviceOptions(d.plan, out.results, [0] * d.plan.G, [0] * d.plan.G), [0])
    # and with them: the totals are cached per pricing model and equal the host loop's
    groups = [f"g{g}" for g in range(d.plan.G)]
    infos = {g: NodeInfo(t) for g, (t, _) in zip(groups, d.c.templates)}
    opts = DeviceOptions(d.plan, out.results, [0] * d.plan.G, [0] * d.plan.G, pods=d.c.pods, node_groups=groups,
                         node_infos=infos)
    totals = opts.price_sums(flt.pricing_model)
    assert opts.price_sums(flt.pricing_model) is totals
    _, lists = d.lists(0)
    price = np.array([flt.pricing_model.PodPrice(p, 0, 0) for p in d.c.pods])
    assert_same_bits(totals, P.expected(price, lists))
