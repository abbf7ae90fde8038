"""The price expander's host form (autoscaler_amd/expander.py PriceBased, price.go:90-187) on the
reference's own test cases, transcribed as data in tests/golden/price_cases.json
(TestPriceExpander, TestPreferredNode, TestSimpleNodeUnfitness), and the corners of the loop
the reference's cases do not reach."""
import json
import math
import os

import numpy as np
import pytest

from autoscaler_amd import k8s
from autoscaler_amd.clustersnapshot import NodeInfo
from autoscaler_amd.expander import (ChainStrategy, DeviceOptions, PriceBased, PricingError, SimpleNodeUnfitness,
                                     SimplePreferredNodeProvider, node_has_gpu)
from autoscaler_amd.scaleup import ExpansionOption

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "price_cases.json")))
GI = 1 << 30


class TablePricing:
    """testPricingModel (price_test.go:37-54): prices by name, an error for a missing one."""

    def __init__(self, node_price, pod_price):
        self.node_price, self.pod_price = node_price, pod_price

    def NodePrice(self, node, start, end):  # noqa: N802
        if node.name not in self.node_price:
            raise PricingError(f"price for node {node.name} not found")
        return self.node_price[node.name]

    def PodPrice(self, pod, start, end):  # noqa: N802
        if pod.name not in self.pod_price:
            raise PricingError(f"price for pod {pod.name} not found")
        return self.pod_price[pod.name]


class Preferred:
    def __init__(self, node):
        self.node = node

    def Node(self):  # noqa: N802
        if self.node is None:
            raise RuntimeError("no preferred node")
        return self.node


class Group:
    def __init__(self, gid, exist=True):
        self.gid, self.exist = gid, exist

    def Id(self):  # noqa: N802
        return self.gid

    def Exist(self):  # noqa: N802
        return self.exist


def _preferred(cpu, mem):
    n = k8s.build_test_node("CA-PreferredNode", cpu, mem)
    return Preferred(n)


@pytest.mark.parametrize("case", CASES["price_expander"], ids=lambda c: c["name"])
def test_price_expander_reference_cases(case):
    nodes = {k: k8s.build_test_node(k, *v) for k, v in CASES["nodes"].items()}
    pods = {k: k8s.build_test_pod(k, *v) for k, v in CASES["pods"].items()}
    groups = {k: Group(v["id"], v["exist"]) for k, v in CASES["groups"].items()}
    infos = {CASES["groups"][k]["id"]: NodeInfo(nodes[CASES["groups"][k]["node"]]) for k in case["node_infos"]}
    options = [ExpansionOption(groups[o["group"]], o["count"], [pods[p] for p in o["pods"]]) for o in case["options"]]
    debug = {id(opt): o["debug"] for opt, o in zip(options, case["options"])}
    flt = PriceBased(TablePricing(case["node_price"], case["pod_price"]), _preferred(*case["preferred"]),
                     SimpleNodeUnfitness)
    assert [debug[id(o)] for o in flt.BestOptions(options, infos)] == case["expected"]


@pytest.mark.parametrize("size,cpus", CASES["preferred_node"])
def test_preferred_node(size, cpus):
    class Lister:
        def List(self):  # noqa: N802
            return [k8s.build_test_node("n1", 1000, 1000) for _ in range(size)]
    node = SimplePreferredNodeProvider(Lister()).Node()
    assert k8s.Quantity(node.get_capacity()["cpu"]).value() == cpus
    assert node.get_capacity() == node.allocatable and k8s.Quantity(node.allocatable["pods"]).value() == 100


def test_simple_node_unfitness():
    for c in CASES["simple_node_unfitness"]:
        a, b = k8s.build_test_node("a", *c["preferred"]), k8s.build_test_node("b", *c["evaluated"])
        assert SimpleNodeUnfitness(a, b) == c["want"]
    # a node without cpu capacity: 0 / x and x / 0, Go's math.Max of 0 and +Inf
    none = k8s.build_test_node("none", -1, 1000)
    assert SimpleNodeUnfitness(none, k8s.build_test_node("b", 1000, 1000)) == math.inf
    assert math.isnan(SimpleNodeUnfitness(none, none))


# -- corners ------------------------------------------------------------------------------------
def _setup(n_groups=3, cpu=2000):
    nodes = [k8s.build_test_node(f"n{g}", cpu, GI) for g in range(n_groups)]
    groups = [Group(f"ng{g}") for g in range(n_groups)]
    infos = {f"ng{g}": NodeInfo(nodes[g]) for g in range(n_groups)}
    pods = [k8s.build_test_pod(f"p{i}", 100, 0) for i in range(4)]
    return nodes, groups, infos, pods


def _flt(node_price, pod_price, preferred=(2000, GI), **kw):
    return PriceBased(TablePricing(node_price, pod_price), _preferred(*preferred), SimpleNodeUnfitness, **kw)


def test_ties_keep_both_options_in_input_order():
    _, groups, infos, pods = _setup()
    options = [ExpansionOption(groups[g], 1, pods[:2]) for g in (2, 0, 1)]
    flt = _flt({"n0": 50.0, "n1": 70.0, "n2": 50.0}, {"p0": 5.0, "p1": 6.0, "stabilize": 1.0})
    assert [o.node_group.Id() for o in flt.BestOptions(options, infos)] == ["ng2", "ng0"]


def test_first_option_is_kept_at_score_nan():
    """len(bestOptions) == 0 comes first: a NaN score (0 / 0 without a stabilization price) is
    kept as the first option and then beaten by nothing, as NaN compares false both ways."""
    _, groups, infos, pods = _setup()
    options = [ExpansionOption(groups[0], 0, []), ExpansionOption(groups[1], 1, pods[:1])]
    flt = _flt({"n0": 10.0, "n1": 10.0}, {"p0": 5.0})            # no "stabilize": continuing without
    got = flt.BestOptions(options, infos)
    assert [o.node_group.Id() for o in got] == ["ng0"]
    got = flt.BestOptions(options[::-1], infos)                  # second: neither == nor >
    assert [o.node_group.Id() for o in got] == ["ng1"]


def test_options_without_node_info_or_node_price_are_skipped():
    _, groups, infos, pods = _setup()
    del infos["ng0"]
    options = [ExpansionOption(groups[g], 1, pods[:2]) for g in range(3)]
    flt = _flt({"n0": 1.0, "n2": 30.0}, {"p0": 5.0, "p1": 6.0, "stabilize": 1.0})
    assert [o.node_group.Id() for o in flt.BestOptions(options, infos)] == ["ng2"]


def test_default_preferred_node_when_the_provider_fails():
    nodes = [k8s.build_test_node("n0", 4000, GI), k8s.build_test_node("n1", 2000, GI)]
    groups = [Group("ng0"), Group("ng1")]
    infos = {"ng0": NodeInfo(nodes[0]), "ng1": NodeInfo(nodes[1])}
    pods = [k8s.build_test_pod("p0", 100, 0)]
    options = [ExpansionOption(groups[g], 1, pods) for g in range(2)]
    flt = PriceBased(TablePricing({"n0": 10.0, "n1": 10.0}, {"p0": 5.0, "stabilize": 1.0}), Preferred(None),
                     SimpleNodeUnfitness)
    assert [o.node_group.Id() for o in flt.BestOptions(options, infos)] == ["ng0"]     # 4 cpu is the default


def test_gpu_override_ignores_the_preferred_node():
    """A GPU node group scores 1000 x the price ratio whatever the preferred shape: with equal
    prices the preferred-shaped GPU group loses to an unfit plain one."""
    gpu_node, plain = k8s.build_test_node("n0", 2000, GI), k8s.build_test_node("n1", 32000, GI)
    k8s.add_gpus_to_node(gpu_node, 1)
    assert node_has_gpu(None, gpu_node) and not node_has_gpu(None, plain)
    assert node_has_gpu("cloud.google.com/gke-accelerator", gpu_node) and not node_has_gpu("x", plain)
    labelled = k8s.build_test_node("n2", 2000, GI)
    labelled.labels["accel"] = "yes"
    assert node_has_gpu("accel", labelled) and not node_has_gpu(None, labelled)
    groups = [Group("ng0"), Group("ng1"), Group("ng2")]
    infos = {"ng0": NodeInfo(gpu_node), "ng1": NodeInfo(plain), "ng2": NodeInfo(labelled)}
    pods = [k8s.build_test_pod("p0", 100, 0)]
    options = [ExpansionOption(g, 1, pods) for g in groups]
    prices = ({"n0": 10.0, "n1": 10.0, "n2": 10.0}, {"p0": 5.0, "stabilize": 1.0})
    assert [o.node_group.Id() for o in _flt(*prices).BestOptions(options, infos)] == ["ng2"]
    assert [o.node_group.Id() for o in _flt(*prices, gpu_label="accel").BestOptions(options, infos)] == ["ng1"]
    flt = _flt(*prices, gpu_label="accel")
    score = flt.option_score(10.0, 1, 5.0, 1.0, k8s.build_test_node("pref", 2000, GI), gpu_node, True)
    assert score == 1000.0 * (11.0 / 6.0)


def test_not_exist_doubles_the_score():
    flt = _flt({}, {})
    node, pref = k8s.build_test_node("n", 2000, GI), k8s.build_test_node("pref", 2000, GI)
    a = flt.option_score(200.0, 1, 30.0, 10.0, pref, node, True)
    assert a == 210.0 / 40.0 and flt.option_score(200.0, 1, 30.0, 10.0, pref, node, False) == 2.0 * a
    # the suppression: (unfitness - 1) * (1 - tanh((count - 1) / 15)) + 1
    wide = k8s.build_test_node("w", 8000, GI)
    want = ((4.0 - 1.0) * (1.0 - math.tanh(39.0 / 15.0)) + 1.0) * (8010.0 / 40.0)
    assert flt.option_score(200.0, 40, 30.0, 10.0, pref, wide, True) == want


def test_chain_with_an_empty_price_result_reaches_the_fallback():
    seen = []

    class Fallback:
        def BestOption(self, options, node_infos):  # noqa: N802
            seen.append(list(options))
            return None

    _, groups, infos, pods = _setup()
    options = [ExpansionOption(groups[g], 1, pods[:2]) for g in range(3)]
    chain = ChainStrategy([_flt({}, {})], Fallback())
    assert chain.BestOption(options, infos) is None and seen == [[]]


# -- the device form's loop, on given totals ------------------------------------------------------
class _Totals(DeviceOptions):
    """DeviceOptions with the totals given (no plan): what best_indices does with them."""

    def __init__(self, totals, results, pods, node_groups, node_infos):
        super().__init__(None, results, [0] * len(totals), [0] * len(totals), pods=pods, node_groups=node_groups,
                         node_infos=node_infos)
        self.totals = np.asarray(totals, np.float64)

    def price_sums(self, pricing_model, start=None, end=None):
        return self.totals


def _results(counts):
    from autoscaler_amd import abi
    r = np.zeros(len(counts), abi.ESTIMATE_RESULT_DTYPE)
    r["node_count"] = counts
    return r


def test_nan_total_skips_the_option():
    _, groups, infos, pods = _setup()
    flt = _flt({"n0": 1.0, "n1": 50.0, "n2": 60.0}, {"stabilize": 1.0})
    dev = _Totals([np.nan, 11.0, 11.0], _results([1, 1, 1]), pods, groups, infos)
    assert flt.best_indices(dev, [0, 1, 2]).tolist() == [1]
    dev = _Totals([np.nan] * 3, _results([1, 1, 1]), pods, groups, infos)
    assert flt.best_indices(dev, [0, 1, 2]).tolist() == []
    assert flt.best_indices(dev, []).tolist() == []


def test_device_loop_equals_host_loop_on_the_reference_cases():
    nodes = {k: k8s.build_test_node(k, *v) for k, v in CASES["nodes"].items()}
    for case in CASES["price_expander"]:
        names = [o["group"] for o in case["options"]]
        groups = [Group(CASES["groups"][k]["id"], CASES["groups"][k]["exist"]) for k in names]
        infos = {CASES["groups"][k]["id"]: NodeInfo(nodes[CASES["groups"][k]["node"]]) for k in case["node_infos"]}
        totals = []
        for o in case["options"]:
            t = 0.0
            for p in o["pods"]:
                t += case["pod_price"].get(p, math.nan)
            totals.append(t)
        dev = _Totals(totals, _results([o["count"] for o in case["options"]]), [], groups, infos)
        flt = _flt(case["node_price"], case["pod_price"], tuple(case["preferred"]))
        got = flt.best_indices(dev, list(range(len(names)))).tolist()
        assert [case["options"][g]["debug"] for g in got] == case["expected"], case["name"]


def test_best_indices_without_the_api_objects_is_a_type_error():
    dev = DeviceOptions(None, _results([1]), [0], [0])
    with pytest.raises(TypeError, match="pods="):
        _flt({}, {}).best_indices(dev, [0])
    with pytest.raises(TypeError, match="pods="):
        dev.price_sums(TablePricing({}, {}))
