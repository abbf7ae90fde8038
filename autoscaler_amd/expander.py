"""ExpanderStrategy.BestOption for the least-waste, most-pods and price filters (CA/expander).

Two forms of each filter:

* the host form carries the reference's signature, ``BestOptions(options, node_infos)`` over
  ``scaleup.ExpansionOption`` objects and a {node group id: NodeInfo} map.  It restates
  waste.go:36-94 and mostpods.go:33-53 at the API level (Quantity sums of the pods' container
  requests, the node's Capacity) and is what the tests compare the device form against;
* the device form, ``best_indices(dev, options)``, works on an Estimate plan whose pod lists
  stayed in device memory (``DeviceOptions``): the per-option request sums come from
  ``EstimatePlan.option_sums`` (one kernel over the resident lists) and the filter loop is
  the library's ``ca_expander_best_options``.  Options are indices into the plan's groups.

``PriceBased`` is expander/price (price.go:90-187, preferred.go): the host form is the
reference's loop over API objects and a pricing model; the device form takes every option's
totalPodPrice — a float64 sum the reference adds left to right — from
``EstimatePlan.option_price_sums`` (one wave per option adds the resident list's prices in
list order, bit for bit the host loop's sum) and runs the same scoring loop over option
indices.  A pod whose PodPrice raised ``PricingError`` is priced NaN there: its options' totals
are NaN and they are skipped, the reference's ``continue nextoption`` — so a pricing model must
not return NaN.  Both forms use ``math.tanh`` where the reference uses Go's ``math.Tanh``; the
two may differ in the last ulp, which matters only to scores within an ulp of a tie.

``ChainStrategy`` is expander/factory/chain.go:37-46: filters in order, the first that leaves
one option decides, otherwise the caller's fallback strategy (the reference's is random)
picks among the rest.  The priority, random and gRPC expanders stay with the caller.  What
follows BestOption when similar node groups are balanced (FindSimilarNodeGroups,
filterNodeGroupsByPods on the same resident lists, BalanceScaleUpBetweenGroups) is
``nodegroupset.py`` and ``scaleup.ComputeBalancedScaleUp``.

Requests are summed on the device as per-pod MilliValue / Value int64s (the podset's
containers-only score fields): equal to the reference's Quantity sums when every request is
a whole milli-unit, and the sums must stay below 2^63.
"""
from __future__ import annotations

import math
import time
from fractions import Fraction

import numpy as np

from . import abi, native
from .k8s import Quantity

__all__ = ["LeastWaste", "MostPods", "PriceBased", "PricingError", "SimplePreferredNodeProvider",
           "SimpleNodeUnfitness", "ChainStrategy", "DeviceOptions", "wasted_score", "resources_for_pods",
           "resources_for_node", "node_has_gpu"]


def _group_id(node_group):
    return node_group.Id() if hasattr(node_group, "Id") else node_group


def _wrap64(v: int) -> int:
    """Go int64 arithmetic wraps."""
    return ((int(v) + (1 << 63)) % (1 << 64)) - (1 << 63)


def resources_for_pods(pods: list) -> tuple:
    """resourcesForPods (waste.go:74-87): Quantity sums over the pods' containers, then
    MilliValue() / Value()."""
    c, m = Fraction(0), Fraction(0)
    for pod in pods:
        for ct in pod.containers:
            if "cpu" in ct.requests:
                c += Quantity(ct.requests["cpu"]).v
            if "memory" in ct.requests:
                m += Quantity(ct.requests["memory"]).v
    return Quantity(c).milli_value(), Quantity(m).value()


def resources_for_node(node) -> tuple:
    """resourcesForNode (waste.go:89-94): the node's Capacity (a missing resource is the zero
    Quantity), as MilliValue() / Value()."""
    cap = node.get_capacity()
    return Quantity(cap.get("cpu", 0)).milli_value(), Quantity(cap.get("memory", 0)).value()


def wasted_score(cap_milli_cpu: int, cap_memory: int, node_count: int, req_milli_cpu: int, req_memory: int):
    """wastedScore of one option (waste.go:49-53): int64 products and differences, IEEE
    float64 conversions, divisions and sum — NaN for 0 / 0, an infinity for x / 0."""
    with np.errstate(all="ignore"):
        avail_cpu = _wrap64(int(cap_milli_cpu) * int(node_count))
        avail_mem = _wrap64(int(cap_memory) * int(node_count))
        wasted_cpu = np.float64(_wrap64(avail_cpu - int(req_milli_cpu))) / np.float64(avail_cpu)
        wasted_mem = np.float64(_wrap64(avail_mem - int(req_memory))) / np.float64(avail_mem)
        return wasted_cpu + wasted_mem


def least_waste_indices(scores) -> list:
    """The loop of waste.go:37-71 over the options' scores: surviving positions."""
    least = np.float64(0)
    best = None
    with np.errstate(all="ignore"):
        for k, s in enumerate(scores):
            if s == least:
                best = (best or []) + [k]
            if best is None or s < least:
                least = s
                best = [k]
    return best or []


def most_pods_indices(counts) -> list:
    """The loop of mostpods.go:34-52 over the options' pod counts: surviving positions."""
    max_pods = 0
    best = None
    for k, n in enumerate(counts):
        if n == max_pods:
            best = (best or []) + [k]
        if n > max_pods:
            max_pods = n
            best = [k]
    return best or []


class DeviceOptions:
    """The options of one Estimate plan run whose lists stayed in device memory: the plan, its
    results and the node groups' Capacity (milli cpu, memory) per group.  The request sums
    are computed once, when a filter first needs them.  The price filter also needs the API
    objects: `pods` (the plan's pod table, one Pod per pod-set index), `node_groups` (one per
    plan group) and `node_infos` ({node group id: NodeInfo})."""

    def __init__(self, plan: "native.EstimatePlan", results: np.ndarray, cap_milli_cpu, cap_memory, *,
                 pods: list = None, node_groups: list = None, node_infos: dict = None):
        self.plan = plan
        self.results = results
        self.cap_milli_cpu = np.ascontiguousarray(cap_milli_cpu, dtype=np.int64)
        self.cap_memory = np.ascontiguousarray(cap_memory, dtype=np.int64)
        self.pods = pods
        self.node_groups = node_groups
        self.node_infos = node_infos
        self._sums = None
        self._price_sums = {}

    def sums(self) -> tuple:
        if self._sums is None:
            self._sums = self.plan.option_sums()
        return self._sums

    def price_sums(self, pricing_model, start=None, end=None) -> np.ndarray:
        """totalPodPrice of every option under `pricing_model` (price.go:126-134): PodPrice once
        per pod of the plan's pod table (NaN where it raised PricingError), one
        option_price_sums call; kept per pricing model."""
        if self.pods is None:
            raise TypeError("DeviceOptions.price_sums needs the plan's pods: pass pods= to DeviceOptions")
        got = self._price_sums.get(id(pricing_model))
        if got is None:
            if start is None:
                start = time.time()
                end = start + 3600.0
            price = np.empty(len(self.pods), np.float64)
            for i, pod in enumerate(self.pods):
                try:
                    price[i] = pricing_model.PodPrice(pod, start, end)
                except PricingError:
                    price[i] = np.nan
            got = (pricing_model, self.plan.option_price_sums(price))       # (the model is kept: its id stays its own)
            self._price_sums[id(pricing_model)] = got
        return got[1]


class LeastWaste:
    """expander/waste: the options that waste the least fraction of cpu plus memory."""

    def scores(self, options: list, node_infos: dict) -> list:
        out = []
        for o in options:
            cpu, mem = resources_for_node(node_infos[_group_id(o.node_group)].Node())
            req_cpu, req_mem = resources_for_pods(o.pods)
            out.append(wasted_score(cpu, mem, o.node_count, req_cpu, req_mem))
        return out

    def BestOptions(self, options: list, node_infos: dict) -> list:  # noqa: N802
        known = [o for o in options if _group_id(o.node_group) in node_infos]      # waste.go:42-46
        return [known[k] for k in least_waste_indices(self.scores(known, node_infos))]

    def best_indices(self, dev: DeviceOptions, options) -> np.ndarray:
        req_cpu, req_mem = dev.sums()
        return native.expander_best_options(abi.CA_EXPANDER_LEAST_WASTE, dev.results, req_cpu, req_mem,
                                            dev.cap_milli_cpu, dev.cap_memory, options)[0]


class MostPods:
    """expander/mostpods: the options that schedule the most pods."""

    def BestOptions(self, options: list, node_infos: dict = None) -> list:  # noqa: N802
        return [options[k] for k in most_pods_indices([len(o.pods) for o in options])]

    def best_indices(self, dev: DeviceOptions, options) -> np.ndarray:
        return native.expander_best_options(abi.CA_EXPANDER_MOST_PODS, dev.results, None, None, None, None,
                                            options)[0]


class PricingError(Exception):
    """The error of cloudprovider.PricingModel.NodePrice / PodPrice."""


GPU_RESOURCE = "nvidia.com/gpu"                    # gpu.ResourceNvidiaGPU (utils/gpu/gpu.go:27)
NOT_EXIST_COEFFICIENT = 2.0                        # price.go:60
GPU_UNFITNESS_OVERRIDE = 1000.0                    # price.go:74


def node_has_gpu(gpu_label, node) -> bool:
    """gpu.NodeHasGpu (utils/gpu/gpu.go:100-104): the provider's GPU label on the node, or a
    non-zero nvidia.com/gpu allocatable."""
    if gpu_label is not None and gpu_label in node.labels:
        return True
    q = node.allocatable.get(GPU_RESOURCE)
    return q is not None and Quantity(q).v != 0


def _build_node(millicpu: int, mem: int):
    """buildNode (preferred.go:67-84): capacity == allocatable, 100 pods."""
    from .k8s import Node
    return Node(name="CA-PreferredNode", allocatable={"pods": Quantity(100), "cpu": Quantity.milli(millicpu),
                                                      "memory": Quantity(mem)})


def _build_pod(name: str, millicpu: int, mem: int):
    """buildPod (price.go:190-210)."""
    from .k8s import Container, Pod
    return Pod(name=name, containers=[Container(requests={"cpu": Quantity.milli(millicpu), "memory": Quantity(mem)})])


_MIB, _GIB = 1 << 20, 1 << 30
DEFAULT_PREFERRED_NODE = _build_node(4 * 1000, 4 * 4 * _GIB)             # price.go:51
PRICE_STABILIZATION_POD = _build_pod("stabilize", 500, 500 * _MIB)       # price.go:55


class SimplePreferredNodeProvider:
    """SimplePreferredNodeProvider (preferred.go:30-65): the preferred node doubles each time the
    cluster grows threefold.  `node_lister` has List() -> nodes."""

    def __init__(self, node_lister):
        self.node_lister = node_lister

    def Node(self):  # noqa: N802
        size = len(self.node_lister.List())
        cpu = 1000
        for limit, k in ((2, 1), (6, 2), (20, 4), (60, 8), (200, 16)):
            if size <= limit:
                return _build_node(k * cpu, k * 3750 * _MIB)
        return _build_node(32 * cpu, 120000 * _MIB)


def _go_div(a, b):
    """Go's float64 division: IEEE, no exception at a zero divisor."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _go_max(x: float, y: float) -> float:
    """math.Max (special cases first: an infinity wins over NaN)."""
    if math.isinf(x) and x > 0 or math.isinf(y) and y > 0:
        return math.inf
    if math.isnan(x) or math.isnan(y):
        return math.nan
    if x == 0 and x == y:
        return y if math.copysign(1.0, x) < 0 else x
    return x if x > y else y


def SimpleNodeUnfitness(preferred_node, evaluated_node) -> float:  # noqa: N802
    """SimpleNodeUnfitness (preferred.go:87-92): by Capacity cpu only."""
    pref = Quantity(preferred_node.get_capacity().get("cpu", 0)).milli_value()
    ev = Quantity(evaluated_node.get_capacity().get("cpu", 0)).milli_value()
    return _go_max(_go_div(float(pref), float(ev)), _go_div(float(ev), float(pref)))


class PriceBased:
    """expander/price (price.go:42-187).  `pricing_model` has NodePrice(node, start, end) and
    PodPrice(pod, start, end), each returning a float or raising PricingError;
    `preferred_node_provider` has Node() (any exception: the default preferred node, 4 cpu and
    16 GiB); `node_unfitness(preferred, evaluated)` -> float; `gpu_label` is the cloud
    provider's GPULabel()."""

    def __init__(self, pricing_model, preferred_node_provider, node_unfitness, gpu_label=None):
        self.pricing_model = pricing_model
        self.preferred_node_provider = preferred_node_provider
        self.node_unfitness = node_unfitness
        self.gpu_label = gpu_label

    def _begin(self):
        """price.go:93-111: (now, then, preferred node, stabilization price)."""
        now = time.time()
        then = now + 3600.0
        try:
            preferred = self.preferred_node_provider.Node()
        except Exception:                                       # :97-100
            preferred = DEFAULT_PREFERRED_NODE
        try:
            stabilization = float(self.pricing_model.PodPrice(PRICE_STABILIZATION_POD, now, then))
        except PricingError:                                    # :108-111 continuing without stabilization
            stabilization = 0.0
        return now, then, preferred, stabilization

    def option_score(self, node_price, node_count, total_pod_price, stabilization, preferred, node, exists) -> float:
        """price.go:125-159 for one option."""
        with np.errstate(all="ignore"):
            total_node_price = np.float64(node_price) * np.float64(float(int(node_count)))
            price_sub_score = ((total_node_price + np.float64(stabilization)) /
                               (np.float64(total_pod_price) + np.float64(stabilization)))
            unfitness = np.float64(self.node_unfitness(preferred, node))
            suppressed = ((unfitness - np.float64(1.0)) *
                          (np.float64(1.0) - np.float64(math.tanh(float(int(node_count) - 1) / 15.0))) + np.float64(1.0))
            if node_has_gpu(self.gpu_label, node):
                suppressed = np.float64(GPU_UNFITNESS_OVERRIDE)
            score = suppressed * price_sub_score
            if not exists:
                score = score * np.float64(NOT_EXIST_COEFFICIENT)
        return float(score)

    @staticmethod
    def _exists(node_group) -> bool:
        return node_group.Exist() if hasattr(node_group, "Exist") else True

    def _pick(self, candidates):
        """price.go:178-184 over (key, score) pairs: the `==` test before the `>` test; the first
        option is kept whatever its score."""
        best, best_score = [], 0.0
        for key, score in candidates:
            if len(best) == 0 or best_score == score:
                best.append(key)
                best_score = score
            elif best_score > score:
                best = [key]
                best_score = score
        return best

    def BestOptions(self, options: list, node_infos: dict) -> list:  # noqa: N802
        now, then, preferred, stabilization = self._begin()
        scored = []
        for option in options:
            info = node_infos.get(_group_id(option.node_group))
            if info is None:                                    # :115-119
                continue
            try:
                node_price = self.pricing_model.NodePrice(info.Node(), now, then)
            except PricingError:                                # :120-124
                continue
            total_pod_price = 0.0
            failed = False
            for pod in option.pods:                             # :126-134, left to right
                try:
                    total_pod_price += float(self.pricing_model.PodPrice(pod, now, then))
                except PricingError:
                    failed = True
                    break
            if failed:
                continue
            scored.append((option, self.option_score(node_price, option.node_count, total_pod_price, stabilization,
                                                     preferred, info.Node(), self._exists(option.node_group))))
        return self._pick(scored)

    def best_indices(self, dev: DeviceOptions, options) -> np.ndarray:
        if dev.pods is None or dev.node_groups is None or dev.node_infos is None:
            raise TypeError("PriceBased.best_indices needs the options' API objects: build DeviceOptions with "
                            "pods=, node_groups= and node_infos=")
        now, then, preferred, stabilization = self._begin()
        totals = dev.price_sums(self.pricing_model, now, then)
        scored = []
        for g in np.asarray(options, dtype=np.int64).tolist():
            node_group = dev.node_groups[g]
            info = dev.node_infos.get(_group_id(node_group))
            if info is None:
                continue
            try:
                node_price = self.pricing_model.NodePrice(info.Node(), now, then)
            except PricingError:
                continue
            total_pod_price = float(totals[g])
            if math.isnan(total_pod_price):                     # a PodPrice failed: `continue nextoption`
                continue
            scored.append((g, self.option_score(node_price, int(dev.results[g]["node_count"]), total_pod_price,
                                                stabilization, preferred, info.Node(), self._exists(node_group))))
        return np.array(self._pick(scored), dtype=np.int32)


class ChainStrategy:
    """chainStrategy (expander/factory/chain.go:25-46).  `fallback` is an expander.Strategy:
    an object with BestOption(options, node_infos)."""

    def __init__(self, filters: list, fallback):
        self.filters = list(filters)
        self.fallback = fallback

    def BestOption(self, options: list, node_infos: dict):  # noqa: N802
        filtered = options
        for f in self.filters:
            filtered = f.BestOptions(filtered, node_infos)
            if len(filtered) == 1:
                return filtered[0]
        return self.fallback.BestOption(filtered, node_infos)

    def best_indices(self, dev: DeviceOptions, options) -> np.ndarray:
        """The filters of BestOption over option indices: one index when a filter decided,
        else what is left for the fallback (the caller fetches those options' pods)."""
        filtered = np.ascontiguousarray(options, dtype=np.int32)
        for f in self.filters:
            filtered = f.best_indices(dev, filtered)
            if len(filtered) == 1:
                break
        return filtered
