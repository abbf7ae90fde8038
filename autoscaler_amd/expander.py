"""ExpanderStrategy.BestOption for the least-waste and most-pods filters (CA/expander).

Two forms of each filter:

* the host form carries the reference's signature, ``BestOptions(options, node_infos)`` over
  ``scaleup.ExpansionOption`` objects and a {node group id: NodeInfo} map.  It restates
  waste.go:36-94 and mostpods.go:33-53 at the API level (Quantity sums of the pods' container
  requests, the node's Capacity) and is what the tests compare the device form against;
* the device form, ``best_indices(dev, options)``, works on an Estimate plan whose pod lists
  stayed in device memory (``DeviceOptions``): the per-option request sums come from
  ``EstimatePlan.option_sums`` (one kernel over the resident lists) and the filter loop is
  the library's ``ca_expander_best_options``.  Options are indices into the plan's groups.

``ChainStrategy`` is expander/factory/chain.go:37-46: filters in order, the first that leaves
one option decides, otherwise the caller's fallback strategy (the reference's is random)
picks among the rest.  The price, priority and gRPC expanders stay with the caller.  What
follows BestOption when similar node groups are balanced (FindSimilarNodeGroups,
filterNodeGroupsByPods on the same resident lists, BalanceScaleUpBetweenGroups) is
``nodegroupset.py`` and ``scaleup.ComputeBalancedScaleUp``.

Requests are summed on the device as per-pod MilliValue / Value int64s (the podset's
containers-only score fields): equal to the reference's Quantity sums when every request is
a whole milli-unit, and the sums must stay below 2^63.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from . import abi, native
from .k8s import Quantity

__all__ = ["LeastWaste", "MostPods", "ChainStrategy", "DeviceOptions", "wasted_score", "resources_for_pods",
           "resources_for_node"]


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
    are computed once, when a filter first needs them."""

    def __init__(self, plan: "native.EstimatePlan", results: np.ndarray, cap_milli_cpu, cap_memory):
        self.plan = plan
        self.results = results
        self.cap_milli_cpu = np.ascontiguousarray(cap_milli_cpu, dtype=np.int64)
        self.cap_memory = np.ascontiguousarray(cap_memory, dtype=np.int64)
        self._sums = None

    def sums(self) -> tuple:
        if self._sums is None:
            self._sums = self.plan.option_sums()
        return self._sums


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
