"""Balancing a scale-up between similar node groups (CA/processors/nodegroupset and the
orchestrator's filterNodeGroupsByPods), restated at the API level.

* ``create_generic_node_info_comparator`` / ``is_cloud_provider_node_info_similar``
  (compare_nodegroups.go:46-155): two template NodeInfos are similar when their Capacity
  matches exactly (memory: within a ratio), their Allocatable and free resources are within a
  ratio and every label that is not ignored is on both nodes with one value;
* ``BalancingNodeGroupSetProcessor`` (balancing_processor.go:30-181): ``FindSimilarNodeGroups``
  and ``BalanceScaleUpBetweenGroups``, the loop literally, its ``sort.Slice`` through
  ``gosort.sort_slice`` so tied groups land where Go 1.19 puts them;
* ``filter_node_groups_by_pods`` (orchestrator.go:596-628) in two forms: the host form over
  ``ExpansionOption`` objects (pods by identity, as Go compares ``*apiv1.Pod``), and
  ``filter_plan_groups_by_pods`` over the groups of an Estimate plan whose lists stayed in
  device memory (``EstimatePlan.groups_missing_pods``: pods by pod-set index, so the plan's
  groups must index one shared pod table).

Everything but the device form is host code and needs no device.  The AWS / Azure / GCE / label
comparators stay with the caller.
"""
from __future__ import annotations

from dataclasses import dataclass, field

from . import gosort
from .intern import PodRequest
from .k8s import Quantity

__all__ = ["BASIC_IGNORED_LABELS", "NodeGroupDifferenceRatios", "is_cloud_provider_node_info_similar",
           "create_generic_node_info_comparator", "BalancingNodeGroupSetProcessor", "ScaleUpInfo", "NodeGroup",
           "BalanceError", "filter_node_groups_by_pods", "filter_plan_groups_by_pods", "requested_resource_list"]

# compare_nodegroups.go:32-40 (apiv1.LabelHostname, LabelZoneFailureDomain, LabelZoneRegion and
# their stable forms, then the two literal labels)
BASIC_IGNORED_LABELS = {
    "kubernetes.io/hostname": True,
    "failure-domain.beta.kubernetes.io/zone": True,
    "failure-domain.beta.kubernetes.io/region": True,
    "topology.kubernetes.io/zone": True,
    "topology.kubernetes.io/region": True,
    "beta.kubernetes.io/fluentd-ds-ready": True,
    "kops.k8s.io/instancegroup": True,
}


@dataclass
class NodeGroupDifferenceRatios:
    """config.NodeGroupDifferenceRatios with NewDefaultNodeGroupDifferenceRatios' values
    (config/autoscaling_options.go:50-55)."""
    max_allocatable_difference_ratio: float = 0.05
    max_free_difference_ratio: float = 0.05
    max_capacity_memory_difference_ratio: float = 0.015


def _q(v) -> Quantity:
    return v if isinstance(v, Quantity) else Quantity(v)


def requested_resource_list(node_info) -> dict:
    """scheduler.ResourceToResourceList(NodeInfo.Requested) (utils/scheduler/scheduler.go:93-108):
    cpu, memory, pods and ephemeral-storage always, then the scalar resources.  Requested is the
    sum of the pods' effective requests (containers, max with the init containers, plus
    overhead: intern.PodRequest); its AllowedPodNumber is 0."""
    cpu = mem = eph = 0
    scalar: dict = {}
    for pod in node_info.pods:
        r = PodRequest(pod)
        cpu += r.cpu
        mem += r.mem
        eph += r.eph
        for name, v in r.scalar.items():
            scalar[name] = scalar.get(name, 0) + v
    out = {"cpu": Quantity.milli(cpu), "memory": Quantity(mem), "pods": Quantity(0), "ephemeral-storage": Quantity(eph)}
    for name, v in scalar.items():
        out[name] = Quantity(v)
    return out


def _list_within_tolerance(qtys: list, ratio: float) -> bool:
    """resourceListWithinTolerance (:56-63): float64 of the MilliValues."""
    if len(qtys) != 2:
        return False
    a, b = float(qtys[0].milli_value()), float(qtys[1].milli_value())
    larger, smaller = max(a, b), min(a, b)
    return larger - smaller <= larger * ratio


def _maps_within_tolerance(resources: dict, ratio: float) -> bool:
    return all(_list_within_tolerance(q, ratio) for q in resources.values())


def _compare_labels(nodes: list, ignored: dict) -> bool:
    """compareLabels (:65-81)."""
    labels: dict = {}
    for info in nodes:
        for label, value in info.Node().labels.items():
            if not ignored.get(label, False):
                labels.setdefault(label, []).append(value)
    return all(len(v) == 2 and v[0] == v[1] for v in labels.values())


def is_cloud_provider_node_info_similar(n1, n2, ignored_labels: dict, ratios: NodeGroupDifferenceRatios) -> bool:
    """IsCloudProviderNodeInfoSimilar (compare_nodegroups.go:103-155)."""
    capacity: dict = {}
    allocatable: dict = {}
    free: dict = {}
    nodes = [n1, n2]
    for info in nodes:
        node = info.Node()
        for res, q in node.get_capacity().items():
            capacity.setdefault(res, []).append(_q(q))
        for res, q in node.allocatable.items():
            allocatable.setdefault(res, []).append(_q(q))
        for res, q in requested_resource_list(info).items():
            free.setdefault(res, []).append(Quantity(_q(node.allocatable.get(res, 0)).v - q.v))
    for kind, qtys in capacity.items():
        if len(qtys) != 2:
            return False
        if kind == "memory":
            if not _list_within_tolerance(qtys, ratios.max_capacity_memory_difference_ratio):
                return False
        elif qtys[0].v != qtys[1].v:          # other capacity types match exactly
            return False
    if not _maps_within_tolerance(allocatable, ratios.max_allocatable_difference_ratio):
        return False
    if not _maps_within_tolerance(free, ratios.max_free_difference_ratio):
        return False
    return _compare_labels(nodes, ignored_labels)


def create_generic_node_info_comparator(extra_ignored_labels=(), ratios: NodeGroupDifferenceRatios = None):
    """CreateGenericNodeInfoComparator (:84-96)."""
    ignored = dict(BASIC_IGNORED_LABELS)
    for k in extra_ignored_labels:
        ignored[k] = True
    ratios = NodeGroupDifferenceRatios() if ratios is None else ratios

    def comparator(n1, n2) -> bool:
        return is_cloud_provider_node_info_similar(n1, n2, ignored, ratios)
    return comparator


@dataclass(eq=False)
class NodeGroup:
    """The parts of cloudprovider.NodeGroup the balancing reads, for tests and non-Go callers
    (compared and hashed by identity, as Go's interface values holding pointers are)."""
    id: str
    target_size: int
    max_size: int
    min_size: int = 0

    def Id(self) -> str:  # noqa: N802 - reference spelling
        return self.id

    def TargetSize(self) -> int:  # noqa: N802
        return self.target_size

    def MaxSize(self) -> int:  # noqa: N802
        return self.max_size

    def MinSize(self) -> int:  # noqa: N802
        return self.min_size


@dataclass
class ScaleUpInfo:
    """nodegroupset.ScaleUpInfo (nodegroup_set_processor.go)."""
    group: object
    current_size: int
    new_size: int
    max_size: int

    Group = property(lambda self: self.group)
    CurrentSize = property(lambda self: self.current_size)
    NewSize = property(lambda self: self.new_size)
    MaxSize = property(lambda self: self.max_size)


class BalanceError(RuntimeError):
    """errors.AutoscalerError of the processor (InternalError)."""


@dataclass
class BalancingNodeGroupSetProcessor:
    """BalancingNodeGroupSetProcessor (balancing_processor.go:30-33)."""
    comparator: object = field(default_factory=create_generic_node_info_comparator)

    def FindSimilarNodeGroups(self, node_groups: list, node_group, node_infos: dict) -> list:  # noqa: N802
        """:37-68.  `node_groups` stands for context.CloudProvider.NodeGroups(): the result
        keeps its order."""
        gid = node_group.Id()
        if gid not in node_infos:
            raise BalanceError(f"failed to find template node for node group {gid}")
        info = node_infos[gid]
        result = []
        for ng in node_groups:
            if ng.Id() == gid or ng.Id() not in node_infos:
                continue
            if self.comparator is None:
                raise BalanceError("BalancingNodeGroupSetProcessor comparator not set")
            if self.comparator(info, node_infos[ng.Id()]):
                result.append(ng)
        return result

    def BalanceScaleUpBetweenGroups(self, groups: list, new_nodes: int) -> list:  # noqa: N802
        """:79-181: `new_nodes` spread over `groups`, smallest first, within MaxSize; the
        ScaleUpInfos of the groups whose size changed, in the loop's final order."""
        if len(groups) == 0:
            raise BalanceError("Can't balance scale up between 0 groups")
        infos = []
        total_capacity = 0
        for ng in groups:
            current, max_size = ng.TargetSize(), ng.MaxSize()
            if current == max_size:            # group already maxed, ignore it
                continue
            if max_size > current:
                total_capacity += max_size - current
            infos.append(ScaleUpInfo(ng, current, current, max_size))
        if total_capacity < new_nodes:
            new_nodes = total_capacity

        def swap(i, j):
            infos[i], infos[j] = infos[j], infos[i]

        gosort.sort_slice(len(infos), lambda i, j: infos[i].current_size < infos[j].current_size, swap)
        start = cur = 0
        while new_nodes > 0:
            # (currentInfo is a pointer to the slot: after the swap below it reads the group
            # that was swapped in)
            if infos[cur].new_size < infos[cur].max_size:
                infos[cur].new_size += 1
                new_nodes -= 1
            else:
                swap(start, cur)
                start += 1
            if cur < len(infos) - 1 and infos[cur].new_size > infos[cur + 1].new_size:
                cur += 1
            else:
                cur = start
        return [i for i in infos if i.new_size != i.current_size]


def filter_node_groups_by_pods(groups: list, pods_required: list, options: dict) -> list:
    """filterNodeGroupsByPods (orchestrator.go:596-628): the groups that have an option holding
    every required pod.  `options`: {node group id: ExpansionOption}; pods by identity."""
    result = []
    for group in groups:
        option = options.get(group.Id())
        if option is None:
            continue
        fitting = {id(p) for p in option.pods}
        if all(id(p) in fitting for p in pods_required):
            result.append(group)
    return result


def filter_plan_groups_by_pods(plan, required: int, groups) -> list:
    """The device form: `required` and `groups` are group indices of an Estimate plan whose last
    run left its lists in device memory (every group in `groups` has an option).  Returns the
    indices whose list holds every pod of `required`'s list, in input order.  `plan` is a
    native.EstimatePlan or a native.MultiEstimatePlan after a resident run (global indices; the
    required list is copied to another device only where a group of `groups` lies there)."""
    groups = [int(g) for g in groups]
    if not groups:
        return []
    n_missing, _ = plan.groups_missing_pods(int(required), groups)
    return [g for g, n in zip(groups, n_missing) if n == 0]
