"""Legacy scale-down bookkeeping around the removal sweep (CA/core/scaledown/legacy).

``ScaleDown.UpdateUnneededNodes`` (legacy.go:101-225) is the caller of the sweep in
every RunOnce (static_autoscaler.go:615 -> wrapper.go:50-52): per-node eligibility and
utilization (eligibility.go:66-176), the empty nodes (legacy.go:358-422 over
FindEmptyNodesToRemove), the candidate split (chooseCandidates :468-484),
FindNodesToRemove over the candidates and an additional pool (:146-176), and the
unneeded / unremovable node books (unneeded.go, unremovable/nodes.go:50-112).  The
policy parts are host code (O(nodes) bookkeeping); both sweeps and the
utilization pass run on the device through the facades.  Used to pin the path against
the reference's TestFindUnneededNodes (legacy_test.go:58-216).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Optional

from . import simulator as sim
from . import utilization
from .clustersnapshot import ClusterSnapshot
from .k8s import Node

ScaleDownDisabledKey = "cluster-autoscaler.kubernetes.io/scale-down-disabled"   # eligibility.go:38
ToBeDeletedTaint = "ToBeDeletedByClusterAutoscaler"                             # utils/taints/taints.go:38
MaxKubernetesEmptyNodeDeletionTime = 3 * 60.0                                    # delete_in_batch.go:42
MaxCloudProviderNodeDeletionTime = 5 * 60.0                                      # delete_in_batch.go:44


@dataclass
class NodeGroup:
    """The cloudprovider.NodeGroup fields scale-down reads."""
    id: str
    min_size: int
    max_size: int
    target_size: int


@dataclass
class ScaleDownOptions:
    """The config.AutoscalingOptions fields UpdateUnneededNodes reads."""
    scale_down_utilization_threshold: float = 0.5
    scale_down_gpu_utilization_threshold: float = 0.5
    unremovable_node_recheck_timeout: float = 5 * 60.0
    scale_down_non_empty_candidates_count: int = 30
    scale_down_candidates_pool_ratio: float = 0.1
    scale_down_candidates_pool_min_count: int = 50
    scale_down_unready_enabled: bool = False
    ignore_daemonsets_utilization: bool = False
    ignore_mirror_pods_utilization: bool = False


def to_be_deleted_time(node: Node) -> Optional[float]:
    """taints.GetToBeDeletedTime (taints.go:180-202): the taint value as unix seconds."""
    for t in node.taints:
        if t.key == ToBeDeletedTaint:
            try:
                return float(int(t.value))
            except ValueError:
                return None
    return None


def is_node_being_deleted(node: Node, timestamp: float) -> bool:
    """actuation.IsNodeBeingDeleted (delete_in_batch.go:179-182)."""
    t = to_be_deleted_time(node)
    return t is not None and (timestamp - t < MaxCloudProviderNodeDeletionTime
                              or timestamp - t < MaxKubernetesEmptyNodeDeletionTime)


class UnremovableNodes:
    """unremovable.Nodes (unremovable/nodes.go:30-112): reasons of this loop, TTLs across loops."""

    def __init__(self):
        self.reasons: dict = {}
        self.ttls: dict = {}

    def Update(self, snapshot: ClusterSnapshot, timestamp: float) -> None:  # noqa: N802
        self.reasons = {}
        names = set(snapshot.node_names())
        self.ttls = {n: ttl for n, ttl in self.ttls.items() if n in names and ttl > timestamp}

    def Add(self, u: sim.UnremovableNode) -> None:  # noqa: N802
        self.reasons[u.node.name] = u

    def AddTimeout(self, u: sim.UnremovableNode, timeout: float) -> None:  # noqa: N802
        self.ttls[u.node.name] = timeout
        self.Add(u)

    def AddReason(self, node: Node, reason: int) -> None:  # noqa: N802
        self.Add(sim.UnremovableNode(node, reason))

    def AsList(self) -> list:  # noqa: N802
        return list(self.reasons.values())

    def HasReason(self, name: str) -> bool:  # noqa: N802
        return name in self.reasons

    def IsRecent(self, name: str) -> bool:  # noqa: N802
        return name in self.ttls


class UnneededNodes:
    """unneeded.Nodes (core/scaledown/unneeded/nodes.go): the current set with since-times."""

    def __init__(self):
        self.since: dict = {}

    def Update(self, to_remove: list, timestamp: float) -> None:  # noqa: N802
        self.since = {t.node.name: self.since.get(t.node.name, timestamp) for t in to_remove}

    def Contains(self, name: str) -> bool:  # noqa: N802
        return name in self.since

    def AsList(self) -> list:  # noqa: N802
        return list(self.since)


class ScaleDown:
    """legacy.ScaleDown (legacy.go:56-99) restricted to UpdateUnneededNodes."""

    def __init__(self, snapshot: ClusterSnapshot, removal_simulator: sim.RemovalSimulator, node_groups: dict,
                 options: ScaleDownOptions, gpu_configs: Optional[dict] = None,
                 calculate_all: Optional[Callable] = None, device_candidates: bool = False,
                 resident_rows: bool = False):
        if resident_rows and not device_candidates:
            raise ValueError("resident_rows=True needs device_candidates=True")
        if device_candidates:
            from .native import Mirror
            if not isinstance(snapshot.backend, Mirror):
                raise TypeError("device_candidates=True needs the device mirror as the snapshot's backend")
        self.device_candidates = device_candidates
        self.device_updates = 0                        # UpdateUnneededNodes calls served by the candidates handle
        # resident_rows: the pod rows stay on the mirror (Mirror.set_pod_util_rows); each loop sends
        # the new and changed ones and clears those that went away
        self.resident_rows = resident_rows
        self._row_ids: set = set()                     # mirror pod ids that hold a row of ours ...
        self._row_clears = None                        # ... on the mirror as of this snapshot.backend_clears
        self.snapshot = snapshot
        self.removal_simulator = removal_simulator
        self.node_groups = node_groups                 # node name -> NodeGroup (NodeGroupForNode)
        self.options = options
        self.gpu_configs = gpu_configs or {}           # node name -> utilization.GpuConfig
        self.calculate_all = calculate_all or utilization.CalculateAll
        self.unneeded_nodes = UnneededNodes()
        self.unremovable_nodes = UnremovableNodes()
        self.node_utilization_map: dict = {}

    # eligibility.FilterOutUnremovable (eligibility.go:66-103)
    def _filter_out_unremovable(self, candidates: list, timestamp: float):
        ineligible, util_map, unneeded = [], {}, []
        names = set(self.snapshot.node_names())
        resolved = [n for n in candidates if n.name in names]
        infos = {n.name: self.snapshot.Get(n.name) for n in resolved}
        todo = [n for n in resolved if not self.unremovable_nodes.IsRecent(n.name)
                and not is_node_being_deleted(n, timestamp) and n.annotations.get(ScaleDownDisabledKey) != "true"]
        calc = dict(zip([n.name for n in todo],
                        self.calculate_all([infos[n.name] for n in todo], self.options.ignore_daemonsets_utilization,
                                           self.options.ignore_mirror_pods_utilization,
                                           [self.gpu_configs.get(n.name) for n in todo], timestamp))) if todo else {}
        for node in candidates:
            if node.name not in names:
                ineligible.append(sim.UnremovableNode(node, sim.UnexpectedError))
                continue
            if self.unremovable_nodes.IsRecent(node.name):
                ineligible.append(sim.UnremovableNode(node, sim.RecentlyUnremovable))
                continue
            reason, info = self._reason_and_utilization(node, calc.get(node.name), timestamp)
            if info is not None:
                util_map[node.name] = info
            if reason != sim.NoReason:
                ineligible.append(sim.UnremovableNode(node, reason))
                continue
            unneeded.append(node.name)
        return unneeded, util_map, ineligible

    # unremovableReasonAndNodeUtilization (eligibility.go:105-156)
    def _reason_and_utilization(self, node: Node, calc, timestamp: float):
        if is_node_being_deleted(node, timestamp):
            return sim.CurrentlyBeingDeleted, None
        if node.annotations.get(ScaleDownDisabledKey) == "true":
            return sim.ScaleDownDisabledAnnotation, None
        info, _err = calc                                  # an error only logs (:125-128)
        ng = self.node_groups.get(node.name)
        if ng is None:
            return sim.NotAutoscaled, None
        if not self.options.scale_down_unready_enabled and not node.ready:
            return sim.ScaleDownUnreadyDisabled, None
        gpu = self.gpu_configs.get(node.name) is not None
        threshold = (self.options.scale_down_gpu_utilization_threshold if gpu
                     else self.options.scale_down_utilization_threshold)
        if info.Utilization >= threshold:                  # isNodeBelowUtilizationThreshold (:158-178)
            return sim.NotUnderutilized, info
        return sim.NoReason, info

    # getEmptyNodesToRemove (legacy.go:364-422) without resource limits
    def _empty_nodes_to_remove(self, candidates: list, timestamp: float) -> list:
        return self._empty_within_limits(self.removal_simulator.FindEmptyNodesToRemove(candidates, timestamp))

    def _empty_within_limits(self, empty: list) -> list:
        available: dict = {}
        out = []
        for name in empty:
            ng = self.node_groups.get(name)
            if ng is None:
                continue
            if ng.id not in available:
                available[ng.id] = max(ng.target_size - ng.min_size, 0)
            if available[ng.id] > 0:
                available[ng.id] -= 1
                out.append(sim.NodeToBeRemoved(self.snapshot.Get(name).node, []))
        return out

    def _choose_candidates(self, nodes: list):
        """chooseCandidates (legacy.go:468-484)."""
        if self.options.scale_down_non_empty_candidates_count <= 0:
            return nodes, []
        cand = [n for n in nodes if self.unneeded_nodes.Contains(n)]
        non = [n for n in nodes if not self.unneeded_nodes.Contains(n)]
        return cand, non

    def _host_reason(self, node: Node, names: set, timestamp: float) -> int:
        """The checks of FilterOutUnremovable that need no utilization, in its order
        (eligibility.go:66-147); NoReason: the node goes on to the threshold check."""
        if node.name not in names:
            return sim.UnexpectedError
        if self.unremovable_nodes.IsRecent(node.name):
            return sim.RecentlyUnremovable
        if is_node_being_deleted(node, timestamp):
            return sim.CurrentlyBeingDeleted
        if node.annotations.get(ScaleDownDisabledKey) == "true":
            return sim.ScaleDownDisabledAnnotation
        if self.node_groups.get(node.name) is None:
            return sim.NotAutoscaled
        if not self.options.scale_down_unready_enabled and not node.ready:
            return sim.ScaleDownUnreadyDisabled
        return sim.NoReason

    def _device_inputs(self, dest: list, scale_down_candidates: list, timestamp: float):
        """FilterOutUnremovable, the empty nodes and the sweeps' inputs from one
        native.ScaleDownCandidates on the snapshot's mirror: the host's eligibility checks go in
        as the `eligible` mask, its GetPodsToMove verdicts as pod override rows.  Returns
        (unneeded, util_map, ineligible, empty, sweep), `sweep(names)` standing in for
        FindNodesToRemove, or None when a host verdict has no form in the handle (a drain error
        without a blocking pod, a utilization error, a candidate that is no destination, an empty
        node beyond its group's limits): the caller then takes the host path.  Changes nothing
        before it returns, except that with resident_rows the loop's pod rows are on the mirror
        by then (also when it returns None after the handle was made: the host path reads none
        of them, and the next loop sends what differs)."""
        import numpy as np
        from . import abi
        from .drain import get_pods_to_move
        snap, rs, opt = self.snapshot, self.removal_simulator, self.options
        names = snap.node_names()
        in_snap, dest_set = set(names), set(dest)
        reasons = {n.name: self._host_reason(n, in_snap, timestamp) for n in scale_down_candidates}
        eligible = np.zeros(len(names), np.uint8)
        verdicts, flag = {}, {}
        for name, reason in reasons.items():
            if reason != sim.NoReason:
                continue
            if name not in dest_set:
                return None
            eligible[snap.position(name)] = 1
            v = get_pods_to_move(snap.Get(name).pods, rs.delete_options, rs.listers, [], timestamp)
            if v[3] is not None and v[2] is None:
                return None
            verdicts[name] = v
            if v[3] is None:
                flag.update((id(p), abi.CA_UPOD_MOVABLE) for p in v[0])
            else:
                flag[id(v[2].pod)] = abi.CA_UPOD_BLOCKING
        node_over, pod_over = utilization.snapshot_overrides(snap, list(verdicts), self.gpu_configs,
                                                             pod_flags=lambda p: flag.get(id(p), 0))
        if self.resident_rows:
            self._send_changed_rows(pod_over)
            pod_over = None
        sd = snap.backend.scale_down_candidates(
            opt.ignore_daemonsets_utilization, opt.ignore_mirror_pods_utilization, round(timestamp * 1e9),
            opt.scale_down_utilization_threshold, opt.scale_down_gpu_utilization_threshold, eligible, node_over, pod_over,
            resident=self.resident_rows)
        ls = sd.fetch()
        if (ls.node_class == abi.CA_SD_UTIL_ERROR).any():
            sd.close()
            return None
        unneeded, util_map, ineligible, empty = [], {}, [], []
        for node in scale_down_candidates:
            if reasons[node.name] != sim.NoReason:
                ineligible.append(sim.UnremovableNode(node, reasons[node.name]))
                continue
            pos = snap.position(node.name)
            util_map[node.name] = utilization.info_from_row(ls.info[pos], node.name, self.gpu_configs.get(node.name))[0]
            if ls.node_class[pos] == abi.CA_SD_NOT_BELOW:
                ineligible.append(sim.UnremovableNode(node, sim.NotUnderutilized))
                continue
            unneeded.append(node.name)
            if ls.node_class[pos] == abi.CA_SD_EMPTY:
                empty.append(node.name)
        within = self._empty_within_limits(empty)
        if len(within) != len(empty):
            sd.close()
            return None
        mask = np.array([n in dest_set for n in names], np.uint8)

        def sweep(cands: list):
            if not cands:
                return [], []
            with sd.removal_plan(nodes=[snap.position(n) for n in cands], dest_mask=mask) as plan:
                return rs.FindNodesToRemovePlanned(plan, cands, verdicts)
        sweep.close = sd.close
        return unneeded, util_map, ineligible, within, sweep

    def _send_changed_rows(self, pod_over) -> None:
        """This loop's pod rows as resident rows: only what differs from what the mirror holds.
        What it holds is read from the mirror's own host copy (Mirror.pod_util_rows), not
        remembered here: a replay or a Clear of the snapshot clears the backend, the rows go with
        it, and the same pod ids come back without them.  Only the ids to clear are remembered,
        and forgotten when snapshot.backend_clears says the mirror started over."""
        import numpy as np
        from . import abi
        snap, m = self.snapshot, self.snapshot.backend
        if self._row_clears != snap.backend_clears:
            self._row_ids, self._row_clears = set(), snap.backend_clears
        if pod_over is None:
            ids, rows = np.zeros(0, np.int32), np.zeros(0, abi.UTIL_POD_DTYPE)
        else:
            ids = np.ascontiguousarray(pod_over[0], dtype=np.int32)
            rows = np.ascontiguousarray(pod_over[1], dtype=abi.UTIL_POD_DTYPE)
        held, has = m.pod_util_rows(ids)
        width = abi.UTIL_POD_DTYPE.itemsize
        same = (held.view(np.uint8).reshape(-1, width) == rows.view(np.uint8).reshape(-1, width)).all(axis=1)
        changed = np.nonzero((has == 0) | ~same)[0]
        now = set(ids.tolist())
        gone = sorted(self._row_ids - now)
        if changed.size:
            m.set_pod_util_rows(ids[changed], rows[changed])
        if gone:
            m.set_pod_util_rows(np.array(gone, np.int32), None)
        self._row_ids = now

    def UpdateUnneededNodes(self, destination_nodes: list, scale_down_candidates: list,  # noqa: N802
                            timestamp: float) -> None:
        """legacy.go:101-225."""
        all_nodes = self.snapshot.node_names()
        self.unremovable_nodes.Update(self.snapshot, timestamp)
        dest = [n.name for n in destination_nodes]
        dev = self._device_inputs(dest, scale_down_candidates, timestamp) if self.device_candidates else None
        if dev is not None:
            unneeded, util_map, ineligible, empty, sweep = dev
            self.device_updates += 1
        else:
            unneeded, util_map, ineligible = self._filter_out_unremovable(scale_down_candidates, timestamp)
            empty = self._empty_nodes_to_remove(unneeded, timestamp)
            sweep = lambda names: self.removal_simulator.FindNodesToRemove(names, dest, timestamp, [])  # noqa: E731
        for u in ineligible:
            self.unremovable_nodes.Add(u)
        empty_names = {e.node.name for e in empty}
        non_empty = [n for n in unneeded if n not in empty_names]
        cand, non = self._choose_candidates(non_empty)
        to_remove, unremovable = sweep(cand)
        extra = self.options.scale_down_non_empty_candidates_count - len(to_remove)
        extra = min(extra, len(non))
        pool = int(math.ceil(len(all_nodes) * self.options.scale_down_candidates_pool_ratio))
        pool = min(max(pool, self.options.scale_down_candidates_pool_min_count), len(non))
        if extra > 0:
            more, more_un = sweep(non[:pool])
            to_remove += more[:extra]
            unremovable += more_un
        if dev is not None:
            sweep.close()
        to_remove += empty
        self.unneeded_nodes.Update(to_remove, timestamp)
        if unremovable:
            timeout = timestamp + self.options.unremovable_node_recheck_timeout
            for u in unremovable:
                self.unremovable_nodes.AddTimeout(u, timeout)
        for node in scale_down_candidates:
            if not self.unneeded_nodes.Contains(node.name) and not self.unremovable_nodes.HasReason(node.name):
                self.unremovable_nodes.AddReason(node, sim.NotUnneededOtherReason)
        self.removal_simulator.DropOldHints()
        self.node_utilization_map = util_map
