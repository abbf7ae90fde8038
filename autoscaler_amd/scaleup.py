"""ScaleUp's option computation for every node group in one pass (CA/core/scaleup).

The reference computes, per node group (orchestrator.go:139-178 -> ComputeExpansionOption
:443-491): Fork; add the template node with its pods; CheckPredicates(sample pod of
every pod equivalence group, template node); Revert; then Estimate(pods of the
groups that passed, template).  Here:

* ``BuildPodGroups`` (equivalence/groups.go:38-102) stays on the host: pods grouped by
  controller UID + equal labels and spec, at most 10 groups per controller, pods
  without a controller (or DaemonSet pods) alone;
* the feasibility of every (node group, pod group) pair is one device call
  (``ca_check_templates``: CheckPredicates of the sample on a fresh template copy,
  schedulerbased.go:139-185 results, reasons included for eg.SchedulingErrors);
* the options' Estimates are one batch (``estimate_batch``: shared lastIndex, exactly
  as the reference's consecutive Estimate calls).

Order: the reference ranges over BuildPodGroups' map (random order in Go); groups
here are in first-occurrence order, so an option's pods are in a canonical order
(Estimate's tie order).

The grouping can also be built on the device: ``BuildPodGroupsOnDevice`` returns the same
groups from the interned records (``ca_pod_groups_create``) and carries the resident handle,
which ``ComputeBestExpansionOption`` and ``ComputeBalancedScaleUp`` read in place.
"""
from __future__ import annotations

from contextlib import contextmanager
from dataclasses import dataclass, field

import numpy as np

from . import abi
from .clustersnapshot import ClusterSnapshot, NodeInfo
from .estimator import ThresholdBasedEstimationLimiter, estimate_batch
from .k8s import Pod, is_daemonset_pod
from .predicatechecker import SchedulerBasedPredicateChecker
from .simulator import SimilarPodsScheduling

MAX_EQUIVALENCE_GROUPS_BY_CONTROLLER = 10          # groups.go:57


@dataclass
class PodGroup:
    """equivalence.PodGroup (groups.go:30-35)."""
    pods: list
    scheduling_errors: dict = field(default_factory=dict)     # node group id -> ca_pred_result
    schedulable: bool = False


def BuildPodGroups(pods: list) -> list:  # noqa: N802
    """groupPodsBySchedulingProperties (groups.go:59-102), groups in first-occurrence order."""
    groups: list[PodGroup] = []
    by_controller: dict = {}
    for pod in pods:
        ref = pod.controller_ref()
        if ref is None or is_daemonset_pod(pod):                  # :68-72 (pod_util.IsDaemonSetPod)
            groups.append(PodGroup([pod]))
            continue
        egs = by_controller.setdefault(ref.uid, [])
        sig = SimilarPodsScheduling._sig(pod)                      # labels + spec equality (:105-112)
        gid = next((g for s, g in egs if s == sig), None)
        if gid is not None:
            groups[gid].pods.append(pod)
            continue
        if len(egs) < MAX_EQUIVALENCE_GROUPS_BY_CONTROLLER:       # :79-86
            egs.append((sig, len(groups)))
        groups.append(PodGroup([pod]))
    return groups


class DevicePodGroups(list):
    """BuildPodGroupsOnDevice's result: the list[PodGroup] of BuildPodGroups(pods), plus the
    groups where they were built: `pods` (the input, whose positions are the pod-set indices),
    `table` / `podset` (their records, resident on the snapshot's backend) and `handle` (the
    native.PodGroups over them).  close() frees the device side; the list stays usable."""

    pods: list
    table = None
    podset = None
    handle = None

    def _build(self, snapshot: ClusterSnapshot, table) -> None:
        self.close()
        self.table = table
        self.podset = snapshot.backend.podset(table)
        cls = table.pods["similar_class"]
        n_classes = int(cls.max()) + 1 if len(cls) else 0
        self.handle = snapshot.backend.build_pod_groups(
            self.podset, class_owner=snapshot.interner.class_owners(max(n_classes, 0)))

    def resident(self, snapshot: ClusterSnapshot, table):
        """(podset, handle) for `table`, the current encoding of `pods`: rebuilt when the
        interner's universes grew since the build and the records changed."""
        same = self.handle is not None and all(
            getattr(self.table, k).tobytes() == getattr(table, k).tobytes() for k in ("pods", "terms", "reqs", "names"))
        if not same:
            self._build(snapshot, table)
        return self.podset, self.handle

    def close(self) -> None:
        if self.handle is not None:
            self.handle.close()
            self.handle = None
        if self.podset is not None:
            self.podset.close()
            self.podset = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def BuildPodGroupsOnDevice(snapshot: ClusterSnapshot, pods: list) -> DevicePodGroups:  # noqa: N802
    """BuildPodGroups(pods) computed on the snapshot's device mirror from the interned records
    (similar class, DaemonSet flag, the classes' controllers; ca_pod_groups_create): the same
    groups with the same pods in the same order.  The returned list carries the resident handle
    (DevicePodGroups); close() it, or use it as a context manager."""
    _backend_must_be_mirror(snapshot, "BuildPodGroupsOnDevice")
    pods = list(pods)
    snapshot.ensure(pods=pods)
    out = DevicePodGroups()
    out.pods = pods
    out._build(snapshot, snapshot.interner.encode_pods(pods))
    eg_off, eg_pod = out.handle.fetch()
    for e in range(out.handle.n_groups):
        out.append(PodGroup([pods[i] for i in eg_pod[eg_off[e]:eg_off[e + 1]]]))
    return out


def _device_groups(pod_groups, option_lists: str):
    """The DevicePodGroups whose handle the facades read: given as the pod groups, with the
    lists built on the device."""
    return pod_groups if isinstance(pod_groups, DevicePodGroups) and option_lists == "device" else None


@dataclass
class ExpansionOption:
    """expander.Option (the parts the Estimate fills): node group, count, pods."""
    node_group: object
    node_count: int
    pods: list


def _feasible_pods(snapshot: ClusterSnapshot, pod_groups: list, node_groups: list):
    """The feasibility matrix of ComputeExpansionOption (orchestrator.go:455-481) in one device
    call; marks the pod groups.  Returns ([(pods, template NodeInfo)] of the node groups that
    got pods, their indices in `node_groups`, the matrix)."""
    samples = [g.pods[0] for g in pod_groups]
    templates_api = [(t.node, list(t.pods)) for _, t in node_groups]
    snapshot.ensure(pods=[p for g in pod_groups for p in g.pods], templates=templates_api)
    table = snapshot.interner.encode_pods(samples)
    tm = np.zeros(len(node_groups), abi.TEMPLATE_DTYPE)
    for k, (node, tpods) in enumerate(templates_api):
        tm[k] = snapshot.interner.encode_template(node, tpods)
    feas = snapshot.backend.check_templates(table, np.arange(len(samples), dtype=np.int32), tm)
    est_groups, est_index = [], []
    for k, (ng, info) in enumerate(node_groups):
        pods = []
        for e, pg in enumerate(pod_groups):
            r = feas[k, e]
            if int(r["type"]) == abi.CA_PRED_OK:
                pods.extend(pg.pods)
                pg.schedulable = True
            else:
                pg.scheduling_errors[ng] = r.copy()
        if pods:
            est_groups.append((pods, info))
            est_index.append(k)
    return est_groups, est_index, feas


def ComputeExpansionOptions(snapshot: ClusterSnapshot, checker: SchedulerBasedPredicateChecker,  # noqa: N802
                            pod_groups: list, node_groups: list, limiter: ThresholdBasedEstimationLimiter):
    """ComputeExpansionOption (orchestrator.go:443-491) for every (node group, template
    NodeInfo) in ``node_groups``: pod groups' feasibility in one device call, then one
    Estimate batch over the options that got pods.  Marks pod groups schedulable and
    records their per-node-group predicate results, as the reference does."""
    est_groups, est_index, feas = _feasible_pods(snapshot, pod_groups, node_groups)
    options = [ExpansionOption(ng, 0, []) for ng, _ in node_groups]
    if est_groups:
        counts, scheduled = estimate_batch(checker, snapshot, est_groups, limiter)
        for k, c, s in zip(est_index, counts, scheduled):
            options[k].node_count = c
            options[k].pods = s
    return options, feas


@contextmanager
def _resident_estimate(snapshot: ClusterSnapshot, checker: SchedulerBasedPredicateChecker,
                       limiter: ThresholdBasedEstimationLimiter, node_groups: list, est_groups: list,
                       est_index: list, all_pods: list, pod_idx, offs, multi, options=None, device_groups=None):
    """What ComputeBestExpansionOption and ComputeBalancedScaleUp share after the feasibility
    matrix: the Estimate plan over `all_pods` (group g's pods are pod_idx[offs[g]:offs[g + 1]]),
    one run with the lists left in device memory, the checker's counters, the :174 filter and the
    device form of the options.  The plan is an EstimatePlan on the snapshot's backend, or, with
    `multi` (a native.Multi), a MultiEstimatePlan over its mirrors, each of which is first made to
    hold the snapshot (ClusterSnapshot.sync_replica).  Yields (plan, run output, valid group
    indices, DeviceOptions, node infos by node group id); the plan is closed on exit.  With
    `options` = (eg_off, eg_pod, ok) (see _option_inputs) the plan builds the lists itself
    (native.EstimatePlan.from_options) and pod_idx / offs are not read.  With `device_groups` (a
    DevicePodGroups; all_pods is then its pods in input order and options[2] the matrix over all
    of its groups) the plan reads the groups from the handle (native.EstimatePlan.from_groups).
    With `multi` both forms build the sharded plan's counterpart (MultiEstimatePlan.from_options /
    .from_groups, the handle resident on the snapshot's backend): every block builds its own lists."""
    from . import native
    from .expander import DeviceOptions, resources_for_node
    from .predicatechecker import unsupported
    from .scope import UnsupportedByKernels, out_of_scope_reason

    table = snapshot.interner.encode_pods(all_pods)
    templates = np.zeros(len(est_groups), abi.TEMPLATE_DTYPE)
    for g, (_, info) in enumerate(est_groups):
        templates[g] = snapshot.interner.encode_template(info.node, list(info.pods))
    caps = [resources_for_node(info.node) for _, info in est_groups]
    with unsupported("Estimate: the snapshot holds a pod with required anti-affinity"):
        if multi is not None:
            for m in multi.mirrors:            # (after _feasible_pods, which may have re-interned and replayed)
                snapshot.sync_replica(m)
        if device_groups is not None:
            ps, handle = device_groups.resident(snapshot, table)
            if multi is None:
                plan = native.EstimatePlan.from_groups(snapshot.backend, ps, handle, options[2], templates)
            else:
                plan = native.MultiEstimatePlan.from_groups(multi, table, handle, options[2], templates)
        elif options is not None:
            if multi is None:
                plan = native.EstimatePlan.from_options(snapshot.backend, table, *options, templates)
            else:
                plan = native.MultiEstimatePlan.from_options(multi, table, *options, templates)
        elif multi is None:
            plan = native.EstimatePlan(snapshot.backend, table, np.array(offs, np.int32),
                                       np.array(pod_idx, np.int32), templates)
        else:
            plan = native.MultiEstimatePlan(multi, table, np.array(offs, np.int32), np.array(pod_idx, np.int32),
                                            templates)
    node_infos = {(ng.Id() if hasattr(ng, "Id") else ng): info for ng, info in node_groups}
    with plan:
        with unsupported("Estimate: the snapshot holds a pod with required anti-affinity"):
            out = plan.run(limiter.max_nodes, checker.last_index, device_results=True)
        for g, r in enumerate(out.results):
            if int(r["status"]) == abi.CA_EUNSUPPORTED:
                why = next((out_of_scope_reason(p) for p in est_groups[g][0] if out_of_scope_reason(p)), None)
                raise UnsupportedByKernels(f"node group {g}: " + (why or "pods depend on node identity (hostname / "
                                                                          "nodeName) or template pods need InterPodAffinity"))
            checker.evals += int(r["evals"])
        checker.last_index = out.last_index
        valid = [g for g, r in enumerate(out.results) if int(r["n_scheduled"]) > 0 and int(r["node_count"]) > 0]
        dev = DeviceOptions(plan, out.results, [c for c, _ in caps], [m for _, m in caps], pods=all_pods,
                            node_groups=[node_groups[k][0] for k in est_index], node_infos=node_infos)
        yield plan, out, valid, dev, node_infos


# "device": at C2 the option-form constructor's median (0.378 ms) lies below the host-list
# constructor's lower quartile (0.710 ms), DESIGN.md §5 "Cold latency" / profiles/option_lists_cold.txt
OPTION_LISTS_DEFAULT = "device"


def _option_inputs(pod_groups: list, est_index: list, feas):
    """The device form of the options' lists (native.EstimatePlan.from_options): the shared pod
    table holds every pod of a pod group that passes anywhere once, group after group (so a pod
    has one id in every option); the pod groups are its CSR; `ok` is the feasibility matrix of
    the node groups that got pods over those pod groups.  Returns (all_pods, (eg_off, eg_pod, ok))."""
    ok = (feas["type"] == abi.CA_PRED_OK)[np.asarray(est_index, np.int64)]
    passing = np.nonzero(ok.any(axis=0))[0]
    all_pods, eg_off = [], [0]
    for e in passing:
        all_pods.extend(pod_groups[e].pods)
        eg_off.append(len(all_pods))
    ok = np.ascontiguousarray(ok[:, passing], np.uint8)
    return all_pods, (np.array(eg_off, np.int32), np.arange(len(all_pods), dtype=np.int32), ok)


def _handle_inputs(dpg: DevicePodGroups, est_index: list, feas):
    """_option_inputs for pod groups built on the device: the pod table is the given pods in
    input order (the handle's indices), the CSR stays in the handle, and `ok` covers every pod
    group: a group that passes nowhere is an all-zero column.  Returns (all_pods, (None, None, ok))."""
    ok = (feas["type"] == abi.CA_PRED_OK)[np.asarray(est_index, np.int64)]
    return dpg.pods, (None, None, np.ascontiguousarray(ok, np.uint8))


def _check_option_lists(option_lists, multi=None) -> str:
    """`option_lists` with its default filled in: OPTION_LISTS_DEFAULT on one mirror, "host" with
    `multi` (the sharded default waits for a measurement on several physical devices)."""
    if option_lists is None:
        option_lists = OPTION_LISTS_DEFAULT if multi is None else "host"
    if option_lists not in ("device", "host"):
        raise ValueError('option_lists: "device" or "host"')
    return option_lists


def _backend_must_be_mirror(snapshot: ClusterSnapshot, who: str) -> None:
    from . import native
    if not isinstance(snapshot.backend, native.Mirror):
        raise TypeError(f"{who} reads the Estimate plan's device-resident lists: "
                        "the snapshot's backend must be native.Mirror")


def ComputeBestExpansionOption(snapshot: ClusterSnapshot, checker: SchedulerBasedPredicateChecker,  # noqa: N802
                               pod_groups: list, node_groups: list, limiter: ThresholdBasedEstimationLimiter,
                               strategy, multi=None, option_lists=None):
    """ComputeExpansionOptions followed by the orchestrator's option filter and
    ExpanderStrategy.BestOption (orchestrator.go:139-195), with the options' pod lists left
    in device memory: one Estimate plan run with device results, the `len(Pods) > 0 &&
    NodeCount > 0` filter (:174) on its counts, `strategy` (an expander.ChainStrategy) on
    the device form of its filters, and one copy of the pod list of each option that is left
    (one option unless the chain fell through to the fallback).  Returns (the best
    ExpansionOption or None, the feasibility matrix); the snapshot's backend must be the
    device mirror.  `multi` (a native.Multi): the Estimate plan is sharded over its mirrors,
    which are synced to the snapshot first; the feasibility matrix still runs on the backend and
    everything after the run is the same code.  `option_lists`: "host" appends the options' pod
    lists here and uploads them; "device" encodes every pod of a passing pod group once and
    hands the pod groups and the feasibility matrix to the plan, which builds the lists in
    device memory (same results); with `multi` every block builds the lists of its own node
    groups on its own device.  None: "device" on one mirror, "host" with `multi`."""
    _backend_must_be_mirror(snapshot, "ComputeBestExpansionOption")
    option_lists = _check_option_lists(option_lists, multi)
    est_groups, est_index, feas = _feasible_pods(snapshot, pod_groups, node_groups)
    if not est_groups:
        return None, feas
    all_pods, offs, options = [], [0], None
    dpg = _device_groups(pod_groups, option_lists)
    if dpg is not None:
        all_pods, options = _handle_inputs(dpg, est_index, feas)
    elif option_lists == "device":
        all_pods, options = _option_inputs(pod_groups, est_index, feas)
    else:
        for pods, _ in est_groups:
            all_pods.extend(pods)
            offs.append(len(all_pods))
    with _resident_estimate(snapshot, checker, limiter, node_groups, est_groups, est_index, all_pods,
                            np.arange(len(all_pods), dtype=np.int32), offs, multi,
                            options, dpg) as (plan, out, valid, dev, node_infos):
        if not valid:                      # "No expansion options" (orchestrator.go:181-188)
            return None, feas
        options = []
        for g in strategy.best_indices(dev, valid):
            ng = node_groups[est_index[g]][0]
            pods = [all_pods[i] for i in plan.fetch_group(int(g))]
            options.append(ExpansionOption(ng, int(out.results[g]["node_count"]), pods))
    if len(options) == 1:
        return options[0], feas
    return strategy.fallback.BestOption(options, node_infos), feas


def ComputeBalancedScaleUp(snapshot: ClusterSnapshot, checker: SchedulerBasedPredicateChecker,  # noqa: N802
                           pod_groups: list, node_groups: list, limiter: ThresholdBasedEstimationLimiter,
                           strategy, processor, cap_new_nodes=None, multi=None, option_lists=None):
    """ScaleUp from the options to the final scale-up plan (orchestrator.go:139-313) with
    --balance-similar-node-groups, the options' pod lists left in device memory: the
    feasibility matrix; ONE Estimate plan over a shared pod table (every pending pod encoded
    once, each group's pod_idx slice naming its feasible pods in that table, so a pod has one
    id in every group); a run with device results; the :174 filter; `strategy` on the device
    form of its filters (its fallback gets the fetched survivors); `cap_new_nodes(node_count)`
    if given (the caller's GetCappedNewNodeCount / ApplyLimits; IsNodeGroupSafeToScaleUp stays
    with the caller too); `processor.FindSimilarNodeGroups`; the similar groups that have an
    option and whose option holds every pod of the winner's (filterNodeGroupsByPods :596-628,
    on the device: nodegroupset.filter_plan_groups_by_pods);
    `processor.BalanceScaleUpBetweenGroups([best] + kept, new_nodes)`; one copy of the winner's
    list.  The node groups are objects with Id() / TargetSize() / MaxSize().  Returns (the best
    ExpansionOption or None, [ScaleUpInfo], the feasibility matrix).  `multi`: as on
    ComputeBestExpansionOption; the winner's list then crosses devices only if a similar group's
    option lies in another block (casim.h, ca_multi_estimate_plan_groups_missing_pods).
    `option_lists`: as on ComputeBestExpansionOption ("device": the pod_idx slices are built in
    device memory from the pod groups and the feasibility matrix)."""
    from .nodegroupset import filter_plan_groups_by_pods

    _backend_must_be_mirror(snapshot, "ComputeBalancedScaleUp")
    option_lists = _check_option_lists(option_lists, multi)
    est_groups, est_index, feas = _feasible_pods(snapshot, pod_groups, node_groups)
    if not est_groups:
        return None, [], feas
    all_pods, row = [], {}
    pod_idx, offs, options = [], [0], None
    dpg = _device_groups(pod_groups, option_lists)
    if dpg is not None:
        all_pods, options = _handle_inputs(dpg, est_index, feas)
    elif option_lists == "device":
        all_pods, options = _option_inputs(pod_groups, est_index, feas)
    else:
        for pods, _ in est_groups:                  # the shared table: every feasible pod once
            for p in pods:
                if id(p) not in row:
                    row[id(p)] = len(all_pods)
                    all_pods.append(p)
                pod_idx.append(row[id(p)])
            offs.append(len(pod_idx))
    with _resident_estimate(snapshot, checker, limiter, node_groups, est_groups, est_index, all_pods, pod_idx, offs,
                            multi, options, dpg) as (plan, out, valid, dev, node_infos):
        if not valid:                      # "No expansion options" (orchestrator.go:181-188)
            return None, [], feas
        group_of = {node_groups[est_index[g]][0].Id(): g for g in valid}      # expansionOptions' keys

        def option(g):
            return ExpansionOption(node_groups[est_index[g]][0], int(out.results[g]["node_count"]),
                                   [all_pods[i] for i in plan.fetch_group(int(g))])

        left = [int(g) for g in strategy.best_indices(dev, valid)]
        best = option(left[0]) if len(left) == 1 else strategy.fallback.BestOption([option(g) for g in left], node_infos)
        if best is None or best.node_count <= 0:          # :196-202
            return None, [], feas
        best_g = group_of[best.node_group.Id()]
        new_nodes = best.node_count if cap_new_nodes is None else cap_new_nodes(best.node_count)
        similar = processor.FindSimilarNodeGroups([ng for ng, _ in node_groups], best.node_group, node_infos)
        with_option = [ng for ng in similar if ng.Id() in group_of]
        fit = set(filter_plan_groups_by_pods(plan, best_g, [group_of[ng.Id()] for ng in with_option]))
        kept = [ng for ng in with_option if group_of[ng.Id()] in fit]
    return best, processor.BalanceScaleUpBetweenGroups([best.node_group] + kept, new_nodes), feas


__all__ = ["PodGroup", "BuildPodGroups", "BuildPodGroupsOnDevice", "DevicePodGroups","ExpansionOption", "ComputeExpansionOptions", "ComputeBestExpansionOption",
           "ComputeBalancedScaleUp", "NodeInfo", "Pod"]
