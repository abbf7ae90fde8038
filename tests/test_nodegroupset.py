"""autoscaler_amd/nodegroupset.py (host code): the comparator and the balancing processor on
the reference's own test cases (tests/golden/nodegroupset_cases.json), the balancing loop
against an independent statement of its result on random groups, the host form of
filterNodeGroupsByPods, and TestScaleUpBalanceGroups' known answer through the host forms."""
import json
import os
import random

import pytest

from autoscaler_amd import gosort, k8s
from autoscaler_amd.clustersnapshot import NodeInfo
from autoscaler_amd.k8s import Quantity
from autoscaler_amd.nodegroupset import (BASIC_IGNORED_LABELS, BalanceError, BalancingNodeGroupSetProcessor, NodeGroup,
                                         NodeGroupDifferenceRatios, create_generic_node_info_comparator,
                                         filter_node_groups_by_pods, requested_resource_list)
from autoscaler_amd.scaleup import ExpansionOption

CASES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nodegroupset_cases.json")))


def _node(spec, labels=None):
    mem = spec["memory"]
    n = k8s.build_test_node(spec["name"], spec["cpu_milli"], Quantity(mem).value() if isinstance(mem, str) else mem)
    n.capacity = dict(n.allocatable)
    for res, q in spec.get("capacity", {}).items():
        n.capacity[res] = Quantity(q)
    for res, q in spec.get("allocatable", {}).items():
        n.allocatable[res] = Quantity(q)
    n.labels.update(spec.get("labels", {}))
    n.labels.update(labels or {})
    return n


def _pods(specs):
    return [k8s.build_test_pod(s["name"], s["cpu_milli"], s["memory"]) for s in specs]


def _groups(specs):
    return [NodeGroup(i, size, mx, mn) for i, mn, mx, size in specs]


def test_defaults():
    r = NodeGroupDifferenceRatios()
    assert (r.max_allocatable_difference_ratio, r.max_free_difference_ratio,
            r.max_capacity_memory_difference_ratio) == (0.05, 0.05, 0.015)
    assert len(BASIC_IGNORED_LABELS) == 7 and all(BASIC_IGNORED_LABELS.values())
    assert "topology.kubernetes.io/zone" in BASIC_IGNORED_LABELS and "kops.k8s.io/instancegroup" in BASIC_IGNORED_LABELS


@pytest.mark.parametrize("case", CASES["compare"], ids=[c["name"] for c in CASES["compare"]])
def test_comparator_golden(case):
    cmp = create_generic_node_info_comparator(case["extra_ignored"], NodeGroupDifferenceRatios())
    n1 = NodeInfo(_node(case["n1"]), _pods(case.get("pods1", [])))
    n2 = NodeInfo(_node(case["n2"]), _pods(case.get("pods2", [])))
    assert cmp(n1, n2) is case["similar"]
    assert cmp(n2, n1) is case["similar"]          # (every criterion is symmetric)


def test_requested_is_the_effective_request():
    """Requested: containers summed, max with the init containers, plus overhead; the list has
    cpu, memory, pods and ephemeral-storage even for an empty node."""
    p = k8s.build_test_pod("p", 300, 1000)
    p.init_containers.append(k8s.Container(requests={"cpu": Quantity.milli(1500)}))
    p.overhead = {"cpu": Quantity.milli(10), "memory": Quantity(5)}
    q = k8s.build_test_pod("q", 200, 100)
    rl = requested_resource_list(NodeInfo(k8s.build_test_node("n", 4000, 1 << 20), [p, q]))
    assert rl["cpu"].milli_value() == 1500 + 10 + 200 and rl["memory"].value() == 1000 + 5 + 100
    assert sorted(requested_resource_list(NodeInfo(k8s.build_test_node("n", 1, 1)))) == \
        ["cpu", "ephemeral-storage", "memory", "pods"]


@pytest.mark.parametrize("variant", CASES["find_similar"]["variants"], ids=lambda v: v["name"])
def test_find_similar_golden(variant):
    fs = CASES["find_similar"]
    groups = _groups(fs["groups"])
    infos = {g: NodeInfo(_node(spec, variant["labels"].get(g))) for g, spec in fs["nodes"].items()}
    if variant["comparator"] == "generic":
        proc = BalancingNodeGroupSetProcessor(create_generic_node_info_comparator(
            variant["extra_ignored"], NodeGroupDifferenceRatios(0.0, 0.0, 0.0)))
    else:
        names = set(variant["similar_names"])
        proc = BalancingNodeGroupSetProcessor(
            lambda a, b: a.Node().name != b.Node().name and {a.Node().name, b.Node().name} == names)
    for g in groups:
        assert [s.Id() for s in proc.FindSimilarNodeGroups(groups, g, infos)] == fs["expected"][g.Id()]
    with pytest.raises(BalanceError):
        proc.FindSimilarNodeGroups(groups, NodeGroup("unknown", 1, 2), infos)


def test_find_similar_keeps_the_callers_order_and_skips_groups_without_info():
    groups = [NodeGroup(f"g{i}", 1, 5) for i in range(6)]
    infos = {g.Id(): NodeInfo(k8s.build_test_node(g.Id(), 1000, 1000)) for g in groups if g.Id() != "g4"}
    proc = BalancingNodeGroupSetProcessor()
    assert [s.Id() for s in proc.FindSimilarNodeGroups(groups[::-1], groups[2], infos)] == ["g5", "g3", "g1", "g0"]


def literal_loop(groups, new_nodes):
    """The loop of balancing_processor.go:139-170 over records in gosort.sort_slice's order, on
    plain lists: [id, current, new, max]."""
    recs = [[g.Id(), g.TargetSize(), g.TargetSize(), g.MaxSize()] for g in groups if g.TargetSize() != g.MaxSize()]
    new_nodes = min(new_nodes, sum(max(0, r[3] - r[1]) for r in recs))

    def swap(i, j):
        recs[i], recs[j] = recs[j], recs[i]

    gosort.sort_slice(len(recs), lambda i, j: recs[i][1] < recs[j][1], swap)
    start = cur = 0
    while new_nodes > 0:
        if recs[cur][2] < recs[cur][3]:
            recs[cur][2] += 1
            new_nodes -= 1
        else:
            swap(start, cur)
            start += 1
        if cur < len(recs) - 1 and recs[cur][2] > recs[cur + 1][2]:
            cur += 1
        else:
            cur = start
    return [(r[0], r[1], r[2], r[3]) for r in recs if r[2] != r[1]]


def _tuples(infos):
    return [(i.Group.Id(), i.CurrentSize, i.NewSize, i.MaxSize) for i in infos]


@pytest.mark.parametrize("case", CASES["balance"], ids=[c["name"] for c in CASES["balance"]])
def test_balance_golden(case):
    groups = _groups(case["groups"])
    got = BalancingNodeGroupSetProcessor().BalanceScaleUpBetweenGroups(groups, case["new_nodes"])
    if "sizes" in case:
        assert {i.Group.Id(): i.NewSize for i in got} == case["sizes"] and len(got) == len(case["sizes"])
    else:                                   # the reference accepts either order
        assert sorted(i.Group.Id() for i in got) == sorted(case["ids"])
        assert sorted(i.NewSize for i in got) == sorted(case["sizes_multiset"])
    assert _tuples(got) == literal_loop(groups, case["new_nodes"])


def test_balance_zero_groups_is_an_error():
    with pytest.raises(BalanceError):
        BalancingNodeGroupSetProcessor().BalanceScaleUpBetweenGroups([], 3)


@pytest.mark.parametrize("seed", range(40))
def test_balance_random_groups(seed):
    """Against an independent statement of the result (who gets the odd nodes is the sort's
    business, the literal loop above pins that): sizes within [CurrentSize, MaxSize], the sum
    min(new_nodes, capacity), and the smallest groups filled first."""
    rng = random.Random(seed)
    n = rng.choice([1, 2, 5, 13, 14, 20, 40])            # (above 12 the sort leaves its insertion-sort range)
    groups = []
    for i in range(n):
        size = rng.randint(0, 20) if rng.random() < 0.7 else rng.choice([3, 7])      # ties
        mx = max(0, size + rng.choice([-2, 0, 0, 1, 2, 5, 30]))
        groups.append(NodeGroup(f"g{i}", size, mx))
    live = [g for g in groups if g.TargetSize() < g.MaxSize()]
    capacity = sum(g.MaxSize() - g.TargetSize() for g in live)
    new_nodes = rng.choice([0, 1, 2, rng.randint(0, capacity + 1), capacity, capacity + 7])
    got = BalancingNodeGroupSetProcessor().BalanceScaleUpBetweenGroups(groups, new_nodes)
    assert _tuples(got) == literal_loop(groups, new_nodes)
    new = {g.Id(): g.TargetSize() for g in groups}
    for i in got:
        assert i.CurrentSize == new[i.Group.Id()] and i.MaxSize == i.Group.MaxSize()
        assert i.CurrentSize < i.NewSize <= i.MaxSize      # within [CurrentSize, MaxSize], changed ones only
        new[i.Group.Id()] = i.NewSize
    assert len({i.Group.Id() for i in got}) == len(got)
    assert all(i.Group.TargetSize() < i.Group.MaxSize() for i in got)        # maxed (and over-max) groups are dropped
    assert sum(i.NewSize - i.CurrentSize for i in got) == min(new_nodes, capacity)
    # no unmaxed group ends more than one above a group that received nodes: nodes go to the
    # smallest group first
    for r in got:
        for g in live:
            if new[g.Id()] < g.MaxSize():
                assert new[g.Id()] >= r.NewSize - 1, (g.Id(), r.Group.Id())


def test_filter_node_groups_by_pods_host_form():
    pods = [k8s.build_test_pod(f"p{i}", 100, 100) for i in range(5)]
    twin = k8s.build_test_pod("p0", 100, 100)                # equal to pods[0], another object
    groups = [NodeGroup(n, 1, 5) for n in ("none", "subset", "superset", "same", "twin")]
    options = {"subset": ExpansionOption(groups[1], 1, pods[:2]),
               "superset": ExpansionOption(groups[2], 2, pods[::-1]),
               "same": ExpansionOption(groups[3], 1, pods[:3]),
               "twin": ExpansionOption(groups[4], 1, [twin] + pods[1:3])}
    kept = filter_node_groups_by_pods(groups, pods[:3], options)
    assert [g.Id() for g in kept] == ["superset", "same"]
    assert [g.Id() for g in filter_node_groups_by_pods(groups, [], options)] == ["subset", "superset", "same", "twin"]


def test_scale_up_balance_groups_known_answer():
    """TestScaleUpBalanceGroups (orchestrator_test.go:763-837) through the host forms: four
    groups of 100m nodes, two pending 80m pods (one per node: an option of 2 nodes in every
    group that is not maxed), ng1 skipped as maxed; whichever option wins, ng2 and ng3 end at 2."""
    cfg = {"ng1": (1, 1, 1), "ng2": (1, 2, 1), "ng3": (1, 5, 1), "ng4": (1, 5, 3)}
    groups = [NodeGroup(g, size, mx, mn) for g, (mn, mx, size) in cfg.items()]
    infos = {g.Id(): NodeInfo(k8s.build_test_node(f"{g.Id()}-node-0", 100, 1000)) for g in groups}
    pods = [k8s.build_test_pod(f"test-pod-{i}", 80, 0) for i in range(2)]
    options = {g.Id(): ExpansionOption(g, 2, list(pods)) for g in groups if g.TargetSize() < g.MaxSize()}
    proc = BalancingNodeGroupSetProcessor()
    for best in options.values():
        similar = proc.FindSimilarNodeGroups(groups, best.node_group, infos)
        assert sorted(s.Id() for s in similar) == sorted(set(cfg) - {best.node_group.Id()})
        kept = filter_node_groups_by_pods(similar, best.pods, options)
        assert "ng1" not in [k.Id() for k in kept] and len(kept) == 2
        plan = proc.BalanceScaleUpBetweenGroups([best.node_group] + kept, best.node_count)
        assert {i.Group.Id(): i.NewSize for i in plan} == {"ng2": 2, "ng3": 2}
