"""Inputs of the option-matrix form of the Estimate plan (ca_estimate_plan_create_options):
the numpy statement of ComputeExpansionOption's append loop, the option form of an
EstimateWorkload, and the cases the CPU and GPU tests share.

A case is (name, workload, eg_off, eg_pod, ok, templates): `workload` names the podset and the
existing nodes (most cases share BASE's), the rest is what the constructor takes.  T is the
kernel's output tile and C its scan chunk; the cases sit on both.
"""
import functools

import numpy as np

from autoscaler_amd import abi, workloads as W

T, C = abi.OPTION_LIST_TILE, abi.OPTION_LIST_CHUNK
GI = W.GI


def lists_of(eg_off, eg_pod, ok):
    """option.Pods of every node group (orchestrator.go:468-482): for e ascending with
    ok[g][e] != 0, the pods of equivalence group e.  Returns (group_off, pod_idx)."""
    eg_off = np.asarray(eg_off, np.int64)
    eg_pod = np.asarray(eg_pod, np.int32)
    ok = np.asarray(ok)
    off, parts = [0], []
    for g in range(ok.shape[0]):
        n = 0
        for e in np.nonzero(ok[g])[0]:
            seg = eg_pod[eg_off[e]:eg_off[e + 1]]
            parts.append(seg)
            n += len(seg)
        off.append(off[-1] + n)
    pod_idx = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return np.array(off, np.int32), pod_idx


def equivalence_groups(workload):
    """The pod equivalence groups of a workload's podset as a CSR: pods of one similar_class
    (their controller) in pod order, groups in first-occurrence order; a pod without one
    (similar_class < 0) alone."""
    sc = np.asarray(workload.table.pods["similar_class"], np.int64)
    groups, where = [], {}
    for i, c in enumerate(sc.tolist()):
        if c < 0:
            groups.append([i])
        elif c in where:
            groups[where[c]].append(i)
        else:
            where[c] = len(groups)
            groups.append([i])
    eg_off = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=eg_off[1:])
    eg_pod = np.array([i for g in groups for i in g], np.int32)
    return eg_off, eg_pod


def options_of(workload):
    """(eg_off, eg_pod, ok) of an EstimateWorkload: its equivalence groups, and ok[g][e] = the
    sample (first pod) of group e is in node group g's list.  For the workloads whose lists are
    whole controllers in pod order (C2, C4), lists_of gives back their group_off / pod_idx."""
    eg_off, eg_pod = equivalence_groups(workload)
    G, E = len(workload.templates), len(eg_off) - 1
    ok = np.zeros((G, E), np.uint8)
    sample = eg_pod[eg_off[:-1]] if E else np.zeros(0, np.int32)
    member = np.zeros(len(workload.table), bool)
    for g in range(G):
        member[:] = False
        member[workload.pod_idx[workload.group_off[g]:workload.group_off[g + 1]]] = True
        ok[g] = member[sample]
    return eg_off, eg_pod, ok


def _templates(n, rng=None, shapes=None):
    """Templates every pod of base() fits on (as every pod of an option's list does: its group's
    sample passed CheckPredicates on the template), of three cpu : memory ratios."""
    shapes = shapes or TEMPLATE_SHAPES[:4]
    tm = np.zeros(n, abi.TEMPLATE_DTYPE)
    for g in range(n):
        cpu, mem = shapes[g % len(shapes)] if rng is None else shapes[int(rng.integers(0, len(shapes)))]
        tm[g] = W.make_template(cpu, mem, 110, g % 3, name_id=-1000 - g)[0]
    return tm


def _csr(lens, first=0):
    eg_off = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=eg_off[1:])
    return eg_off, np.arange(first, first + int(eg_off[-1]), dtype=np.int32)


def _rows(E, rng):
    """zeros, ones, alternating (both phases), first and last failing, random."""
    alt = (np.arange(E) % 2).astype(np.uint8)
    inner = np.ones(E, np.uint8)
    inner[0] = inner[-1] = 0
    return np.stack([np.zeros(E, np.uint8), np.ones(E, np.uint8), alt, 1 - alt, inner,
                     (rng.random(E) < 0.5).astype(np.uint8)])


BASE_CPU = [100, 250, 700, 1900]
BASE_MEM = [300 * W.MI, 1100 * W.MI, 2900 * W.MI, 7000 * W.MI]
TEMPLATE_SHAPES = [(8000, 32 * GI), (16000, 64 * GI), (6000, 48 * GI), (32000, 64 * GI), (8000, 128 * GI)]


def score_ties(shapes, templates):
    """Pairs of distinct pod shapes whose float64 scores (cpu / alloc cpu + memory / alloc memory,
    binpacking_estimator.go:164-193) are equal on one of the templates."""
    ties = 0
    for acpu, amem in templates:
        sc = [float(c) / float(acpu) + float(m) / float(amem) for c, m in shapes]
        ties += len(sc) - len(set(sc))
    return ties


@functools.lru_cache(maxsize=None)
def base():
    """The podset most cases share: 20 000 pods of 16 shapes in controllers of 50, identical but
    for their controller (uniform score classes), and no two shapes tie on any template used
    here, so the plans take the decoupled Go order unless a knob forbids it."""
    rng = np.random.default_rng(5)
    n, per = 20_000, 50
    shapes = [(c, m) for c in BASE_CPU for m in BASE_MEM]
    ctrl_shape = rng.integers(0, len(shapes), n // per)
    cpu = np.array([shapes[s][0] for s in np.repeat(ctrl_shape, per)], np.int64)
    mem = np.array([shapes[s][1] for s in np.repeat(ctrl_shape, per)], np.int64)
    pods = W.resource_pods(cpu, mem)
    pods["similar_class"] = np.repeat(np.arange(n // per), per)
    existing = abi.empty_nodes(40)
    existing["alloc_milli_cpu"] = 16000
    existing["alloc_memory"] = 64 * GI
    existing["alloc_pods"] = 110
    existing["name_id"] = np.arange(40)
    return W.EstimateWorkload("options-base", abi.PodTable(pods), np.zeros(1, np.int32), np.zeros(0, np.int32),
                              np.zeros(0, abi.TEMPLATE_DTYPE), 40, 0, existing, {})


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(77)
    b = base()
    P = len(b.table)
    out = []

    # list lengths 0, 1, T-1, T, T+1, 2T+1 from groups of 1, T-2, 1, 1, T pods
    eg_off, eg_pod = _csr([1, T - 2, 1, 1, T], first=100)
    ok = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 1, 0, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 1, 0],
                   [1, 1, 1, 1, 1]], np.uint8)
    out.append(("lengths", b, eg_off, eg_pod, ok, _templates(6), {"lengths": [0, 1, T - 1, T, T + 1, 2 * T + 1]}))

    # one equivalence group longer than 3T between short ones
    eg_off, eg_pod = _csr([3, 3 * T + 5, 7, 2], first=0)
    ok = np.array([[0, 1, 0, 0], [1, 1, 1, 1], [1, 0, 1, 1], [0, 1, 0, 1]], np.uint8)
    out.append(("long_group", b, eg_off, eg_pod, ok, _templates(4), {"max_eg": 3 * T + 5}))

    # every pod its own group (a permutation of the pods: the lists are not ascending)
    n = 3 * C + 17
    eg_off = np.arange(n + 1, dtype=np.int32)
    eg_pod = rng.permutation(P)[:n].astype(np.int32)
    out.append(("singletons", b, eg_off, eg_pod, _rows(n, rng), _templates(6), {"n_eg": n}))

    # n_eg at 1, C-1, C, C+1: groups of 1..40 pods, some empty
    for E in (1, C - 1, C, C + 1):
        lens = rng.integers(0, 41, E)
        lens[0] = max(lens[0], 1)
        eg_off, _ = _csr(lens)
        eg_pod = rng.permutation(P)[: int(eg_off[-1])].astype(np.int32)
        ok = _rows(E, rng) if E > 1 else np.ones((1, 1), np.uint8)
        out.append((f"n_eg_{E}", b, eg_off, eg_pod, ok, _templates(len(ok)), {"n_eg": E, "n_groups": len(ok)}))

    # 300 node groups
    lens = rng.integers(5, 30, 40)
    eg_off, _ = _csr(lens)
    eg_pod = rng.permutation(P)[: int(eg_off[-1])].astype(np.int32)
    ok = (rng.random((300, 40)) < 0.4).astype(np.uint8)
    out.append(("groups_300", b, eg_off, eg_pod, ok, _templates(300, rng), {"n_groups": 300}))

    # equal rows: on templates that rank the classes alike (groups 0, 2: same allocatable; 3: both
    # doubled) one sort serves them; group 1 has the row on a template of another cpu : memory
    # ratio, group 4 another row
    lens = rng.integers(20, 60, 30)
    eg_off, _ = _csr(lens)
    eg_pod = rng.permutation(P)[: int(eg_off[-1])].astype(np.int32)
    row = (rng.random(30) < 0.6).astype(np.uint8)
    other = row.copy()
    other[3] ^= 1
    tm = np.zeros(5, abi.TEMPLATE_DTYPE)
    for g, (cpu, mem) in enumerate([(8000, 32 * GI), (8000, 128 * GI), (8000, 32 * GI), (16000, 64 * GI), (8000, 32 * GI)]):
        tm[g] = W.make_template(cpu, mem, 110, 0, name_id=-1000 - g)[0]
    out.append(("equal_rows", b, eg_off, eg_pod, np.stack([row, row, row, row, other]), tm, {}))

    # workloads of their own: cross-class score ties (the coupled path), non-uniform classes (C4),
    # more than 256 score classes (the comparison sort)
    from estgen import tied_workload
    tw, _ = tied_workload(1, n_pods=3000, n_groups=6)
    out.append(("tied", tw, *options_of(tw), tw.templates, {}))
    c4 = W.c4(n_pods=3000, n_groups=8, n_existing=40, pods_per_controller=30)
    out.append(("c4", c4, *options_of(c4), c4.templates, {}))
    wide = W.c2(n_pods=4000, n_groups=6, n_existing=40, pods_per_controller=10, n_random_shapes=400)
    out.append(("classes_400", wide, *options_of(wide), wide.templates, {"min_classes": 257}))
    return out


def case(name):
    return next(c for c in cases() if c[0] == name)


CASE_NAMES = ["lengths", "long_group", "singletons", "n_eg_1", f"n_eg_{C - 1}", f"n_eg_{C}", f"n_eg_{C + 1}",
              "groups_300", "equal_rows", "tied", "c4", "classes_400"]
