"""Inputs of the device form of BuildPodGroups (ca_pod_groups_create): the reference loop
stated on the interned records (`groups_of`), and the cases the CPU and GPU tests share.

A case is (name, pods, order, node, class_owner, claim): `pods` are ca_pod_spec records (the
pod set), `order` / `node` / `class_owner` what the call takes (None = NULL), `claim` what the
case says about itself (tests/test_pod_groups.py checks it).  T is the kernels' tile of list
positions; the cases sit on it.
"""
import functools

import numpy as np

from autoscaler_amd import abi, workloads as W

T = abi.POD_GROUP_TILE
CAP = 10                                    # groups.go:57
CHUNK = abi.OPTION_LIST_CHUNK               # the scan chunk of k_option_lists downstream


def groups_of(pods, order=None, node=None, class_owner=None):
    """equivalence.BuildPodGroups (groups.go:38-102) on records: (eg_off, eg_pod) int32."""
    cls = np.asarray(pods["similar_class"]).tolist()
    ds = (np.asarray(pods["flags"]) & abi.CA_POD_DAEMONSET).tolist()
    n = len(order) if order is not None else (len(node) if node is not None else len(cls))
    groups, gid_of, registered = [], {}, {}
    for k in range(n):
        if node is not None and node[k] >= 0:
            continue
        i = int(order[k]) if order is not None else k
        c = cls[i]
        if c < 0 or ds[i]:
            groups.append([i])
            continue
        if c in gid_of:
            groups[gid_of[c]].append(i)
            continue
        o = int(class_owner[c]) if class_owner is not None else c
        if class_owner is None or registered.get(o, 0) < CAP:
            registered[o] = registered.get(o, 0) + 1
            gid_of[c] = len(groups)
        groups.append([i])
    eg_off = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=eg_off[1:])
    eg_pod = np.array([i for g in groups for i in g], np.int32).reshape(-1)
    return eg_off, eg_pod


CPU = [100, 250, 700, 1900]
MEM = [300 * W.MI, 1100 * W.MI, 2900 * W.MI, 7000 * W.MI]


def records(cls, daemonset=None):
    """ca_pod_spec records with the given similar classes (resource shape by class)."""
    cls = np.asarray(cls, np.int64)
    shape = np.where(cls >= 0, cls, np.arange(len(cls))) % 16
    p = W.resource_pods(np.array(CPU)[shape % 4], np.array(MEM)[shape // 4])
    p["similar_class"] = cls
    if daemonset is not None:
        p["flags"] |= np.where(np.asarray(daemonset, bool), abi.CA_POD_DAEMONSET, 0).astype(p["flags"].dtype)
    return p


def _node_with(n, n_unsched, rng):
    """A node column of n entries of which exactly n_unsched are -1."""
    node = rng.integers(0, 50, n).astype(np.int32)
    node[rng.choice(n, n_unsched, replace=False)] = -1
    return node


def _owner_case(K, rng, extra_placed=False):
    """One owner (0) with K classes 0..K-1 whose first occurrences run in a shuffled class
    order; every class recurs three more times later, interleaved, so pods of the classes past
    the cap lie between pods of registered ones.  A second owner (1) with 3 classes and a few
    pods without a controller are mixed in."""
    first = rng.permutation(K)
    body = np.concatenate([rng.permutation(K) for _ in range(3)])
    other = K + rng.integers(0, 3, 40)
    seq = np.concatenate([first[:K // 2], other[:10], [-1, -1], first[K // 2:], body, other[10:], [-1]])
    owner = np.array([0] * K + [1] * 3, np.int32)
    return seq.astype(np.int64), owner, first


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20)
    out = []

    def add(name, cls, order=None, node=None, class_owner=None, daemonset=None, **claim):
        pods = records(cls, daemonset)
        if order is not None:
            order = np.ascontiguousarray(order, np.int32)
        if node is not None:
            node = np.ascontiguousarray(node, np.int32)
        if class_owner is not None:
            class_owner = np.ascontiguousarray(class_owner, np.int32)
        out.append((name, pods, order, node, class_owner, claim))

    n = 2 * T + 500
    mixed = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 40, n))
    add("n_0", mixed, order=np.zeros(0, np.int32), n_unsched=0, n_eg=0)
    for k in (1, T - 1, T, T + 1, 2 * T + 1):
        add(f"unsched_{k}", mixed, node=_node_with(n, k, rng), class_owner=np.arange(40) // 4, n_unsched=k)
    add("all_placed", mixed[:T + 7], node=rng.integers(0, 9, T + 7), n_unsched=0, n_eg=0)
    add("node_none", mixed, class_owner=np.arange(40) // 4, n_unsched=n)
    add("no_class", np.full(T + 3, -1), n_unsched=T + 3, n_eg=T + 3)
    add("daemonset", rng.integers(0, 5, T + 3), daemonset=np.ones(T + 3), class_owner=np.zeros(5), n_unsched=T + 3,
        n_eg=T + 3)
    add("one_class", np.zeros(2 * T + 9), class_owner=[0], n_unsched=2 * T + 9, n_eg=1)
    gap = np.concatenate([rng.integers(1, 6, T), rng.integers(1, 6, T), rng.integers(1, 6, T)])
    gap[[5, 77, T - 1, 2 * T, 2 * T + 900]] = 0
    add("class_gap", gap, class_owner=np.zeros(6), n_unsched=3 * T, n_eg=6, tiles_of_class0=[0, 2])
    inter = np.concatenate([rng.permutation(64) for _ in range((5 * T) // 64 + 1)])[:4 * T + 300]
    add("interleaved_64", inter, class_owner=np.arange(64) // 8, n_unsched=4 * T + 300, n_eg=64, n_tiles=5)
    for K in (10, 11, 25):
        seq, owner, first = _owner_case(K, rng)
        add(f"owner_{K}", seq, class_owner=owner, cut=sorted(first[CAP:].tolist()), not_in_id_order=True)
        if K == 25:
            add("owner_25_nocap", seq, class_owner=None, cut=[], n_eg=K + 3 + 3)
    # an owner whose placed pods alone would have used up the cap: classes 0..11 occur first, all
    # placed; classes 12..17 follow unplaced and are all registered
    cls = np.concatenate([np.arange(12), np.repeat(np.arange(12, 18), 3), np.arange(12, 18)])
    node = np.concatenate([np.arange(12), np.full(24, -1)])
    add("placed_fill_cap", cls, node=node, class_owner=np.zeros(18), n_unsched=24, n_eg=6, cut=[])
    # a class whose first pods were placed and later ones were not
    cls = np.array([3, 3, 1, 3, 1, 3, 2, 3])
    add("first_placed", cls, node=[4, 4, -1, -1, -1, 7, -1, -1], class_owner=[0, 0, 0, 1], n_unsched=5, n_eg=3)
    seq = np.concatenate([rng.permutation(400), rng.integers(0, 400, 1200)])
    add("owner_400", seq, class_owner=np.zeros(400), n_unsched=1600, n_cut_classes=390)
    per = rng.integers(1, 13, 3000)
    owner = np.repeat(np.arange(3000), per).astype(np.int32)
    seq = rng.permutation(np.concatenate([np.arange(len(owner)), rng.integers(0, len(owner), 500)]))
    add("owners_3000", seq, class_owner=owner, n_owners=3000, max_per_owner=12)
    sh = np.where(rng.random(3 * T) < 0.05, -1, rng.integers(0, 30, 3 * T))
    add("shuffled_order", sh, order=rng.permutation(3 * T), node=_node_with(3 * T, T + 11, rng),
        class_owner=np.arange(30) // 15, n_unsched=T + 11)
    add("subset_order", sh, order=rng.permutation(3 * T)[:T + 5], class_owner=np.arange(30) // 15, n_unsched=T + 5,
        subset=True)
    for E in (CHUNK - 1, CHUNK, CHUNK + 1):
        # E groups: E - 20 classes of 8 owners (none past the cap ... 30 per owner: cut) is avoided
        # by giving every class its own owner
        seq = np.concatenate([np.arange(E - 20), np.full(20, -1), rng.integers(0, E - 20, 700)])
        add(f"n_eg_{E}", rng.permutation(seq), class_owner=np.arange(E - 20), n_eg=E)
    return out


CASE_NAMES = ["n_0", "unsched_1", f"unsched_{T - 1}", f"unsched_{T}", f"unsched_{T + 1}", f"unsched_{2 * T + 1}",
              "all_placed", "node_none", "no_class", "daemonset", "one_class", "class_gap", "interleaved_64",
              "owner_10", "owner_11", "owner_25", "owner_25_nocap", "placed_fill_cap", "first_placed", "owner_400",
              "owners_3000", "shuffled_order", "subset_order", f"n_eg_{CHUNK - 1}", f"n_eg_{CHUNK}", f"n_eg_{CHUNK + 1}"]


def case(name):
    return next(c for c in cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """groups_of of a case, computed once and shared."""
    _, pods, order, node, class_owner, _ = case(name)
    eg_off, eg_pod = groups_of(pods, order, node, class_owner)
    eg_off.setflags(write=False)
    eg_pod.setflags(write=False)
    return eg_off, eg_pod


def cut_classes(pods, order, node, class_owner):
    """The classes of an owner past its first CAP, by first occurrence among the listed pods."""
    if class_owner is None:
        return []
    cls = np.asarray(pods["similar_class"])
    ds = np.asarray(pods["flags"]) & abi.CA_POD_DAEMONSET
    n = len(order) if order is not None else (len(node) if node is not None else len(cls))
    seen, per_owner, cut = set(), {}, []
    for k in range(n):
        if node is not None and node[k] >= 0:
            continue
        i = int(order[k]) if order is not None else k
        c = int(cls[i])
        if c < 0 or ds[i] or c in seen:
            continue
        seen.add(c)
        o = int(class_owner[c])
        per_owner[o] = per_owner.get(o, 0) + 1
        if per_owner[o] > CAP:
            cut.append(c)
    return sorted(cut)
