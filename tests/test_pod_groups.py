"""The device form of BuildPodGroups, the parts that need no device: the record statement of
the reference loop (groupgen.groups_of) against the two host forms, the cases the GPU test
runs, and the library's new entry points."""
import ctypes as C
import random

import numpy as np

import groupgen
from groupgen import T, CAP, CHUNK
from autoscaler_amd import abi, k8s, native, runonce
from autoscaler_amd.intern import Interner
from autoscaler_amd.k8s import OwnerReference
from autoscaler_amd.scaleup import BuildPodGroups

GI, MI = 1 << 30, 1 << 20


def _random_pods(seed):
    """Pods of a few controllers with 1 to 25 label variants each, DaemonSet pods and pods
    without a controller."""
    rng = random.Random(seed)
    variants = {f"rs{c}": rng.choice([1, 3, 9, 10, 11, 14, 25]) for c in range(rng.randint(1, 5))}
    pods = []
    for i in range(rng.randint(1, 260)):
        p = k8s.build_test_pod(f"p{i}", rng.choice([100, 250]), rng.choice([128, 256]) * MI)
        u = rng.random()
        if u < 0.08:
            pass                                                   # no controller
        elif u < 0.16:
            p.owner_refs = [OwnerReference("DaemonSet", "ds", "ds")]
            p.labels = {"v": str(rng.randint(0, 2))}
        else:
            rs = rng.choice(sorted(variants))
            p.owner_refs = [OwnerReference("ReplicaSet", rs, rs)]
            p.labels = {"v": str(rng.randint(0, variants[rs] - 1))}
        pods.append(p)
    return pods, rng


def _names(groups_csr, pods):
    eg_off, eg_pod = groups_csr
    return [[pods[i].name for i in eg_pod[eg_off[e]:eg_off[e + 1]]] for e in range(len(eg_off) - 1)]


def test_groups_of_is_build_pod_groups_on_interned_pods():
    capped = 0
    for seed in range(30):
        pods, rng = _random_pods(seed)
        it = Interner()
        it.observe([], pods, [])
        table = it.encode_pods(pods)
        cls = table.pods["similar_class"]
        owner = it.class_owners(int(cls.max()) + 1 if len(cls) else 0)
        want = [[p.name for p in g.pods] for g in BuildPodGroups(pods)]
        got = groupgen.groups_of(table.pods, None, None, owner)
        assert _names(got, pods) == want, seed
        capped += bool(groupgen.cut_classes(table.pods, None, None, owner))
        if seed % 2:
            # through a shuffled order with a node column: BuildPodGroups of the listed pods
            order = list(range(len(pods)))
            rng.shuffle(order)
            node = [rng.choice([-1, -1, 3]) for _ in order]
            listed = [pods[i] for k, i in enumerate(order) if node[k] < 0]
            want = [[p.name for p in g.pods] for g in BuildPodGroups(listed)]
            got = groupgen.groups_of(table.pods, np.array(order, np.int32), np.array(node, np.int32), owner)
            assert _names(got, pods) == want, seed
    assert capped >= 5                                             # the cap was in play


def test_groups_of_is_the_runonce_helper_below_the_cap():
    rng = np.random.default_rng(4)
    for trial in range(6):
        n = int(rng.integers(1, 3000))
        cls = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 60, n))
        pods = groupgen.records(cls)
        order = rng.permutation(n).astype(np.int32)
        node = np.where(rng.random(n) < 0.4, 2, -1).astype(np.int32)
        want = runonce._equivalence_groups(pods, order[node < 0])
        owner = (np.arange(60) // CAP).astype(np.int32)           # at most CAP classes per owner
        for co in (None, owner):
            eg_off, eg_pod = groupgen.groups_of(pods, order, node, co)
            got = [eg_pod[eg_off[e]:eg_off[e + 1]].tolist() for e in range(len(eg_off) - 1)]
            assert got == want, trial


def test_cases_hold_what_they_claim():
    cases = {c[0]: c for c in groupgen.cases()}
    assert list(cases) == groupgen.CASE_NAMES
    assert (T, CAP, CHUNK) == (2048, 10, 256)
    for name, pods, order, node, owner, claim in cases.values():
        assert len(pods) <= 21_000, name
        n = len(order) if order is not None else (len(node) if node is not None else len(pods))
        if order is not None and len(order):
            assert order.min() >= 0 and order.max() < len(pods) and len(np.unique(order)) == len(order), name
        if owner is not None:
            elig = pods["similar_class"][(pods["flags"] & abi.CA_POD_DAEMONSET) == 0]
            assert owner.min() >= 0 and elig.max(initial=-1) < len(owner), name
        eg_off, eg_pod = groupgen.expected(name)
        n_unsched = n if node is None else int((node < 0).sum())
        assert eg_off[-1] == len(eg_pod) == n_unsched and (np.diff(eg_off) >= 1).all(), name
        assert len(np.unique(eg_pod)) == len(eg_pod), name
        if "n_unsched" in claim:
            assert n_unsched == claim["n_unsched"], name
        if "n_eg" in claim:
            assert len(eg_off) - 1 == claim["n_eg"], name
        cut = groupgen.cut_classes(pods, order, node, owner)
        if "cut" in claim:
            assert cut == claim["cut"], name
        if "n_cut_classes" in claim:
            assert len(cut) == claim["n_cut_classes"], name
        if cut:
            # a pod of a cut class is a group of its own every time it occurs
            size = np.diff(eg_off)
            for e in np.nonzero(np.isin(pods["similar_class"][eg_pod[eg_off[:-1]]], cut))[0]:
                assert size[e] == 1, name
            assert np.isin(pods["similar_class"][eg_pod], cut).sum() > len(cut), name
    # every pod placed / none listed
    assert cases["all_placed"][3].min() >= 0 and len(cases["n_0"][2]) == 0
    assert cases["node_none"][3] is None and cases["node_none"][2] is None
    # singletons for both reasons
    assert (cases["no_class"][1]["similar_class"] < 0).all()
    ds = cases["daemonset"][1]
    assert (ds["similar_class"] >= 0).all() and (ds["flags"] & abi.CA_POD_DAEMONSET).all()
    # class 0 of class_gap sits in tiles 0 and 2 of the list and not in tile 1
    where = np.nonzero(cases["class_gap"][1]["similar_class"] == 0)[0]
    assert sorted(set((where // T).tolist())) == cases["class_gap"][5]["tiles_of_class0"] == [0, 2]
    # 64 classes, each with members in all 5 tiles, never two equal neighbours in a row of 64
    inter = cases["interleaved_64"][1]["similar_class"]
    assert -(-len(inter) // T) == 5
    for c in range(64):
        assert set((np.nonzero(inter == c)[0] // T).tolist()) == set(range(5))
    # the capped owners: first occurrences are not in class-id order, and a cut class recurs
    # between pods of registered classes
    for K in (10, 11, 25):
        name, pods, order, node, owner, claim = cases[f"owner_{K}"]
        cls = pods["similar_class"]
        mine = cls[(cls >= 0) & (cls < K)]
        _, first = np.unique(mine, return_index=True)
        assert (np.diff(first) < 0).any() and (owner[:K] == 0).all()
        assert len(claim["cut"]) == max(0, K - CAP)
        for c in claim["cut"]:
            pos = np.nonzero(cls == c)[0]
            reg = np.nonzero((cls >= 0) & (cls < K) & ~np.isin(cls, claim["cut"]))[0]
            assert len(pos) == 4 and ((reg > pos[1]) & (reg < pos[-1])).any()
    assert cases["owner_25_nocap"][4] is None
    assert cases["owner_25_nocap"][1].tobytes() == cases["owner_25"][1].tobytes()
    # the placed pods alone would have used up the cap
    name, pods, order, node, owner, _ = cases["placed_fill_cap"]
    placed_classes = set(pods["similar_class"][node >= 0].tolist())
    assert len(placed_classes) > CAP and (owner == 0).all()
    assert groupgen.cut_classes(pods, order, None, owner) != []           # (counted, they would cut)
    # a class whose first pods were placed
    name, pods, order, node, owner, _ = cases["first_placed"]
    assert node[0] >= 0 and node[1] >= 0 and pods["similar_class"][0] == 3 and node[3] < 0
    eg_off, eg_pod = groupgen.expected("first_placed")
    assert eg_pod.tolist() == [2, 4, 3, 7, 6] and eg_off.tolist() == [0, 2, 4, 5]
    assert (cases["owner_400"][4] == 0).all() and len(cases["owner_400"][4]) == 400
    per = np.bincount(cases["owners_3000"][4])
    assert len(per) == 3000 and per.min() >= 1 and per.max() == 12 and (per > CAP).any()
    assert groupgen.cut_classes(*cases["owners_3000"][1:5])
    name, pods, order, node, owner, _ = cases["shuffled_order"]
    assert sorted(order.tolist()) == list(range(len(pods))) and (np.diff(order) < 0).any()
    assert len(cases["subset_order"][2]) < len(cases["subset_order"][1])


def test_hand_case():
    """The loop by hand: owner 0 holds classes 0..11, class 10 and 11 come first."""
    cls = [10, 11, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 8, 9, 0, -1]
    pods = groupgen.records(cls)
    eg_off, eg_pod = groupgen.groups_of(pods, None, None, np.zeros(12, np.int32))
    got = [eg_pod[eg_off[e]:eg_off[e + 1]].tolist() for e in range(len(eg_off) - 1)]
    assert got == [[0, 12], [1], [2, 15], [3], [4], [5], [6], [7], [8], [9], [10], [11], [13], [14], [16]]


def test_library_exports_the_pod_group_calls():
    lib = native.load()
    for f in ("ca_pod_groups_create", "ca_pod_groups_info", "ca_pod_groups_fetch", "ca_pod_groups_timings",
              "ca_pod_groups_destroy", "ca_expansion_plan_run_groups", "ca_estimate_plan_create_groups"):
        assert hasattr(lib, f), f
        assert f in native.exported_symbols()
    out = (C.c_int32 * 32)()
    n = lib.ca_abi_struct_sizes(out, 32)
    assert list(out[:n]) == abi.EXPECTED_SIZES                         # additive: no record changed
    assert lib.ca_abi_version() == abi.CASIM_ABI_VERSION
    assert callable(native.Mirror.build_pod_groups) and callable(native.EstimatePlan.from_groups)
    assert abi.POD_GROUP_TILE == T
