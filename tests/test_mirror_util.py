"""Scale-down eligibility from the mirror, the parts that need no device: the default-row rule
(utilgen.rows_of) against utilization.build_table on k8s objects, the cases against the CPU
oracle (each holds what it claims), the classification rule against runonce.run's host split,
and the library's new exports."""
import ctypes as C
import math

import numpy as np
import pytest

import utilgen
from autoscaler_amd import abi, native, runonce
from autoscaler_amd import utilization as U
from autoscaler_amd import workloads as W
from autoscaler_amd.clustersnapshot import NodeInfo
from autoscaler_amd.intern import Interner
from autoscaler_amd.k8s import OwnerReference, build_test_node, build_test_pod, set_rs_pod

NEW_CALLS = ("ca_mirror_utilization", "ca_scale_down_candidates_create", "ca_scale_down_candidates_info",
             "ca_scale_down_candidates_fetch", "ca_scale_down_candidates_timings",
             "ca_scale_down_candidates_destroy", "ca_removal_plan_create_candidates")


def test_library_exports_the_scale_down_calls():
    lib = native.load()
    for f in NEW_CALLS:
        assert hasattr(lib, f), f
        assert f in native.exported_symbols()
    out = (C.c_int32 * 32)()
    n = lib.ca_abi_struct_sizes(out, 32)
    assert list(out[:n]) == abi.EXPECTED_SIZES                         # additive: no record changed
    assert lib.ca_abi_version() == abi.CASIM_ABI_VERSION
    assert callable(native.Mirror.utilization) and callable(native.ScaleDownCandidates.removal_plan)
    assert callable(native.RemovalPlan.from_handle) and callable(U.CalculateAllOnSnapshot)


def _object_cluster():
    """Nodes and pods as k8s objects: several containers, an init container larger than the
    containers (it counts for the fit, not for utilization), DaemonSet pods by owner and by
    annotation, a pod without requests."""
    infos = []
    for i in range(5):
        node = build_test_node(f"n{i}", 2000 + 500 * i, (4 + i) * utilgen.GI)
        pods = []
        for k in range(i + 1):
            p = set_rs_pod(build_test_pod(f"p{i}-{k}", 100 + 50 * k, (64 + k) * utilgen.MI), "rs")
            if k % 2:                                            # a second container
                extra = build_test_pod("x", 30, 5 * utilgen.MI).containers[0]
                p.containers = p.containers + [extra]
            if k == 2:                                           # init container above the containers' sum
                p.init_containers = [build_test_pod("i", 900, 512 * utilgen.MI).containers[0]]
            pods.append(p)
        ds = build_test_pod(f"ds{i}", 70, 32 * utilgen.MI)
        ds.owner_refs = [OwnerReference("DaemonSet", "ds")]
        pods.append(ds)
        if i == 3:
            ann = build_test_pod("ds-ann", 20, utilgen.MI)
            ann.owner_refs = [OwnerReference("CustomDaemonSet", "cds")]
            ann.annotations = {"cluster-autoscaler.kubernetes.io/daemonset-pod": "true"}
            pods.append(ann)
            pods.append(build_test_pod("none", -1, -1))
        infos.append(NodeInfo(node, pods))
    return infos


def test_default_rows_are_build_table_rows():
    infos = _object_cluster()
    want_nodes, want_off, want_pods = U.build_table(infos, [None] * len(infos))
    it = Interner()
    it.observe([ni.node for ni in infos], [p for ni in infos for p in ni.pods])
    nodes = it.encode_nodes([ni.node for ni in infos])
    specs = it.encode_pods([p for ni in infos for p in ni.pods]).pods
    lists = [list(range(int(a), int(b))) for a, b in zip(want_off[:-1], want_off[1:])]
    un, off, up = utilgen.rows_of(nodes, specs, lists)
    assert un.tobytes() == want_nodes.tobytes()
    assert np.array_equal(off, want_off)
    assert np.array_equal(up["req_milli"], want_pods["req_milli"])
    init = [k for k, p in enumerate(p for ni in infos for p in ni.pods) if p.init_containers]
    assert init and all(specs["req_milli_cpu"][k] > specs["score_milli_cpu"][k] for k in init)   # containers only
    # the DaemonSet bit is the table's; everything else is movable until the host says otherwise
    ds = (want_pods["flags"] & abi.CA_UPOD_DAEMONSET) != 0
    assert ds.sum() == 6
    assert np.array_equal(up["flags"], np.where(ds, abi.CA_UPOD_DAEMONSET, abi.CA_UPOD_MOVABLE))


@pytest.mark.parametrize("name", utilgen.CASE_NAMES)
def test_cases_are_well_formed(name, oracle_lib):
    c = utilgen.case(name)
    lists = c.node_lists()
    on_node = sorted(i for l in lists for i in l)
    assert on_node == sorted(set(range(len(c.pods))) - set(c.removed))
    for over in (c.node_over, c.pod_over):
        if over is not None:
            assert np.all(np.diff(over[0]) > 0) and len(over[0]) == len(over[1])
    for sds in (False, True):
        info, drain = utilgen.expected(name, sds, sds)
        assert len(info) == len(c.nodes) == len(drain)
        assert np.array_equal(info["empty"] != 0, drain == 0)


def test_case_sizes_sit_on_the_edges():
    n = {len(utilgen.case(k).nodes) for k in utilgen.CASE_NAMES}
    assert {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025} <= n
    assert {len(utilgen.case(f"p_{p}").pods) for p in (65535, 65536, 65537)} == {65535, 65536, 65537}
    per = sorted(len(l) for l in utilgen.case("pods_per_node").node_lists())
    assert {0, 1, 15, 16, 17, 255, 256, 257} <= set(per)
    c = utilgen.case("detached")
    assert 0 in c.removed and len(c.pods) - 1 in c.removed and 1 not in c.removed      # interleaved with live ids
    assert len(utilgen.case("over_all").pod_over[0]) == len(utilgen.case("over_all").pods)
    c = utilgen.case("over_detached")
    assert set(c.removed) <= set(c.pod_over[0].tolist())
    assert utilgen.case("over_first_last").pod_over[0].tolist() == [0, len(utilgen.case("over_first_last").pods) - 1]
    assert not utilgen.case("eligible_none").eligible.any()


def test_edges_hold_what_they_claim(oracle_lib):
    c = utilgen.case("edges")
    k = c.claims
    plain, _ = utilgen.expected("edges", False, False)
    skip, drain = utilgen.expected("edges", True, True)
    un, off, up = c.rows()
    assert up["req_milli"][off[0]:off[1], 0].sum() == 1 << 62 and plain["cpu"][k["sum62"]] == (1 << 62) / ((1 << 62) + (1 << 61))
    assert math.isinf(skip["utilization"][k["inf"]]) and plain["utilization"][k["inf"]] > 1.0
    assert math.isnan(skip["utilization"][k["nan"]]) and skip["status"][k["nan"]] == abi.CA_UTIL_OK
    assert plain["cpu"][k["rounded"]] == float(2**52) / float(2**53 + 1) and float(2**53 + 1) == float(2**53)
    assert plain["utilization"][k["equal"]] == 0.5
    assert plain["cpu"][k["counted"]] == 0.6 and plain["cpu"][k["dropped"]] == 0.0
    assert plain["resource"][k["gpu"]] == abi.CA_UTIL_GPU and plain["gpu"][k["gpu"]] == 0.5
    assert plain["resource"][k["gpu_unready"]] == abi.CA_UTIL_GPU and plain["utilization"][k["gpu_unready"]] == 0.0
    for node, st in k["status"].items():
        assert plain["status"][node] == st
    assert drain[k["blocked"]] == abi.CA_UPOD_MOVABLE | abi.CA_UPOD_BLOCKING
    assert all(plain["empty"][x] for x in k["empty"])
    # the classes: NaN is below, equality is not, one ulp under a raised threshold is
    for name, sds in (("edges", False), ("edges", True), ("edges_ulp", False)):
        cc = utilgen.case(name)
        info, dr = utilgen.expected(name, sds, sds)
        got = utilgen.candidates_of(info, dr, cc.thr, cc.gpu_thr, cc.eligible, cc.node_lists(), cc.pod_flags())
        cls = got["node_class"]
        assert cls[k["equal"]] == (abi.CA_SD_CANDIDATE if name == "edges_ulp" else abi.CA_SD_NOT_BELOW)
        if sds:                                                  # NaN counts as below; (flags off: 1.0, not below)
            assert math.isnan(info["utilization"][k["nan"]]) and cls[k["nan"]] == abi.CA_SD_EMPTY
        assert cls[k["gpu"]] == abi.CA_SD_CANDIDATE              # 0.5 under the GPU threshold 0.6
        assert all(cls[x] == abi.CA_SD_UTIL_ERROR for x in k["status"])
        assert cls[k["blocked"]] == abi.CA_SD_CANDIDATE
        c_at = got["cand"].tolist().index(k["blocked"])
        assert got["cand_status"][c_at] == abi.CA_UNREMOVABLE_BLOCKED_BY_POD
        assert got["move_off"][c_at + 1] - got["move_off"][c_at] == 1     # the blocking pod itself is not movable
        assert cls[k["dropped"]] == abi.CA_SD_CANDIDATE and cls[k["counted"]] == abi.CA_SD_NOT_BELOW
    got = utilgen.candidates_of(*utilgen.expected("eligible_none", False, False), 0.5, 0.5,
                                utilgen.case("eligible_none").eligible, utilgen.case("eligible_none").node_lists(),
                                utilgen.case("eligible_none").pod_flags())
    assert (got["node_class"] == abi.CA_SD_INELIGIBLE).all() and len(got["cand"]) == len(got["empty"]) == 0


def test_nan_empty_class_claim(oracle_lib):
    """The DaemonSet-only node is empty in both flag settings; with the flags off its
    utilization is 1.0 (not below), with them on it is NaN (below, class 1)."""
    c = utilgen.case("edges")
    x = c.claims["nan"]
    for sds, want in ((False, abi.CA_SD_NOT_BELOW), (True, abi.CA_SD_EMPTY)):
        info, dr = utilgen.expected("edges", sds, sds)
        cls = utilgen.candidates_of(info, dr, c.thr, c.gpu_thr, None, c.node_lists(), c.pod_flags())["node_class"]
        assert cls[x] == want and dr[x] == 0


def test_candidates_rule_is_the_loops_host_split(oracle_lib):
    """candidates_of on the oracle loop's utilization rows gives runonce.run's candidates and
    empty nodes (every pod of the synthetic cluster is movable)."""
    w = runonce.c5_runonce(n_nodes=600, n_pending=1500, n_groups=12)
    o = oracle_lib.OracleState()
    W.load_filter(o, w.filt)
    r = runonce.run(o, oracle_lib.runonce_cpu_util, w)
    lists = [o.node_pods(x) for x in range(len(w.filt.nodes))]
    n_ids = max(max(l) for l in lists if l) + 1
    flags = np.full(n_ids, abi.CA_UPOD_MOVABLE, np.uint32)
    drain = np.array([abi.CA_UPOD_MOVABLE if l else 0 for l in lists], np.int32)
    got = utilgen.candidates_of(r.util, drain, runonce.UTIL_THRESHOLD, runonce.UTIL_THRESHOLD, None, lists, flags)
    assert len(r.candidates) > 0
    assert np.array_equal(got["cand"], r.candidates) and np.array_equal(got["empty"], r.empty)
    assert not got["cand_status"].any()
    assert got["move_off"][-1] == r.sizes["pods_to_move"]
