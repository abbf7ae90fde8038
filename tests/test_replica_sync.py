"""ClusterSnapshot.sync_replica on the oracle backend: a second OracleState made to hold the
snapshot by replaying the facade's log with the current interner, and the stamp that makes a
second call a no-op while nothing changed.  The sharded ScaleUp path syncs the replicas of a
native.Multi this way (tests/test_gpu_multi_expander.py runs that on the device)."""
import pytest

from autoscaler_amd import k8s
from autoscaler_amd.clustersnapshot import ClusterSnapshot
from autoscaler_amd.k8s import Taint, Toleration

GI = 1 << 30


def _state(backend):
    """Per node position: the oracle's row (free cpu / memory / ..., distinct per node here) and
    its pods' ids in NodeInfo.Pods order."""
    n = backend.node_count()
    return [(backend.node_state(i), backend.node_pods(i)) for i in range(n)]


def _probe_pods():
    pods = [k8s.build_test_pod("probe-small", 300, GI), k8s.build_test_pod("probe-big", 5000, 8 * GI),
            k8s.build_test_pod("probe-huge", 900000, GI)]
    pods[1].node_selector = {"pool": "b"}
    pods[0].tolerations.append(Toleration(key="dedicated", operator="Exists"))
    return pods


def _same(snap, replica):
    """Node order with every node's row and pods, and FitsAnyNode of a few pending pods from
    several lastIndex values, on the replica and on the backend."""
    table = snap.encode(_probe_pods())
    snap.sync_replica(replica)                     # (encoding the probes may itself have re-interned)
    assert _state(replica) == _state(snap.backend)

    def answers(backend):
        return [backend.fits_any_node(table, i, None, li)[:2] for i in range(3) for li in (0, 2, 5)]
    got, want = answers(replica), answers(snap.backend)
    assert got == want and any(node >= 0 for node, _ in want)


def _nodes(n, first=0):
    out = []
    for i in range(first, first + n):
        node = k8s.build_test_node(f"n{i}", 4000 + 1000 * i, (8 + i) * GI, 110)
        node.labels["pool"] = "ab"[i % 2]
        out.append(node)
    return out


def test_sync_replica_follows_the_log(oracle_lib):
    snap = ClusterSnapshot(oracle_lib.OracleState())
    replica = oracle_lib.OracleState()
    nodes = _nodes(6)
    snap.AddNodes(nodes)
    for i in range(10):
        snap.AddPod(k8s.build_scheduled_test_pod(f"p{i}", 200 + 10 * i, GI, f"n{i % 6}"), f"n{i % 6}")
    assert snap.sync_replica(replica) is True
    _same(snap, replica)
    loads = snap.replica_loads
    assert snap.sync_replica(replica) is False and snap.replica_loads == loads       # nothing changed: by stamp

    snap.RemovePod("default", "p3", "n3")
    snap.SetNodeOrder([f"n{i}" for i in (4, 0, 5, 2, 1, 3)])
    assert snap.sync_replica(replica) is True
    _same(snap, replica)

    snap.Fork()
    snap.AddNodeWithPods(_nodes(1, first=6)[0], [k8s.build_scheduled_test_pod("forked", 700, GI, "n6")])
    snap.RemovePod("default", "p0", "n0")
    assert snap.sync_replica(replica) is True
    _same(snap, replica)

    # a node with a label pair and a taint nobody interned yet: the facade re-encodes and replays
    # its backend; the replica's records are of the old encoding until it is synced again
    before = snap._sizes()
    late = k8s.build_test_node("late", 3000, 4 * GI, 110)
    late.labels["pool"] = "c"
    late.labels["tier"] = "gold"
    late.taints.append(Taint("dedicated", "x", "NoSchedule"))
    snap.AddNode(late)
    assert snap._sizes() != before
    assert snap.sync_replica(replica) is True
    _same(snap, replica)
    assert snap.sync_replica(replica) is False

    snap.Revert()
    assert snap.sync_replica(replica) is True
    _same(snap, replica)
    assert replica.node_count() == 6


def test_sync_replica_stamp(oracle_lib):
    """The stamp names the snapshot and its version: another snapshot's replica is reloaded, the
    backend itself never is, and reads (List, encode of known objects) do not move the stamp."""
    a, b = ClusterSnapshot(oracle_lib.OracleState()), ClusterSnapshot(oracle_lib.OracleState())
    a.AddNodes(_nodes(3))
    b.AddNodes(_nodes(2))
    replica = oracle_lib.OracleState()
    assert a.sync_replica(replica) and not a.sync_replica(replica)
    a.List()
    a.node_names()
    assert not a.sync_replica(replica)
    assert b.sync_replica(replica) and replica.node_count() == 2
    assert a.sync_replica(replica) and replica.node_count() == 3
    assert a.sync_replica(a.backend) is False and a.replica_loads == 2
    # a snapshot with the same number of ops (the same version count) is still another snapshot
    c = ClusterSnapshot(oracle_lib.OracleState())
    c.AddNodes(_nodes(3, first=10))
    assert c._version == a._version and c.sync_replica(replica)
    assert _state(replica) == _state(c.backend) and a.sync_replica(replica)
    assert not hasattr(replica, "_replica_stamp")          # (nothing is written on the backend object)
    a.Clear()
    assert a.sync_replica(replica) and replica.node_count() == 0


def test_sync_replica_needs_the_reorder_call_for_a_logged_order(oracle_lib):
    """A backend with reorder_nodes logs SetNodeOrder as an op (the oracle backend, without the
    call, logs the canonical form instead); a replica without the call cannot apply that op."""
    snap = ClusterSnapshot(oracle_lib.OracleState())
    snap.AddNodes(_nodes(2))
    snap._log.append(("order", ["n1", "n0"]))          # (what a native.Mirror backend would have logged)
    snap._version += 1
    with pytest.raises(TypeError):
        snap.sync_replica(oracle_lib.OracleState())
