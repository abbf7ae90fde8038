"""The copy-on-fork model (tests/snapmodel.py) against the CPU oracle: random sequences with
the whole state checked after every step, pinned single cases of the fit rule and of Revert,
and the coverage the seed set must reach.  tests/test_gpu_snapshot_state.py drives the GPU
mirror with the same seeds, so a failure there reproduces here without a device.  The pinned
cases run on the mirror as well (`-m gpu`).
"""
import numpy as np
import pytest

import snapmodel as S
from autoscaler_amd import abi
from snapmodel import GI, LIST_SEEDS, LIST_STEPS, PROBE_SEEDS, PROBE_STEPS


@pytest.fixture(scope="module")
def oracle(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def probe_runs(oracle):
    """The probe-checked sequences, run once: their coverage records and probe statistics."""
    stats, covs = {}, []
    for seed in PROBE_SEEDS:
        covs.append(S.run_sequence(seed, [oracle.OracleState()], PROBE_STEPS, stats=stats).cov)
    return covs, stats


@pytest.fixture(scope="module")
def list_runs(oracle):
    return [S.run_sequence(seed, [oracle.OracleState()], LIST_STEPS, with_probes=False).cov for seed in LIST_SEEDS]


def test_model_against_oracle_lists(list_runs):
    assert len(list_runs) == len(LIST_SEEDS)


def test_model_against_oracle_probes(probe_runs):
    assert len(probe_runs[0]) == len(PROBE_SEEDS)


@pytest.mark.parametrize("which", ["lists", "probes"])
def test_sequence_coverage(which, list_runs, probe_runs):
    covs = list_runs if which == "lists" else probe_runs[0]
    tot = {k: sum(c[k] for c in covs) for k in covs[0] if k != "max_depth"}
    for op in S.OPS:
        assert tot[op] > 0, f"op {op} never occurs"
    for k in S.KINDS:
        assert tot[f"revert_over_{k}"] > 0, f"no revert crosses a {k} entry"
    assert max(c["max_depth"] for c in covs) >= 3
    assert tot["commit_then_outer_revert"] > 0
    assert tot["remove_node_depth0"] > 0
    assert tot["node_added_removed_in_fork"] > 0
    assert tot["shared_port"] > 0, "no two pods share a port triple on one node"
    assert tot["overcommitted"] > 0, "no overcommitted node"
    assert tot["blockers"] > 0


def test_probe_sets_are_not_all_pass(probe_runs):
    """In at least 90 % of the checked steps every dimension of the probe set holds a fitting
    and a non-fitting (probe, node) cell."""
    stats = probe_runs[1]
    assert stats["checked"] >= 0.9 * len(PROBE_SEEDS) * PROBE_STEPS
    assert stats["covered"] >= 0.9 * stats["checked"], stats


# ---------------------------------------------------------------------------
# pinned single cases
# ---------------------------------------------------------------------------
@pytest.fixture(params=["oracle", pytest.param("native", marks=pytest.mark.gpu)])
def make(request, oracle):
    """The backend under the pinned cases: the oracle, and the GPU mirror."""
    if request.param == "oracle":
        return oracle.OracleState
    from autoscaler_amd import native
    return lambda: native.Mirror(0)


def _pair(make, table, nodes):
    m, o = S.SnapModel(table), make()
    m.add_nodes(nodes)
    o.add_nodes(nodes)
    return m, o


def _both(m, o, op, *a):
    if op == "add_pods":
        ids = m.add_pods(*a)
        assert o.add_pods(m.table, *a).tolist() == ids
        return ids
    getattr(m, op)(*a)
    getattr(o, op)(*a)


def _fits(oracle_state, rec, node=0) -> bool:
    return oracle_state.check_predicates(abi.PodTable(rec), 0, node)[0] == abi.CA_PRED_OK


def _model_fits(m, rec) -> list:
    return S.expected_fits(m, S.Probes([rec], [("pin", "pin")]))[0].astype(bool).tolist()


def _overcommitted(make):
    """Node 0 with every free value negative (cpu, memory, ephemeral-storage, scalar 0) and free
    slots; node 1 the same node empty."""
    table = abi.PodTable(np.concatenate([S.pod_record(cpu=1500, mem=5 * GI, eph=11 * GI, scalar=5,
                                                      flags=abi.CA_POD_HAS_SCALAR_KEYS)]))
    nodes = np.concatenate([S.node_record(i, 1000, 4 * GI, 10 * GI, 10, 4) for i in range(2)])
    m, o = _pair(make, table, nodes)
    _both(m, o, "add_pods", [0], [0])
    f = m.free(0)
    assert max(f["cpu"], f["mem"], f["eph"], f["scalar"][0]) < 0 < f["slots"]
    return m, o


def test_all_zero_shortcut(make):
    m, o = _overcommitted(make)
    zero = S.pod_record()
    keyed = S.pod_record(flags=abi.CA_POD_HAS_SCALAR_KEYS)
    assert _model_fits(m, zero) == [True, True] == [_fits(o, zero, x) for x in (0, 1)]
    # with scalar keys the shortcut is off: 0 > free fails in cpu, memory and ephemeral-storage
    assert _model_fits(m, keyed) == [False, True] == [_fits(o, keyed, x) for x in (0, 1)]
    S.assert_state(o, m, "all-zero shortcut")


@pytest.mark.parametrize("neg", ["cpu", "mem", "eph"])
def test_zero_request_against_negative_free(neg, make):
    """A pod that asks for one resource fails where another one's free value is negative."""
    big = dict(cpu=1500, mem=5 * GI, eph=11 * GI)
    table = abi.PodTable(np.concatenate([S.pod_record(**{neg: big[neg]})]))
    m, o = _pair(make, table, S.node_record(0, 1000, 4 * GI, 10 * GI, 10))
    _both(m, o, "add_pods", [0], [0])
    assert m.free(0)[neg] < 0
    other = {"cpu": "mem", "mem": "eph", "eph": "cpu"}[neg]
    probe = S.pod_record(**{other: 1})
    assert _model_fits(m, probe) == [False] == [_fits(o, probe)]
    assert _model_fits(m, S.pod_record()) == [True] == [_fits(o, S.pod_record())]
    S.assert_state(o, m, f"negative free {neg}")


def test_zero_scalar_request_against_negative_free_scalar(make):
    table = abi.PodTable(np.concatenate([S.pod_record(scalar=5, flags=abi.CA_POD_HAS_SCALAR_KEYS)]))
    m, o = _pair(make, table, S.node_record(0, 1000, 4 * GI, 10 * GI, 10, 4))
    _both(m, o, "add_pods", [0], [0])
    assert m.free(0)["scalar"][0] == -1
    probe = S.pod_record(cpu=1, flags=abi.CA_POD_HAS_SCALAR_KEYS)      # scalar request 0: the column is skipped
    assert _model_fits(m, probe) == [True] == [_fits(o, probe)]
    probe = S.pod_record(cpu=1, scalar=1, flags=abi.CA_POD_HAS_SCALAR_KEYS)
    assert _model_fits(m, probe) == [False] == [_fits(o, probe)]
    S.assert_state(o, m, "negative free scalar")


def test_shared_port_triple(make):
    table = abi.PodTable(np.concatenate([S.pod_record(cpu=100, port=3), S.pod_record(mem=100, port=3)]))
    m, o = _pair(make, table, S.node_record(0, 1000, 4 * GI, 0, 10))
    a, b = _both(m, o, "add_pods", [0, 1], [0, 0])
    probe = S.pod_record(port=3)
    assert _model_fits(m, probe) == [False] == [_fits(o, probe)]
    _both(m, o, "fork")
    _both(m, o, "remove_pod", a)
    assert o.node_pods(0) == [b] == m.nodes[0].pods
    assert _model_fits(m, probe) == [True] == [_fits(o, probe)]        # the other holder still sits there
    S.assert_state(o, m, "shared port, one holder removed")
    _both(m, o, "revert")
    assert _model_fits(m, probe) == [False] == [_fits(o, probe)]
    S.assert_state(o, m, "shared port, reverted")


@pytest.mark.parametrize("n_pods,victim", [(3, 2), (1, 0), (3, 0)], ids=["last-pod", "only-pod", "first-pod"])
def test_remove_pod_revert(n_pods, victim, make):
    table = abi.PodTable(np.concatenate([S.pod_record(cpu=100 + i, port=S.PORT_BITS[i]) for i in range(3)]))
    m, o = _pair(make, table, S.node_record(0, 1000, 4 * GI, 0, 10))
    ids = _both(m, o, "add_pods", list(range(n_pods)), [0] * n_pods)
    _both(m, o, "fork")
    _both(m, o, "remove_pod", ids[victim])
    S.assert_state(o, m, "removed")
    _both(m, o, "revert")
    assert m.nodes[0].pods == ids
    S.assert_state(o, m, "reverted")


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_remove_node_revert(where, make):
    seq = S.Sequence(77, n_nodes=7)
    o = make()
    seq.load([o])
    m = seq.model
    _both(m, o, "add_pods", list(range(14)), [i % 7 for i in range(14)])
    pos = {"first": 0, "middle": 3, "last": 6}[where]
    _both(m, o, "fork")
    _both(m, o, "remove_node", pos)
    S.assert_state(o, m, f"remove_node {where}")
    _both(m, o, "add_pods", [1, 2], [0, 5])
    _both(m, o, "revert")
    S.assert_state(o, m, f"remove_node {where} reverted")
    assert m.node_count() == 7
