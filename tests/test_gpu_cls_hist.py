"""The class counts a plan keeps beside its lists (k_cls_hist at plan creation, read back with
ca_estimate_plan_fetch_class_counts) against numpy.bincount over the plan's own item classes
(fetch_lists()[1]), per group, for the three constructors: host lists, the option matrix and
device-resident pod groups.  k_run_table starts every run's table from these counts, so the
smallest batches of test_gpu_table_chain's kind also run against the CPU restatement with the
run-table chain and with the stream path (CASIM_TABLE_CHAIN=0: k_emit_runs reads the same
table).

Pod i of a table with U classes is of class i mod U, so a list of ascending pods changes class
at every position (the worst case for the per-run adds), a list sorted by class is long runs.
"""
import numpy as np
import pytest

import optgen
import test_gpu_table_chain as tc
from autoscaler_amd import abi, native, workloads as W

pytestmark = pytest.mark.gpu

T = abi.CLS_HIST_TILE
LENGTHS = (0, 1, 63, 64, 65, T - 1, T, T + 1)


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


@pytest.fixture(scope="module")
def mirror():
    m = native.Mirror(0)
    m.clear()
    yield m
    m.close()


def _table(U, n, per_controller=50):
    cls = np.arange(n) % U
    pods = W.resource_pods(100 + cls.astype(np.int64), np.full(n, 64 * W.MI, np.int64))
    pods["similar_class"] = np.arange(n) // per_controller
    return abi.PodTable(pods), cls


def _lists(groups):
    off = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=off[1:])
    idx = np.concatenate([np.asarray(g, np.int32) for g in groups]) if off[-1] else np.zeros(0, np.int32)
    return off, idx.astype(np.int32)


def _check_counts(plan, U, what, want_cls=None):
    off = plan.group_off
    _, item_cls = plan.fetch_lists()
    cnt = plan.fetch_class_counts()
    assert cnt.shape == (plan.G, U) and cnt.dtype == np.int32, (what, cnt.shape)
    if plan.total == 0:
        assert not cnt.any(), what
        return
    assert item_cls is not None, what
    if want_cls is not None:
        assert np.array_equal(item_cls, want_cls), what
    for g in range(plan.G):
        want = np.bincount(item_cls[off[g]:off[g + 1]], minlength=U)
        assert np.array_equal(cnt[g], want), (what, g, int(off[g + 1] - off[g]))


def _host_groups(U, n):
    """Lists over a table of n pods in U classes: every length around the wave step and the
    tile (ascending pods: a class change at every position when U > 1), a list past 65,536
    positions, one class alone, one class absent, long runs."""
    pods = np.arange(n)
    groups = [pods[:k] for k in LENGTHS if k <= n]
    groups.append(np.arange(70_000) % n)
    groups.append(np.resize(pods[pods % U == U // 2], 5000))                 # all one class
    groups.append(pods[:0])                                                  # (empty, between long ones)
    groups.append(pods[np.argsort(pods % U, kind="stable")])                 # runs of n / U
    if U > 1:
        groups.append(np.resize(pods[pods % U != 1], T + 700))               # class 1 absent
        groups.append(np.resize(pods[(pods % U == 0) | (pods % U == U - 1)], 2 * T + 1))   # two classes alternate
    return groups


@pytest.mark.parametrize("U,n", [(1, 300), (64, 9000), (65, 9000), (4096, 8192)])
def test_host_lists(U, n, mirror):
    table, cls = _table(U, n)
    groups = _host_groups(U, n)
    off, idx = _lists(groups)
    assert int(np.diff(off).max()) == 70_000
    with native.EstimatePlan(mirror, table, off, idx, optgen._templates(len(groups))) as plan:
        _check_counts(plan, U, ("host", U), want_cls=cls[idx])
        if U > 1:
            cnt = plan.fetch_class_counts()
            assert cnt[len(groups) - 2][1] == 0 and cnt[len(groups) - 2].sum() == T + 700      # the absent class
            assert np.count_nonzero(cnt[len(LENGTHS) + 1]) == 1                                 # one class alone


def test_batch_without_items(mirror):
    table, _ = _table(64, 500)
    off, idx = _lists([[], [], []])
    with native.EstimatePlan(mirror, table, off, idx, optgen._templates(3)) as plan:
        _check_counts(plan, 64, "empty batch")


@pytest.mark.parametrize("U", [1, 64, 65])
def test_option_matrix_and_device_groups(U, mirror):
    """Lists built on the device from the option matrix (k_option_lists writes the classes the
    histogram reads), with the equivalence groups uploaded and with the device-resident CSR."""
    n = 9000
    table, cls = _table(U, n, per_controller=37)
    with mirror.podset(table) as ps, native.PodGroups(mirror, ps) as g:
        eg_off, eg_pod = g.fetch()
        E = g.n_groups
        assert E > 1
        ok = optgen._rows(E, np.random.default_rng(U))               # zeros, ones, alternating, random rows
        tm = optgen._templates(len(ok))
        with native.EstimatePlan.from_options(mirror, ps, eg_off, eg_pod, ok, tm) as a, \
                native.EstimatePlan.from_groups(mirror, ps, g, ok, tm) as b:
            want_off, want_idx = optgen.lists_of(eg_off, eg_pod, ok)
            lens = np.diff(want_off)
            assert lens.min() == 0 and lens.max() == n > 2 * T       # an empty list and one over two tiles
            for what, plan in (("options", a), ("groups", b)):
                assert plan.group_off.tobytes() == want_off.tobytes()
                _check_counts(plan, U, (what, U), want_cls=cls[want_idx])


@pytest.mark.parametrize("max_nodes", [0, 2])
def test_run_table_from_the_counts(max_nodes, oracle, monkeypatch):
    """Small batches through the run-table chain and the stream path, both fed by k_run_table
    from the plan's counts: absent classes, the merge rule, non-batchable classes."""
    batches = [
        ([[("s1", 30), ("s2", 25), ("s3", 40), ("bottom", 20)], [("top", 12), ("s1", 30), ("s3", 40)],
          [("top", 9), ("bottom", 70)], [("s2", 33)]], [tc.T_MID, tc.T_SMALL, tc.T_WIDE, tc.T_MID]),
        ([[("s2", 20), ("ma", 40), ("mb", 30), ("s3", 25)], [("s2", 30), ("port", 9), ("s3", 30)],
          [("ma", 10), ("port", 5), ("fpga", 6), ("bottom", 40)]], [tc.T_MID, tc.T_MID, tc.T_WIDE]),
    ]
    for groups, tm in batches:
        tc._check(oracle, monkeypatch, tc._inputs(groups, tm), max_nodes, all_modes=True)
