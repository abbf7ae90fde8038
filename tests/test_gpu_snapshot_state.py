"""The GPU mirror's whole state against the copy-on-fork model (tests/snapmodel.py) after
every kind of mutation: node_count, every pod list in order, pod_node of every id ever issued,
scope_blockers, and the device rows through fits_matrix of probes that bracket every positive
free value of every row (`assert_state`).  The path tests read Mirror.sync_stats() to know
which upload ran.  The thresholds are mirror.hip's:

  sync_nodes            full upload when `dirty_rows.size() > std::max<size_t>(64, n / 4)` (:736)
  sync_nodes            `cap = std::max<size_t>(n, std::max<size_t>(1024, d_cap * 2))` (:722)
  sync_nodes            fill threads `std::min<size_t>(8, n / 2048)` (:742)
  add_placed_batch      threads `std::min(8, np / 2048)`, rounded down to a power of two (:503)
  k_remap_hints         256 threads per block (:702); restore shifts `v >= pos` (:417)

The random sequences use the seeds of tests/test_snapshot_model.py: a failure here reproduces
on the oracle there without a device.
"""
import numpy as np
import pytest

import plangen
import snapmodel as S
import tspgen as T
from autoscaler_amd import abi, native
from autoscaler_amd import workloads as W
from snapmodel import GI, PROBE_SEEDS, PROBE_STEPS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle(oracle_lib):
    return oracle_lib


def _delta(m, before: dict) -> dict:
    now = m.sync_stats()
    return {k: now[k] - before[k] for k in now}


# ---------------------------------------------------------------------------
# random sequences
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", PROBE_SEEDS)
def test_random_sequence_small(seed):
    m = native.Mirror(0)
    stats = {}
    s = S.run_sequence(seed, [m], PROBE_STEPS, n_nodes=12, stats=stats)
    assert stats["checked"] > PROBE_STEPS // 2 and s.cov["revert"] > 0
    m.close()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_sequence_300_nodes(seed):
    """Dirty sets below n / 4 = 75 rows go through the staged scatter, RemoveNode and its
    Revert through the full upload."""
    m = native.Mirror(0)
    S.run_sequence(seed, [m], 160, n_nodes=300, every=8)
    st = m.sync_stats()
    assert st["staged_syncs"] > 0 and st["full_syncs"] > 0
    m.close()


# ---------------------------------------------------------------------------
# staged against full upload
# ---------------------------------------------------------------------------
def _cluster(n: int, seed: int, n_pods: int = 0):
    """A mirror and a model with n generated nodes and n_pods pods, synced by a check."""
    seq = S.Sequence(seed, n_nodes=n)
    m = native.Mirror(0)
    seq.load([m])
    if n_pods:
        idx = [seq.rng.randrange(len(seq.table) - 1) for _ in range(n_pods)]      # (the last record is the blocker)
        pos = [seq.rng.randrange(n) for _ in range(n_pods)]
        assert m.add_pods(seq.table, idx, pos).tolist() == seq.model.add_pods(idx, pos)
    S.assert_state(m, seq.model, f"{n} nodes loaded")
    return seq, m


def _dirty(seq, m, k: int, new_node: bool):
    """Dirty exactly k rows by one add_pods each; the first row twice; with new_node one of
    the k is a node added since the last sync (row index >= d_rows)."""
    model, n = seq.model, seq.model.node_count()
    rows = list(range(0, 2 * k, 2))[:k] if 2 * k <= n else list(range(k))
    if new_node:
        rec = S.gen_nodes(seq.rng, 1, 100000)
        model.add_nodes(rec)
        m.add_nodes(rec)
        rows[-1] = n
    rows.append(rows[0])
    idx = [(3 + 5 * j) % (len(seq.table) - 1) for j in range(len(rows))]
    for i, x in zip(idx, rows):
        assert m.add_pods(seq.table, [i], [x]).tolist() == model.add_pods([i], [x])


def _assert_path(d: dict, k: int, n: int, what: str) -> None:
    staged = k <= max(64, n // 4)                # mirror.hip sync_nodes (:736)
    if k == 0:                                   # nothing dirty: no upload of either kind
        assert (d["full_syncs"], d["staged_syncs"]) == (0, 0), f"{what}: {d}"
        return
    want = {"full_syncs": 0 if staged else 1, "staged_syncs": 1 if staged else 0, "rows_staged": k if staged else 0}
    got = {f: d[f] for f in want}
    assert got == want, f"{what}: k={k} n={n}: {got}, expected {want}"


STAGED_CASES = [(200, 1), (200, 63), (200, 64), (200, 65), (400, 99), (400, 100), (400, 101)]


@pytest.mark.parametrize("new_node", [False, True], ids=["rows", "new-node"])
@pytest.mark.parametrize("n,k", STAGED_CASES)
def test_staged_against_full(n, k, new_node):
    seq, m = _cluster(n, 1000 + n, n_pods=n)
    before = m.sync_stats()
    _dirty(seq, m, k, new_node)
    S.assert_state(m, seq.model, f"{k} dirty rows of {n}")
    d = _delta(m, before)
    _assert_path(d, k, seq.model.node_count(), "add_pods")
    assert d["static_uploads"] == int(new_node)
    m.close()


@pytest.mark.parametrize("new_node", [False, True], ids=["rows", "new-node"])
@pytest.mark.parametrize("n,k", STAGED_CASES)
def test_staged_against_full_revert(n, k, new_node):
    """The same rows dirtied by a Revert: fork, k adds, sync, revert, check."""
    seq, m = _cluster(n, 2000 + n, n_pods=n)
    seq.model.fork()
    m.fork()
    _dirty(seq, m, k, new_node)
    S.assert_state(m, seq.model, "forked")
    before = m.sync_stats()
    seq.model.revert()
    m.revert()
    S.assert_state(m, seq.model, f"revert of {k} dirty rows of {n}")
    # (the added node is gone again: its row is no row of the k any more)
    _assert_path(_delta(m, before), k - int(new_node), n, "revert")
    m.close()


# ---------------------------------------------------------------------------
# capacity growth at 1024 rows
# ---------------------------------------------------------------------------
def test_capacity_growth_in_fork():
    seq, m = _cluster(1000, 31, n_pods=300)
    model, table = seq.model, seq.table
    assert m.sync_stats()["growths"] == 1        # the first sync: 1024 rows (mirror.hip :722)

    def both(op, *a):
        getattr(model, op)(*a)
        getattr(m, op)(*a)

    def add_pods(pos):
        idx = [(7 * x) % (len(table) - 1) for x in pos]
        assert m.add_pods(table, idx, pos).tolist() == model.add_pods(idx, pos)

    both("fork")
    both("add_nodes", S.gen_nodes(seq.rng, 30, 5000))
    add_pods([1001, 1029, 1024, 1023, 0])
    S.assert_state(m, model, "30 nodes added in a fork")
    assert m.sync_stats()["growths"] == 2
    both("revert")
    S.assert_state(m, model, "growth reverted")
    both("add_nodes", S.gen_nodes(seq.rng, 30, 6000))
    add_pods([1000, 1029, 1024])
    S.assert_state(m, model, "30 other nodes")
    both("fork")
    both("fork")
    both("add_nodes", S.gen_nodes(seq.rng, 30, 7000))
    add_pods([1030, 1059, 1024, 5])
    both("remove_pod", model.nodes[1024].pods[0])
    S.assert_state(m, model, "inner fork")
    both("commit")
    S.assert_state(m, model, "inner fork committed")
    both("revert")
    S.assert_state(m, model, "outer fork reverted")
    assert m.sync_stats()["growths"] == 2
    m.close()


# ---------------------------------------------------------------------------
# threaded fill
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,threads", [(4100, 2), (16400, 8)])
def test_threaded_fill(n, threads):
    """Uniform nodes (taints and labels by position, so a shifted static row shows) with two
    pod shapes each; RemoveNode at the first thread's last row (2047 of 2048 per thread,
    mirror.hip :742) inside a fork, and its Revert."""
    table = abi.PodTable(np.concatenate([S.pod_record(cpu=S.CPU_REQ, mem=S.MEM_REQ),
                                         S.pod_record(cpu=2 * S.CPU_REQ + 1, port=3)]))
    nodes = abi.empty_nodes(n)
    nodes[:] = S.node_record(0, 4000, 16 * GI, 10 * GI, 10, 4)[0]
    pos = np.arange(n)
    nodes["name_id"] = pos
    nodes["taints"] = np.array(S.TAINT_SETS, np.uint64)[pos % 4]
    nodes["label_pairs"][:, 0] = np.array(S.LABEL_SETS, np.uint64)[pos % 5]
    model, m = S.SnapModel(table), native.Mirror(0)
    model.add_nodes(nodes)
    m.add_nodes(nodes)
    idx = np.tile(np.array([0, 1], np.int32), n)
    at = np.repeat(pos, 2).astype(np.int32)
    keep = (at % 3 != 0) | (idx == 0)            # every third node: the first shape only
    assert m.add_pods(table, idx[keep], at[keep]).tolist() == model.add_pods(idx[keep].tolist(), at[keep].tolist())
    S.assert_state(m, model, f"{n} nodes loaded")
    st = m.sync_stats()
    assert (st["full_syncs"], st["fill_threads"]) == (1, threads), st
    for op, what in (("fork", None), ("remove_node", 2047), ("revert", None)):
        a = () if what is None else (what,)
        getattr(model, op)(*a)
        getattr(m, op)(*a)
        if op != "fork":
            S.assert_state(m, model, f"{n} nodes, {op}")
    assert m.sync_stats()["fill_threads"] == threads
    m.close()


# ---------------------------------------------------------------------------
# hints by name
# ---------------------------------------------------------------------------
N_HINT_NODES = 9


def _hinted(n_pods: int):
    """9 nodes, n_pods pods round-robin, hints to every node and -1 in turn."""
    seq = S.Sequence(5, n_nodes=N_HINT_NODES)
    m = native.Mirror(0)
    seq.load([m])
    idx = [i % (len(seq.table) - 1) for i in range(n_pods)]
    pos = [i % N_HINT_NODES for i in range(n_pods)]
    assert m.add_pods(seq.table, idx, pos).tolist() == seq.model.add_pods(idx, pos)
    hints = [(i * 7) % (N_HINT_NODES + 1) - 1 for i in range(n_pods)]              # -1 .. 8
    seq.model.set_hints(hints)
    m.set_hints(hints)
    S.assert_state(m, seq.model, "hints set", hints=True)
    return seq.model, m, seq


def _ops(model, m, ops, what):
    for step, op in enumerate(ops):
        name, a = (op, ()) if isinstance(op, str) else (op[0], op[1:])
        getattr(model, name)(*a)
        getattr(m, name)(*a)
        S.assert_state(m, model, f"{what} step {step} op {op}", hints=True)


HINT_SCRIPTS = {
    "first": ["fork", ("remove_node", 0), "revert"],
    "middle": ["fork", ("remove_node", 4), "revert"],
    "last": ["fork", ("remove_node", N_HINT_NODES - 1), "revert"],
    "twice-at-one-position": ["fork", ("remove_node", 3), ("remove_node", 3), "revert"],
    "nested-revert-inner": ["fork", ("remove_node", 2), "fork", ("remove_node", 5), "revert", "revert"],
    "commit-inner-revert-outer": ["fork", ("remove_node", 6), "fork", ("remove_node", 0), "commit", "revert"],
    "depth-0": [("remove_node", 4), ("remove_node", 0), "fork", ("remove_node", 2), "revert"],
}


@pytest.mark.parametrize("script", list(HINT_SCRIPTS))
@pytest.mark.parametrize("n_pods", [255, 256, 257, 1025])
def test_hints_by_name(n_pods, script):
    model, m, _ = _hinted(n_pods)
    _ops(model, m, HINT_SCRIPTS[script], f"{n_pods} pods, {script}")
    m.close()


@pytest.mark.parametrize("n_pods", [255, 256, 257, 1025])
def test_hints_survive_growth(n_pods):
    """Pods added after set_hints: the buffer grows (reserve_keep), the old hints stay, the
    new pods read -1; then a removal and its Revert over the grown buffer."""
    model, m, seq = _hinted(n_pods)
    more = 3 * n_pods + 5
    idx = [i % (len(seq.table) - 1) for i in range(more)]
    pos = [(i * 5) % N_HINT_NODES for i in range(more)]
    assert m.add_pods(seq.table, idx, pos).tolist() == model.add_pods(idx, pos)
    S.assert_state(m, model, "pods added after set_hints", hints=True)
    assert (m.get_hints(n_pods + more)[n_pods:] == -1).all()
    _ops(model, m, ["fork", ("remove_node", 1), ("remove_node", 6), "revert"], "grown")
    m.close()


# ---------------------------------------------------------------------------
# after every entry point that writes state
# ---------------------------------------------------------------------------
def _dims(nodes, *tables) -> dict:
    """The scalar columns and port bits a workload uses (the oracle-based probes of them)."""
    sc = {k for k in range(abi.CA_MAX_SCALAR)
          if nodes["alloc_scalar"][:, k].any() or any(t.pods["req_scalar"][:, k].any() for t in tables)}
    bits = set()
    for t in tables:
        for w in range(abi.CA_PORT_WORDS):
            word = int(np.bitwise_or.reduce(t.pods["port_use"][:, w])) if len(t) else 0
            bits |= {64 * w + b for b in range(64) if (word >> b) & 1}
    return dict(scalar_cols=sorted(sc), port_bits=sorted(bits))


def _check_both(g, o, n_pods, what, dims, fresh=None):
    S.assert_state_oracle(g, o, n_pods, what, **dims)
    if fresh is not None:                        # a mirror loaded from scratch passes the same check
        f = native.Mirror(0)
        fresh(f)
        S.assert_state_oracle(f, o, fresh.n_pods, what + " (fresh mirror)", **dims)
        f.close()


class _Fresh:
    def __init__(self, load, n_pods):
        self.load, self.n_pods = load, n_pods

    def __call__(self, b):
        self.load(b)


FILTER_CFG = {"loose-tiny": dict(n_nodes=37, pods_per_node=10, n_pending=900, hint_frac=0.3, util_low=(0.1, 0.3),
                                 util_high=(0.3, 0.5)),
              "small": dict(n_nodes=500, pods_per_node=20, n_pending=2000)}
_FW = {}


def _filter_workload(cfg):
    if cfg not in _FW:
        _FW[cfg] = W.c5_filter(**FILTER_CFG[cfg])
    return _FW[cfg]


@pytest.mark.parametrize("forked", [False, True], ids=["unforked", "forked"])
@pytest.mark.parametrize("path", ["bitmap", "window"])
@pytest.mark.parametrize("cfg", list(FILTER_CFG))
def test_after_filter_out_schedulable(cfg, path, forked, oracle, monkeypatch):
    """Also after an add_nodes since the last sync: rows the walk wrote itself are dropped from
    the dirty list (bitmap: the device-rows counter moves; window: it does not)."""
    if path == "window":
        monkeypatch.setenv("CASIM_FO_WINDOW", "1")
    w = _filter_workload(cfg)
    g, o = native.Mirror(0), oracle.OracleState()
    dims = _dims(w.nodes, w.table, w.pending)
    extra = w.nodes[:3].copy()
    extra["name_id"] = 10 ** 6 + np.arange(3)
    for b in (g, o):
        W.load_filter(b, w)
    _check_both(g, o, len(w.table), "loaded", dims)
    for b in (g, o):
        if forked:
            b.fork()
        b.add_nodes(extra)                       # rows past d_rows when the call syncs
    before = g.sync_stats()
    rg = g.filter_out_schedulable(w.pending, w.order, w.class_owner, w.hints, 3)
    ro = o.filter_out_schedulable(w.pending, w.order, w.class_owner, w.hints, 3)
    assert g.filter_stats()["path"] == path
    assert np.array_equal(rg.node, ro.node) and rg.placed == ro.placed > 0
    d = _delta(g, before)
    assert (d["device_rows"] > 0) if path == "bitmap" else (d["device_rows"] == 0), d
    n_pods = len(w.table) + rg.placed
    _check_both(g, o, n_pods, f"{cfg} {path} filtered", dims)
    if forked:
        g.revert()
        o.revert()
        _check_both(g, o, n_pods, f"{cfg} {path} reverted", dims, _Fresh(lambda b: W.load_filter(b, w), len(w.table)))
    g.close()


def test_after_filter_threaded_placements(oracle):
    """>= 4096 placements on >= 128 nodes inside a fork: add_placed_batch journals them on
    several host threads (2048 placements per thread, mirror.hip :503)."""
    n, n_pending = 160, 5000
    nodes = abi.empty_nodes(n)
    nodes["alloc_milli_cpu"], nodes["alloc_memory"], nodes["alloc_pods"] = 64000, 256 * GI, 110
    nodes["name_id"] = np.arange(n)
    running = abi.PodTable(W.resource_pods(np.full(n, 500, np.int64), np.full(n, GI, np.int64)))
    pend = W.resource_pods(np.array([100, 150, 250], np.int64)[np.arange(n_pending) % 3],
                           np.array([GI // 4, GI // 8], np.int64)[np.arange(n_pending) % 2])
    pending = abi.PodTable(pend)
    g, o = native.Mirror(0), oracle.OracleState()
    dims = dict(scalar_cols=[], port_bits=[])

    def load(b):
        b.clear()
        b.add_nodes(nodes)
        b.add_pods(running, np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32))

    for b in (g, o):
        load(b)
        b.fork()
    rg = g.filter_out_schedulable(pending, None, None, None, 0)
    ro = o.filter_out_schedulable(pending, None, None, None, 0)
    assert np.array_equal(rg.node, ro.node)
    assert rg.placed >= 4096 and len(np.unique(rg.node[rg.node >= 0])) >= 128
    assert g.sync_stats()["placed_threads"] >= 2, g.sync_stats()
    n_pods = n + rg.placed
    _check_both(g, o, n_pods, "threaded placements", dims)
    g.revert()
    o.revert()
    _check_both(g, o, n_pods, "threaded placements reverted", dims, _Fresh(load, n))
    g.close()


@pytest.mark.parametrize("brk", [False, True], ids=["all", "break"])
@pytest.mark.parametrize("wn,mn", [("n37", "half"), ("n300", "altwords")])
def test_after_try_schedule_pods(wn, mn, brk, oracle):
    w = T.workload(wn)
    match = T.make_match(mn, w, T.L0)
    g, o = native.Mirror(0), oracle.OracleState()
    dims = _dims(w.nodes, w.table, w.pending)
    for b in (g, o):
        W.load_filter(b, w)
        b.fork()
    ref = T.try_schedule_ref(o, w.pending, w.order, match, brk, w.class_owner, w.hints, T.L0)
    got = g.try_schedule_pods(w.pending, w.order, match, brk, w.class_owner, w.hints, T.L0)
    T.eq_try(got, ref, (wn, mn, brk))
    assert got.placed > 0
    n_pods = len(w.table) + got.placed
    _check_both(g, o, n_pods, f"try_schedule {wn} {mn}", dims)
    g.revert()
    o.revert()
    _check_both(g, o, n_pods, f"try_schedule {wn} {mn} reverted", dims,
                _Fresh(lambda b: W.load_filter(b, w), len(w.table)))
    g.close()


def _plan_case(chain: bool):
    case = plangen.rand_plan_case(7, n_nodes=30, pods_per_node=5, limit=0)
    if chain:                                    # the device chain's scope: no host ports, no extended resources
        p = case.table.pods
        p["port_conflict"] = p["port_use"] = p["req_scalar"] = p["tpu_scalar_mask"] = 0
        p["flags"] &= ~np.uint32(abi.CA_POD_HAS_SCALAR_KEYS | abi.CA_POD_HAS_NONTPU_SCALAR_KEYS)
    return case


@pytest.mark.parametrize("forked", [False, True], ids=["committed", "forked"])
@pytest.mark.parametrize("path", ["chain", "speculative"])
def test_after_plan_removals(path, forked, oracle, monkeypatch):
    if path == "speculative":
        monkeypatch.setenv("CASIM_PLAN_SPECULATIVE", "1")
    else:
        monkeypatch.delenv("CASIM_PLAN_SPECULATIVE", raising=False)
    case = _plan_case(path == "chain")
    g, o = native.Mirror(0), oracle.OracleState()
    dims = _dims(case.node_recs, case.table)
    for b in (g, o):
        case.load(b)
        if forked:
            b.fork()
    assert o.scope_blockers() == 0
    po, pg = case.plan(o), case.plan(g)
    assert g.plan_stats()["path"] == path
    assert np.array_equal(po.results, pg.results) and np.array_equal(po.moves, pg.moves) and len(pg.moves) > 0
    n_pods = len(case.table) + len(pg.moves)
    _check_both(g, o, n_pods, f"plan_removals {path}", dims)
    if forked:
        g.revert()
        o.revert()
        _check_both(g, o, n_pods, f"plan_removals {path} reverted", dims, _Fresh(case.load, len(case.table)))
    g.close()
