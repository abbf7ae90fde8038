"""ScaleUp after the run on sharded Estimate plans (csrc/multi.hip: resident runs of
ca_multi_estimate_plan and its readers option_sums / option_price_sums / fetch / fetch_group /
groups_missing_pods) against the CPU restatement's lists and against the one-device plan, on the
cases of tests/similargen.py and tests/pricegen.py and the inputs of tests/test_gpu_multi.py;
and ComputeBestExpansionOption / ComputeBalancedScaleUp with multi= against the same calls
without it.  The replicas are several mirrors on device 0, as in tests/test_gpu_multi.py: the
blocks, threads, the state protocol and the exchange of the required list through host memory
are the code that runs on several GPUs.  Every case is a small plan."""
import copy
import ctypes as C
import random

import numpy as np
import pytest

import pricegen as P
import similargen as S
from autoscaler_amd import abi, k8s, native
from autoscaler_amd import workloads as W
from autoscaler_amd.clustersnapshot import ClusterSnapshot, NodeInfo
from autoscaler_amd.estimator import ThresholdBasedEstimationLimiter
from autoscaler_amd.expander import (ChainStrategy, LeastWaste, MostPods, PriceBased, PricingError,
                                     SimpleNodeUnfitness, SimplePreferredNodeProvider)
from autoscaler_amd.k8s import OwnerReference, Quantity, Taint, Toleration
from autoscaler_amd.nodegroupset import BalancingNodeGroupSetProcessor, NodeGroup, filter_plan_groups_by_pods
from autoscaler_amd.predicatechecker import SchedulerBasedPredicateChecker
from autoscaler_amd.scaleup import BuildPodGroups, ComputeBalancedScaleUp, ComputeBestExpansionOption
from estgen import _encode_estimate, _estimate_inputs

pytestmark = pytest.mark.gpu

REPLICAS = (2, 3, 5)
KNOB = "CASIM_MISSING_SCRATCH"
ONE = 5                                  # mirrors[ONE]: the one-device plan's mirror


@pytest.fixture(scope="module")
def oracle_state(oracle_lib):
    st = oracle_lib.OracleState()
    yield st
    st.close()


@pytest.fixture(scope="module")
def mirrors():
    """Five replicas and the one-device mirror, all on device 0, empty between tests."""
    ms = [native.Mirror(0) for _ in range(6)]
    yield ms
    for m in ms:
        m.close()


class Case:
    """A generator's case, encoded once, with the oracle's output per max_nodes computed once and
    shared by every replica count."""

    def __init__(self, case, oracle_state):
        self.c = case
        self.enc = case.encode()
        self.o = oracle_state
        self._lists = {}

    def lists(self, max_nodes):
        if max_nodes not in self._lists:
            self._lists[max_nodes] = S.oracle_lists(self.o, self.enc, max_nodes)
        return self._lists[max_nodes]


@pytest.fixture(scope="module")
def sim_cases(oracle_state):
    return {c.name: Case(c, oracle_state) for c in S.all_cases()}


@pytest.fixture(scope="module")
def price_cases(oracle_state):
    return {c.name: Case(c, oracle_state) for c in P.all_cases()}


class Shard:
    """One Estimate input as a sharded plan over the first `replicas` mirrors and as a one-device
    plan on mirrors[ONE]."""

    def __init__(self, enc, mirrors, replicas, one=True):
        table, tm, off, idx = enc
        self.mm = native.Multi(mirrors[:replicas])
        self.plan = native.MultiEstimatePlan(self.mm, table, off, idx, tm)
        self.one = native.EstimatePlan(mirrors[ONE], table, off, idx, tm) if one else None
        st = self.plan.stats()
        self.bounds, self.blocks = st["block_first_group"], st["blocks"]

    def block_of(self, g):
        return int(np.searchsorted(self.bounds, g, side="right")) - 1

    def run(self, max_nodes, ro, last_index=0):
        d = self.plan.run(max_nodes, last_index, device_results=True)
        assert d.sched_pod is None and d.sched_node is None
        assert np.array_equal(ro.results, d.results) and ro.last_index == d.last_index
        if self.one is not None:
            s = self.one.run(max_nodes, last_index, device_results=True)
            assert np.array_equal(ro.results, s.results)
        return d

    def close(self):
        self.plan.close()
        if self.one is not None:
            self.one.close()
        self.mm.close()


@pytest.fixture
def shard(mirrors):
    made = []

    def make(enc, replicas, one=True):
        s = Shard(enc, mirrors, replicas, one)
        made.append(s)
        return s
    yield make
    for s in made:
        s.close()


def _status(fn, *a):
    with pytest.raises(native.CasimError) as e:
        fn(*a)
    return e.value.status


def assert_same_bits(got, want, what=""):
    """Raw bytes; where the reference is NaN only isnan is compared (as tests/test_gpu_price.py)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]), what


# -- 1. the similar-group filter -----------------------------------------------------------------
def check_missing(sh, lists, req, cands, place=None, what=""):
    """groups_missing_pods on the sharded plan against set membership over the oracle's lists and
    against the one-device plan; `place` collects where the bitmap rows lay."""
    want_n, want_first = S.expected(lists, req, cands)
    got_n, got_first = sh.plan.groups_missing_pods(req, cands)
    assert got_n.tolist() == want_n.tolist(), what
    assert got_first.tolist() == want_first.tolist(), what
    one_n, one_first = sh.one.groups_missing_pods(req, cands)
    assert got_n.tolist() == one_n.tolist() and got_first.tolist() == one_first.tolist(), what
    assert filter_plan_groups_by_pods(sh.plan, req, cands) == [g for g, n in zip(cands, want_n) if n == 0]
    rows = [c for c in cands if lists[req] and c != req and lists[c]]         # not answered by the lengths
    ex = sh.plan.export_stats()
    crossing = {sh.block_of(c) for c in rows} - {sh.block_of(req)}
    assert ex["importing_blocks"] == len(crossing), what
    assert ex["exported_bytes"] == (4 * len(lists[req]) if crossing else 0), what
    ms = sh.plan.reader_ms("missing")
    assert len(ms) == sh.blocks
    assert [d for d in range(sh.blocks) if ms[d] > 0] == sorted({sh.block_of(c) for c in rows}), what
    if place is not None:
        br = sh.block_of(req)
        for c in rows:
            bc = sh.block_of(c)
            place["other"] |= bc != br
            place["same"] |= bc == br
            place["back"] |= br != 0 and bc == 0
    return got_n, got_first


@pytest.mark.parametrize("replicas", REPLICAS)
def test_similar_group_filter_on_every_case(replicas, sim_cases, shard):
    """Every case of similargen at this replica count, each run of its limits, with the case's own
    required group and with a later group (`two` / `full`) as the required one, the candidates on
    both sides of it.  Over the cases a row must have lain in another block than the required
    group's, in the same block, and in block 0 with the required group further on: read from the
    plan's reported bounds."""
    place = {"other": False, "same": False, "back": False}
    for name, cs in sim_cases.items():
        sh = shard(cs.enc, replicas)
        assert sh.blocks == min(replicas, len(cs.c.groups))
        names = list(cs.c.candidates) + [cs.c.required]
        for lim in cs.c.limits:
            ro, lists = cs.lists(lim)
            sh.run(lim, ro)
            for required in [cs.c.required] + [k for k in ("two", "full") if k in cs.c.index]:
                check_missing(sh, lists, cs.c.g(required), [cs.c.g(k) for k in names], place,
                              (name, replicas, lim, required))
        sh.close()
    assert all(place.values()), place


def test_stale_tail(sim_cases, shard):
    """An unlimited run, then max_nodes = 2 on the same sharded plan: the blocks' buffers keep the
    first run's ids behind n_scheduled, among them the very pods `ten` now lacks."""
    cs = sim_cases["stale"]
    sh = shard(cs.enc, 3)
    names = [cs.c.g(k) for k in cs.c.candidates]
    for lim in (0, S.STALE_LIMIT):
        ro, lists = cs.lists(lim)
        sh.run(lim, ro)
        got_n, got_first = check_missing(sh, lists, cs.c.g("req"), names)
    by = dict(zip(cs.c.candidates, zip(got_n.tolist(), got_first.tolist())))
    assert by["ten"] == (200, 20) and by["same"] == (0, -1) and by["minus0"] == (1, 0)
    full = sh.plan.fetch()
    off = cs.enc[2]
    a, n = int(off[cs.c.g("ten")]), len(lists[cs.c.g("ten")])
    assert n == 20 and (full[a + n:int(off[cs.c.g("ten") + 1])] == -1).all()      # the stale ids are not reported


@pytest.mark.parametrize("replicas", REPLICAS)
def test_batches_and_codes(replicas, sim_cases, shard, monkeypatch):
    """The bitmap rows of every block bounded to one and to two rows a batch: identical results;
    below one row CA_ECAPACITY.  Bad indices and NULL outputs: CA_EINVAL; NULL first_missing is
    allowed."""
    cs = sim_cases["word-95"]
    sh = shard(cs.enc, replicas)
    ro, lists = cs.lists(0)
    sh.run(0, ro)
    req, full = cs.c.g("req"), cs.c.g("full")
    cands = [cs.c.g(k) for k in cs.c.candidates]
    base = check_missing(sh, lists, req, cands)
    row_bytes = 4 * ((95 + 31) // 32)
    for rows in (1, 2):
        monkeypatch.setenv(KNOB, str(rows * row_bytes))
        got = check_missing(sh, lists, req, cands)
        assert got[0].tolist() == base[0].tolist() and got[1].tolist() == base[1].tolist()
    monkeypatch.setenv(KNOB, str(row_bytes - 1))
    assert _status(sh.plan.groups_missing_pods, req, [full]) == abi.CA_ECAPACITY
    monkeypatch.delenv(KNOB)
    check_missing(sh, lists, req, cands)
    G = sh.plan.G
    for bad_req, bad_groups in ((-1, [full]), (G, [full]), (req, [full, -1]), (req, [G])):
        assert _status(sh.plan.groups_missing_pods, bad_req, bad_groups) == abi.CA_EINVAL
    call = sh.plan.lib.ca_multi_estimate_plan_groups_missing_pods
    one, out = np.array([cs.c.g("id0")], np.int32), np.zeros(1, np.int32)
    assert call(sh.plan.h, req, one.ctypes.data, 1, out.ctypes.data, None) == abi.CA_OK and out[0] == 1
    assert call(sh.plan.h, req, one.ctypes.data, 1, None, None) == abi.CA_EINVAL
    assert call(sh.plan.h, req, None, 1, out.ctypes.data, None) == abi.CA_EINVAL
    assert call(None, req, one.ctypes.data, 1, out.ctypes.data, None) == abi.CA_EINVAL
    n, f = sh.plan.groups_missing_pods(req, [])
    assert len(n) == 0 and len(f) == 0 and not sh.plan.reader_ms("missing").any()
    with pytest.raises(ValueError):
        sh.plan.reader_ms(3)


# -- 2. a prefix cut across blocks ---------------------------------------------------------------
def test_prefix_cut_across_blocks(sim_cases, shard):
    """`cut` (CA_EUNSUPPORTED) in a block that is not the last: every group of the later blocks is
    CA_ENOTRUN although its block ran on its device.  Such a group has no sum, no price, no list;
    as a candidate it misses everything, as the required group everything fits."""
    cs = sim_cases["prefix"]
    cut, G = cs.c.g("cut"), len(cs.c.groups)
    sh = None
    for replicas in (5, 3, 2, 4):
        sh = shard(cs.enc, replicas)
        if sh.block_of(cut) < sh.blocks - 1:
            break
    assert sh.block_of(cut) < sh.blocks - 1, sh.bounds
    behind = list(range(sh.bounds[sh.block_of(cut) + 1], G))
    assert cs.c.g("after") in behind and sh.block_of(cs.c.g("after")) > sh.block_of(cut)
    ro, lists = cs.lists(0)
    out = sh.run(0, ro)
    st = out.results["status"].tolist()
    assert st[cut] == abi.CA_EUNSUPPORTED and all(st[g] == abi.CA_ENOTRUN for g in behind)
    cpu, mem = sh.plan.option_sums()
    price = P.random_prices(random.Random(11), len(cs.c.pods))
    tot = sh.plan.option_price_sums(price)
    table = cs.enc[0]
    for g in range(G):
        ids = np.array(lists[g], np.int64)
        assert cpu[g] == table.pods["score_milli_cpu"][ids].sum(dtype=np.int64)
        assert mem[g] == table.pods["score_memory"][ids].sum(dtype=np.int64)
        assert sh.plan.fetch_group(g).tolist() == lists[g]
    assert_same_bits(tot, P.expected(price, lists))
    for g in behind + [cut]:
        assert cpu[g] == 0 and mem[g] == 0 and tot[g:g + 1].tobytes() == np.float64(0.0).tobytes()
        assert len(sh.plan.fetch_group(g)) == 0
    assert all(x == 0 for x in sh.plan.reader_ms("sums")[sh.block_of(cut) + 1:])
    assert all(x == 0 for x in sh.plan.reader_ms("price")[sh.block_of(cut) + 1:])
    every = list(range(G))
    got_n, got_first = check_missing(sh, lists, cs.c.g("req"), every)
    for g in behind + [cut]:
        assert (got_n[g], got_first[g]) == (10, 0)
    for g in behind + [cut]:
        n, f = check_missing(sh, lists, g, every)
        assert not n.any() and (f == -1).all()
        assert not sh.plan.reader_ms("missing").any()
    full = sh.plan.fetch()
    off = cs.enc[2]
    assert (full[int(off[cut]):] == -1).all()


# -- 3. price sums ------------------------------------------------------------------------------
@pytest.mark.parametrize("replicas", REPLICAS)
def test_price_sums_on_every_case(replicas, price_cases, shard):
    """Every case of pricegen, each run of its limits: the totals in raw bytes against the in-order
    Python sums over the oracle's lists and against the one-device plan, the planted NaN / inf /
    subnormal / -0.0 lists among them; a second price table on the same run; a wrong n_prices."""
    for name, cs in price_cases.items():
        sh = shard(cs.enc, replicas)
        price = cs.c.price
        other = P.random_prices(random.Random(7), len(price))
        for lim in cs.c.limits:
            ro, lists = cs.lists(lim)
            sh.run(lim, ro)
            for table in (price, other, price):
                got = sh.plan.option_price_sums(table)
                assert_same_bits(got, P.expected(table, lists), (name, replicas, lim))
                assert_same_bits(got, sh.one.option_price_sums(table), (name, replicas, lim))
            assert len(sh.plan.reader_ms("price")) == sh.blocks
        for bad in (price[:-1], np.concatenate([price, [1.0]]), np.zeros(0)):
            assert _status(sh.plan.option_price_sums, bad) == abi.CA_EINVAL
        sh.close()


def test_planted_specials(price_cases, shard):
    """The known answers of the planted prices, on a sharded plan."""
    cs = price_cases["specials"]
    sh = shard(cs.enc, 3, one=False)
    ro, _ = cs.lists(0)
    sh.run(0, ro)
    got, g = sh.plan.option_price_sums(cs.c.price), cs.c.index
    tiny = np.finfo(np.float64).tiny
    assert 0.0 < got[g["subnormal"]] < tiny
    assert got[g["negzero"]] == 0.0 and not np.signbit(got[g["negzero"]])
    assert np.isfinite(got[g["big"]]) and got[g["overflow"]] == np.inf and got[g["pinf"]] == np.inf
    assert np.isnan(got[g["infnan"]]) and np.isnan(got[g["nan"]]) and np.isfinite(got[g["plain"]])


# -- 4. option sums under re-run and re-base -----------------------------------------------------
def test_option_sums_under_rerun_and_rebase(oracle_lib, mirrors):
    """The inputs of test_gpu_multi.test_multi_estimate_random (random clusters whose blocks'
    lastIndex dependence varies), run resident twice: results and lastIndex are the oracle's, the
    sums are the numpy sums over the oracle's lists and fetch() holds those lists.  Both a run
    with re-run blocks and one whose blocks were only re-based must occur."""
    saw_rerun = saw_rebase_only = False
    for seed in range(6):
        rng, nodes, pods, templates, groups = _estimate_inputs(seed, n_groups=9, n_pods=70)
        table, node_recs, tm, off, pod_idx = _encode_estimate(nodes, pods, templates, groups)
        max_nodes = [0, 1, 3, 40][seed % 4]
        L0 = [0, 3, 11][seed % 3]
        o = oracle_lib.OracleState()
        if len(node_recs):
            o.add_nodes(node_recs)
        ro = o.estimate(table, off, pod_idx, tm, max_nodes, L0)
        o.close()
        G = len(tm)
        lists, cpu, mem = [], np.zeros(G, np.int64), np.zeros(G, np.int64)
        for g in range(G):
            ok = int(ro.results[g]["status"]) == abi.CA_OK
            a, n = int(off[g]), int(ro.results[g]["n_scheduled"]) if ok else 0
            ids = ro.sched_pod[a:a + n]
            lists.append(ids)
            cpu[g] = table.pods["score_milli_cpu"][ids].sum(dtype=np.int64)
            mem[g] = table.pods["score_memory"][ids].sum(dtype=np.int64)
        try:
            for m in mirrors[:5]:
                m.clear()
                if len(node_recs):
                    m.add_nodes(node_recs)
            for replicas in REPLICAS:
                sh = Shard((table, tm, off, pod_idx), mirrors, replicas, one=False)
                try:
                    for _ in range(2):
                        sh.run(max_nodes, ro, L0)
                        got_cpu, got_mem = sh.plan.option_sums()
                        assert got_cpu.tolist() == cpu.tolist() and got_mem.tolist() == mem.tolist(), (seed, replicas)
                        full = sh.plan.fetch()
                        for g in range(G):
                            a, n, e = int(off[g]), len(lists[g]), int(off[g + 1])
                            assert np.array_equal(full[a:a + n], lists[g]), (seed, replicas, g)
                            assert (full[a + n:e] == -1).all()
                            assert np.array_equal(sh.plan.fetch_group(g), lists[g])
                    st = sh.plan.stats()
                    saw_rerun |= st["reruns"] > 0
                    saw_rebase_only |= st["reruns"] == 0 and st["blocks"] > 1
                finally:
                    sh.close()
        finally:
            for m in mirrors[:5]:
                m.clear()
    assert saw_rerun and saw_rebase_only


# -- 5. state -----------------------------------------------------------------------------------
def test_state(sim_cases, shard, mirrors):
    """The readers work after a resident run that returned CA_OK and only then: the caller decides
    by the argument."""
    cs = sim_cases["word-64"]
    sh = shard(cs.enc, 3, one=False)
    p = sh.plan
    req, full = cs.c.g("req"), cs.c.g("full")
    price = np.ones(len(cs.c.pods))
    readers = [(p.option_sums,), (p.option_price_sums, price), (p.fetch,), (p.fetch_group, req),
               (p.groups_missing_pods, req, [full])]
    for r in readers:                                             # before any run
        assert _status(*r) == abi.CA_ESTATE
    ro, lists = cs.lists(0)
    host = p.run(0, 0)                                            # a host-list run
    assert np.array_equal(host.results, ro.results) and host.sched_pod is not None
    for r in readers:
        assert _status(*r) == abi.CA_ESTATE
    sh.run(0, ro)                                                 # a resident run
    for r in readers:
        r[0](*r[1:])
    assert p.fetch_group(req).tolist() == lists[req]
    p.run(0, 0, want_nodes=False)
    assert _status(p.option_sums) == abi.CA_ESTATE
    sh.run(0, ro)
    assert p.groups_missing_pods(req, [full])[0].tolist() == [0]
    # sched_node without sched_pod
    lim, li = abi.LimiterC(0, 0), C.c_int32(0)
    nodes = np.zeros(max(p.total, 1), np.int32)
    st = p.lib.ca_multi_estimate_plan_run(p.h, C.byref(lim), C.byref(li), p.results.ctypes.data, None, nodes.ctypes.data)
    assert st == abi.CA_EINVAL
    assert _status(p.option_sums) == abi.CA_ESTATE                 # (and that call was no resident run)
    # out-of-range and short arguments
    sh.run(0, ro)
    assert _status(p.fetch_group, -1) == abi.CA_EINVAL and _status(p.fetch_group, p.G) == abi.CA_EINVAL
    n = C.c_int32(0)
    buf = np.zeros(4, np.int32)
    assert p.lib.ca_multi_estimate_plan_fetch_group(p.h, req, buf.ctypes.data, 4, C.byref(n)) == abi.CA_ECAPACITY
    assert n.value == len(lists[req]) and not buf.any()
    assert p.lib.ca_multi_estimate_plan_option_sums(p.h, None, None) == abi.CA_EINVAL
    ms = np.zeros(8, np.float32)
    assert p.lib.ca_multi_estimate_plan_reader_ms(p.h, 7, ms.ctypes.data, 8) == abi.CA_EINVAL
    # no groups at all: CA_OK without launches
    table = cs.enc[0]
    with native.Multi(mirrors[:2]) as mm, \
            native.MultiEstimatePlan(mm, table, np.zeros(1, np.int32), np.zeros(0, np.int32),
                                     np.zeros(0, abi.TEMPLATE_DTYPE)) as empty:
        assert _status(empty.option_sums) == abi.CA_ESTATE
        out = empty.run(0, 4, device_results=True)
        assert out.last_index == 4 and len(out.results) == 0
        cpu, mem = empty.option_sums()
        assert len(cpu) == 0 and len(mem) == 0
        assert len(empty.option_price_sums(np.ones(len(table)))) == 0
        assert len(empty.fetch()) == 0
        assert _status(empty.fetch_group, 0) == abi.CA_EINVAL
        assert not empty.reader_ms("sums").any() and not empty.reader_ms("price").any()


# -- 6. one C2-shaped pass ----------------------------------------------------------------------
def test_c2_pass(mirrors):
    """A C2-shaped batch (one pod table shared by all groups) over 4 replicas against one mirror:
    sums, price bytes, the least-waste winner and filterNodeGroupsByPods of the winner."""
    w = W.c2(n_pods=12000, n_groups=24, n_existing=200)
    try:
        for m in mirrors[:4] + [mirrors[ONE]]:
            W.load_estimate(m, w)
        sh = Shard((w.table, w.templates, w.group_off, w.pod_idx), mirrors, 4)
        try:
            d = sh.plan.run(w.max_nodes, 5, device_results=True)
            s = sh.one.run(w.max_nodes, 5, device_results=True)
            assert np.array_equal(d.results, s.results) and d.last_index == s.last_index
            assert sh.blocks == 4
            cpu, mem = sh.plan.option_sums()
            one_cpu, one_mem = sh.one.option_sums()
            assert cpu.tolist() == one_cpu.tolist() and mem.tolist() == one_mem.tolist() and cpu.any()
            price = P.random_prices(random.Random(2), len(w.table))
            assert sh.plan.option_price_sums(price).tobytes() == sh.one.option_price_sums(price).tobytes()
            cap_cpu = np.ascontiguousarray(w.templates["node"]["alloc_milli_cpu"], dtype=np.int64)
            cap_mem = np.ascontiguousarray(w.templates["node"]["alloc_memory"], dtype=np.int64)
            every = np.arange(sh.plan.G, dtype=np.int32)
            valid = every[(d.results["n_scheduled"] > 0) & (d.results["node_count"] > 0)]
            LW = abi.CA_EXPANDER_LEAST_WASTE
            best = native.expander_best_options(LW, d.results, cpu, mem, cap_cpu, cap_mem, valid)[0]
            want = native.expander_best_options(LW, s.results, one_cpu, one_mem, cap_cpu, cap_mem, valid)[0]
            assert best.tolist() == want.tolist() and len(best) >= 1
            win = int(best[0])
            assert np.array_equal(sh.plan.fetch_group(win), sh.one.fetch_group(win))
            got, ref = sh.plan.groups_missing_pods(win, every), sh.one.groups_missing_pods(win, every)
            assert got[0].tolist() == ref[0].tolist() and got[1].tolist() == ref[1].tolist()
            ex = sh.plan.export_stats()
            others = {sh.block_of(int(g)) for g in valid} - {sh.block_of(win)}
            assert len(others) >= 1 and ex["importing_blocks"] == len(others)
            assert ex["exported_bytes"] == 4 * int(d.results[win]["n_scheduled"])
        finally:
            sh.close()
    finally:
        for m in mirrors:
            m.clear()


# -- 7. the facade ------------------------------------------------------------------------------
class _First:
    def BestOption(self, options, node_infos):  # noqa: N802
        return options[0] if options else None


class _Recording(BalancingNodeGroupSetProcessor):
    """Records the groups the scale-up is balanced between ([best] + kept)."""

    def BalanceScaleUpBetweenGroups(self, groups, new_nodes):  # noqa: N802
        self.balanced = ([g.Id() for g in groups], new_nodes)
        return super().BalanceScaleUpBetweenGroups(groups, new_nodes)


def _zones_inputs():
    """tests/test_gpu_similar.py: three similar zones, zone c's template has a taint the `web` pods
    do not tolerate; the other shape is not similar."""
    pods = []
    for i in range(12):
        p = k8s.build_test_pod(f"job{i}", 500, S.GI)
        p.owner_refs = [OwnerReference("ReplicaSet", "job", "job")]
        p.tolerations.append(Toleration(key="dedicated", operator="Exists"))
        pods.append(p)
    for i in range(8):
        p = k8s.build_test_pod(f"web{i}", 300, S.GI)
        p.owner_refs = [OwnerReference("ReplicaSet", "web", "web")]
        pods.append(p)
    groups = []
    for zone, size in (("a", 1), ("b", 3), ("c", 0)):
        n = k8s.build_test_node(f"t-{zone}", 4000, 8 * S.GI, 110)
        n.labels.update({"topology.kubernetes.io/zone": zone, "pool": "std"})
        if zone == "c":
            n.taints.append(Taint("dedicated", "x", "NoSchedule"))
        groups.append((NodeGroup(f"ng-{zone}", size, 10), NodeInfo(n, [])))
    big = k8s.build_test_node("t-big", 32000, 128 * S.GI, 110)
    big.labels.update({"topology.kubernetes.io/zone": "a", "pool": "std"})
    groups.append((NodeGroup("ng-big", 1, 10), NodeInfo(big, [])))
    return [], pods, groups


def _balance_groups_inputs():
    """tests/test_gpu_similar.py: TestScaleUpBalanceGroups (orchestrator_test.go:763-837)."""
    cfg = {"ng1": (1, 1, 1), "ng2": (1, 2, 1), "ng3": (1, 5, 1), "ng4": (1, 5, 3)}
    nodes, groups = [], []
    for gid, (mn, mx, size) in cfg.items():
        for i in range(size):
            nodes.append((k8s.build_test_node(f"{gid}-node-{i}", 100, 1000),
                          [k8s.build_scheduled_test_pod(f"{gid}-pod-{i}", 80, 0, f"{gid}-node-{i}")]))
        if size < mx:
            groups.append((NodeGroup(gid, size, mx, mn), NodeInfo(k8s.build_test_node(f"{gid}-template", 100, 1000), [])))
    pods = [k8s.build_test_pod(f"test-pod-{i}", 80, 0) for i in range(2)]
    return nodes, pods, groups


class LinearPricing:
    """tests/test_gpu_price.py: a pricing model linear in the requests, with a per-name factor so
    that sums round; pods whose name hashes to `fail_mod` have no price."""

    def __init__(self, fail_mod=0):
        self.fail_mod = fail_mod

    @staticmethod
    def _h(name):
        import zlib
        return zlib.crc32(name.encode())

    def NodePrice(self, node, start, end):  # noqa: N802
        cap = node.get_capacity()
        cpu, mem = Quantity(cap.get("cpu", 0)).milli_value(), Quantity(cap.get("memory", 0)).value()
        return (cpu * 0.031 + mem / (1 << 30) * 0.0042) * (1.0 + (self._h(node.name) % 9) / 64.0)

    def PodPrice(self, pod, start, end):  # noqa: N802
        if self.fail_mod and self._h(pod.name) % self.fail_mod == 0:
            raise PricingError(f"no price for {pod.name}")
        cpu = mem = 0
        for ct in pod.containers:
            cpu += Quantity(ct.requests.get("cpu", 0)).milli_value()
            mem += Quantity(ct.requests.get("memory", 0)).value()
        return (cpu * 0.0317 + mem / (1 << 30) * 0.00425) * (1.0 + (self._h(pod.name) % 1000) / 7919.0)


class _Lister:
    def __init__(self, n):
        self.n = n

    def List(self):  # noqa: N802
        return [None] * self.n


def _options_inputs(seed):
    """tests/test_gpu_price.py: a random cluster, pods of a few controllers with twins."""
    rng, nodes, pods, templates, _ = _estimate_inputs(seed, n_groups=10, n_pods=90)
    for i, p in enumerate(pods):
        if rng.random() < 0.7:
            p.owner_refs = [OwnerReference("ReplicaSet", f"rs{i % 5}", f"rs{i % 5}")]
    extra = []
    for p in pods[:30]:
        if p.owner_refs:
            q = copy.deepcopy(p)
            q.name = p.name + "-twin"
            extra.append(q)
    pods = pods + extra
    random.Random(seed).shuffle(pods)
    infos = [(f"ng{g}", NodeInfo(t, list(ds))) for g, (t, ds) in enumerate(templates)]
    return [(n, []) for n in nodes], pods, infos


def _facade(make_inputs, call, extra_node):
    """call(snapshot, checker, pod groups, node groups, limiter, multi) -> something comparable, on
    two snapshots built alike: one without multi, one with a Multi of its backend and two more
    mirrors.  Twice, with `extra_node` added to both snapshots in between; then once more on the
    unchanged snapshot, which must reload no replica."""
    sides = []
    for sharded in (False, True):
        nodes, pods, node_groups = make_inputs()
        snap = ClusterSnapshot(native.Mirror(0))
        for node, scheduled in nodes:
            snap.AddNodeWithPods(node, scheduled)
        extra = [native.Mirror(0), native.Mirror(0)] if sharded else []
        multi = native.Multi([snap.backend] + extra) if sharded else None
        sides.append((snap, pods, node_groups, multi, extra))
    res = [[], []]
    for step in range(3):
        for k, (snap, pods, node_groups, multi, _) in enumerate(sides):
            pc = SchedulerBasedPredicateChecker()
            pc.last_index = step
            lim = ThresholdBasedEstimationLimiter(max_nodes=0 if step != 1 else 7)
            loads = snap.replica_loads
            res[k].append((call(snap, pc, BuildPodGroups(pods), node_groups, lim, multi), pc.last_index, pc.evals))
            if multi is not None:
                # the first call loads both replicas, the call after AddNode reloads them (the
                # stamp moved), the call on the unchanged snapshot loads nothing
                assert snap.replica_loads - loads == (2, 2, 0)[step], step
        if step == 0:
            for snap, *_ in sides:
                snap.AddNode(copy.deepcopy(extra_node))
    for snap, _, _, multi, extra in sides:
        if multi is not None:
            multi.close()
        for m in extra + [snap.backend]:
            m.close()
    assert res[0] == res[1]
    return res[1]


def _balanced(chain_of):
    def call(snap, pc, pod_groups, node_groups, lim, multi):
        proc = _Recording()
        kw = {} if multi is None else {"multi": multi}
        best, plan, feas = ComputeBalancedScaleUp(snap, pc, pod_groups, node_groups, lim, chain_of(), proc, **kw)
        return ((best.node_group.Id(), best.node_count, [p.name for p in best.pods]), proc.balanced,
                [(i.Group.Id(), i.CurrentSize, i.NewSize, i.MaxSize) for i in plan], feas.tobytes())
    return call


def _best(chain_of):
    def call(snap, pc, pod_groups, node_groups, lim, multi):
        kw = {} if multi is None else {"multi": multi}
        best, feas = ComputeBestExpansionOption(snap, pc, pod_groups, node_groups, lim, chain_of(), **kw)
        return (None if best is None else (best.node_group, best.node_count, [p.name for p in best.pods]),
                feas.tobytes())
    return call


def test_balanced_scale_up_zones_over_replicas():
    res = _facade(_zones_inputs, _balanced(lambda: ChainStrategy([LeastWaste(), MostPods()], _First())),
                  k8s.build_test_node("late-node", 2000, 4 * S.GI, 110))
    best, balanced, *_ = res[0][0]
    assert best[0] == "ng-a" and len(best[2]) == 20 and balanced[0] == ["ng-a", "ng-b"]


def test_balanced_scale_up_balance_groups_over_replicas():
    res = _facade(_balance_groups_inputs, _balanced(lambda: ChainStrategy([LeastWaste(), MostPods()], _First())),
                  k8s.build_test_node("late-node", 10, 1000))
    best, balanced, plan, _ = res[0][0]
    assert best[1] == 2 and sorted(balanced[0]) == ["ng2", "ng3", "ng4"]
    assert {g: n for g, _, n, _ in plan} == {"ng2": 2, "ng3": 2}


@pytest.mark.parametrize("chain", ["least-waste", "price"])
@pytest.mark.parametrize("seed", [1, 2])
def test_best_expansion_option_over_replicas(seed, chain):
    def chain_of():
        if chain == "least-waste":
            return ChainStrategy([LeastWaste()], _First())
        return ChainStrategy([PriceBased(LinearPricing(fail_mod=29 if seed % 3 == 2 else 0),
                                         SimplePreferredNodeProvider(_Lister(3 * seed)), SimpleNodeUnfitness)], _First())
    res = _facade(lambda: _options_inputs(seed), _best(chain_of), k8s.build_test_node("late-node", 3000, 8 * S.GI, 110))
    assert any(r[0][0] is not None for r in res)
