"""The planted filter cases of tests/filtgen.py on the CPU: the oracle's loop
(or_filter_out_schedulable) equals the step-by-step reference of tests/tspgen.py
(check_predicates / fits_any_node / add_pods) on every one of them, and every case holds
what its `claims` say, from numpy and the oracle's output alone.
tests/test_gpu_filter_cases.py then compares both kernels of csrc/filter.hip with the
oracle on the same cases."""
from __future__ import annotations

import numpy as np
import pytest

import filtgen as G
import tspgen as T
from autoscaler_amd import abi

CASES = G.all_cases()


@pytest.fixture(scope="module")
def outputs(oracle_lib):
    """name -> the oracle's FilterOutSchedulable output (each case is run once)."""
    memo = {}

    def get(name):
        if name not in memo:
            case = CASES[name]
            o = oracle_lib.OracleState()
            case.load(o)
            memo[name] = case.filter(o)
            o.close()
        return memo[name]
    return get


def node_states(b, n):
    return [(b.node_pods(i), b.node_state(i)) for i in range(n)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_steps(name, oracle_lib, outputs):
    """(No case needs cutting down: the slowest, the LDS pair on 18 752 and 18 753 nodes, takes
    well under a second on either side.)"""
    case = CASES[name]
    a, b = oracle_lib.OracleState(), oracle_lib.OracleState()
    case.load(a)
    case.load(b)
    got = case.filter(a)
    want = T.try_schedule_ref(b, case.pending, case.order, None, False, case.class_owner, case.hints, case.L0)
    assert np.array_equal(got.node, want.node), np.nonzero(got.node != want.node)[0][:10]
    assert np.array_equal(got.pod_id, want.pod_id)
    assert np.array_equal(got.hints, want.hints)
    assert (got.placed, got.last_index, got.evals, got.n_overflowing) == \
           (want.placed, want.last_index, want.evals, want.n_overflowing)
    assert want.tried == len(case.order)
    n = len(case.nodes)
    step = max(1, n // 300)                         # every node of the small rings, a comb of the long ones
    for i in list(range(0, n, step)) + [int(x) for x in got.node if x >= 0]:
        assert (a.node_pods(i), a.node_state(i)) == (b.node_pods(i), b.node_state(i)), i
    first = outputs(name)
    assert np.array_equal(first.node, got.node) and first.evals == got.evals      # deterministic
    a.close()
    b.close()


# ---------------------------------------------------------------------------
# the claims
# ---------------------------------------------------------------------------
def walk(case, out):
    """Per position: (L when the pod's turn comes, placed by a scan).  A pod sits on its
    hinted node only through the hint check, so every other placement is a scan's and moves
    lastIndex behind its node."""
    n = len(case.nodes)
    L = case.L0 % n if n else 0
    rows = []
    for k, x in enumerate(out.node.tolist()):
        scan = x >= 0 and x != int(case.hints[k])
        rows.append((L, scan))
        if scan:
            L = (x + 1) % n
    return rows


def check_lds(case, cl):
    rt = G.route(case)
    if "static_classes" in cl:
        assert (rt["path"], rt["static_classes"], rt["static_in_lds"]) == ("bitmap", cl["static_classes"],
                                                                          cl["static_in_lds"]), rt
    if "spill" in cl:                               # with the static words one word count too many, without: fits
        S, nw, K = cl["spill"]
        assert G.fb_lds(S, nw - 1, K, True, 0, 0, False) <= G.FB_LDS_MAX < G.fb_lds(S, nw, K, True, 0, 0, False)
        assert G.fb_lds(S, nw, K, False, 0, 0, False) <= G.FB_LDS_MAX and G.words(len(case.nodes)) == nw
    if "pair" in cl:                                # the ring sizes either side of 160 KiB
        S, nw = cl["pair"]
        assert G.fb_lds(S, nw, 0, False, 0, 0, False) <= G.FB_LDS_MAX < G.fb_lds(S, nw + 1, 0, False, 0, 0, False)
        assert len(case.nodes) == 64 * nw + (1 if cl["over"] else 0)
        assert rt["path"] == ("window" if cl["over"] else "bitmap")
        assert G.shapes_of(case) == (S, 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_holds_its_claims(name, outputs):
    case = CASES[name]
    out = outputs(name)
    cl = case.claims
    assert cl, f"{name}: a case without claims"
    n = len(case.nodes)
    rows = walk(case, out)
    known = {"placed", "last_index", "wraps", "keeps_last_index", "nodes", "evals", "overflowing", "on_node",
             "hint_in_window", "shapes", "tried", "lds", "route"}
    assert set(cl) <= known, set(cl) - known
    if case.match is None:
        assert set(cl) - {"route"}, f"{name}: only a route claim"
    own = case.match is not None                    # placed / tried of the case's own call: test_own_call
    if "placed" in cl and not own:
        assert out.placed == cl["placed"] == int((out.node >= 0).sum()), out.placed
    if "last_index" in cl:
        assert out.last_index == cl["last_index"], out.last_index
    if cl.get("keeps_last_index"):
        assert out.last_index == case.L0 and not any(s for _, s in rows)
    if "wraps" in cl:
        prev, wrapped = (case.L0 % n), False
        for (_, scan), x in zip(rows, out.node.tolist()):
            if scan:
                wrapped |= x < prev
                prev = x
        assert wrapped == cl["wraps"]
    for k, x in cl.get("nodes", {}).items():
        assert out.node[k] == x, (k, int(out.node[k]), x)
    if "evals" in cl:
        assert out.evals == cl["evals"], out.evals
    if "overflowing" in cl:
        assert out.n_overflowing == cl["overflowing"]
    if "on_node" in cl:
        x, m, k = cl["on_node"]
        hinted = case.hints == x
        assert int(hinted.sum()) == m and int((out.node[hinted] == x).sum()) == k, (int(hinted.sum()),
                                                                                   int((out.node[hinted] == x).sum()))
    for k, inside in cl.get("hint_in_window", {}).items():
        h = int(case.hints[k])
        assert 0 <= h < n and ((h - rows[k][0]) % (64 * G.words(n)) < 64) == inside, (k, h, rows[k][0])
    if "shapes" in cl:
        assert G.shapes_of(case) == cl["shapes"], G.shapes_of(case)
    if "lds" in cl:
        check_lds(case, cl["lds"])
    # what holds for every case: unschedulable nodes only through a tolerated hint, hints set for the
    # placed pods and kept for the others, no row overdrawn
    unsched = (case.nodes["flags"] & abi.CA_NODE_UNSCHEDULABLE) != 0
    p = case.pending.pods[case.order]
    for k, x in enumerate(out.node.tolist()):
        if x >= 0 and unsched[x]:
            assert case.hints[k] == x and int(p[k]["flags"]) & abi.CA_POD_TOLERATES_UNSCHED, k
        assert out.hints[k] == (x if x >= 0 else case.hints[k]), k
    free = case.free_rows()
    for k, x in enumerate(out.node.tolist()):
        if x >= 0:
            free[x] -= [int(p[k]["req_milli_cpu"]), int(p[k]["req_memory"]), int(p[k]["req_ephemeral"]), 1]
    assert (free >= 0).all()


@pytest.mark.parametrize("name", sorted(c for c in CASES if CASES[c].match is not None))
def test_own_call(name, oracle_lib):
    """The planted breaks: the case's own match with break-on-failure stops where it says."""
    case = CASES[name]
    o = oracle_lib.OracleState()
    case.load(o)
    ref = T.try_schedule_ref(o, case.pending, case.order, case.match, case.brk, case.class_owner, case.hints, case.L0)
    o.close()
    assert (ref.tried, ref.placed) == (case.claims["tried"], case.claims["placed"]), (ref.tried, ref.placed)
    assert ref.tried < len(case.order) and ref.node[ref.tried - 1] == -1 and (ref.node[ref.tried:] == -1).all()
    if "hinted-outside-mask" in name:
        assert ref.hint_ok[0] == 1 and not T.match_pos(case.match, int(case.hints[0]))


def test_route_restatement():
    """route(): the fall-backs by content, by shape count and by LDS, and the masks' extra words."""
    want = {"content/port": "window", "content/scalar": "window", "content/names": "window",
            "shapes/live65-dead0": "window", "shapes/collected-1030": "window", "shapes/live64-dead3": "bitmap",
            "static/lds-pair-fits": "bitmap", "static/lds-pair-over": "window", "static/spilled": "bitmap",
            "mixed/f25-n100-L70": "bitmap"}
    for name, path in want.items():
        assert G.route(CASES[name])["path"] == path, name
    assert G.route(CASES["shapes/live64-dead3"])["shapes"] == 65
    assert G.route(CASES["shapes/all-dead"])["shapes"] == 1
    assert G.route(CASES["static/lds-pair-fits"], masked=True)["path"] == "window"      # vis and svis apart
    assert G.route(CASES["mixed/f25-n100-L70"], forced_window=True)["path"] == "window"


def test_case_shapes_and_families():
    """Every family has cases; only the named long rings are long; the ring sizes, lastIndex
    values, run lengths and window sizes of the list are all present; each of the four
    dimensions binds somewhere, the all-zero shape and one-slot rows exist."""
    fam = {f: [c for c in CASES.values() if c.family == f] for f in G.FAMILIES}
    assert all(fam.values()) and sum(map(len, fam.values())) == len(CASES)
    long_rings = {n for n, c in CASES.items() if len(c.nodes) > 600}
    for name, case in CASES.items():
        assert len(case.order) < 300 or name == "shapes/collected-1030", name
    assert all(n.startswith(("single/", "static/spilled", "static/lds-pair", "window/n87")) for n in long_rings), long_rings
    for n in G.RING_SIZES:
        for L0 in (0, n - 1, n + 3):
            for kind in ("wrap", "end", "overfull", "nothing"):
                assert f"ring/{kind}-n{n}-L{L0}" in CASES
        assert any(0 < c.L0 < n - 1 and c.L0 & 63 for c in fam["ring"] if len(c.nodes) == n) or n == 1
    assert {len(c.order) for c in fam["ring"]} >= {0, 1, 63, 64, 65, 128, 129}
    assert {len(c.order) for c in fam["single"]} == {1, 2, 63, 64, 65, 130}
    assert {len(c.nodes) for c in fam["single"]} == {4096, 4160}
    assert {len(c.nodes) for c in fam["window"]} >= {511, 512, 513, 577, 8704, 8705}
    binds = set()
    zero = one_slot = False
    for case in CASES.values():
        if len(case.nodes) > 600:
            continue
        free, p = case.free_rows(), case.pending.pods[case.order]
        one_slot |= bool((free[:, 3] == 1).any())
        req = np.stack([p["req_milli_cpu"], p["req_memory"], p["req_ephemeral"], np.ones(len(p), np.int64)], axis=1)
        zero |= bool((req[:, :3] == 0).all(axis=1).any()) if len(p) else False
        for r in {tuple(x) for x in req.tolist()}:
            short = free < np.array(r)                   # [n][4]
            for d in range(4):
                if (short[:, d] & (short.sum(axis=1) == 1)).any():
                    binds.add(d)
    assert binds == {0, 1, 2, 3} and zero and one_slot
