"""GPU parity of ca_plan_removals on the planted cases of tests/chaingen.py (ring geometry,
block skipping, skylines, dirty bits, lists and copies, commit, staging, PDBs, the bulk step,
the chain's scope edges), pinned on the CPU by tests/test_chain_cases.py.

Every case runs on four paths, each against the oracle bit for bit: the device chain with 7
helper waves, the chain alone, the chain with every scan handed to the helpers after its
first block, and the speculative sweep windows.  The chain spin-waits on its helper waves:
run this file under a time limit of its own, and read a limit hit as a hang."""
from __future__ import annotations

import numpy as np
import pytest

import chaingen as G
from autoscaler_amd import abi, native
from conftest import gpu_available
from test_gpu_planner import _check, _follow_up_sweep

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="no HIP device")]

CASES = G.all_cases()
PATHS = {"chain": {"CASIM_PLAN_HELPERS": "7"}, "chain1": {"CASIM_PLAN_HELPERS": "0"},
         "help-after-1": {"CASIM_PLAN_HELPERS": "7", "CASIM_PLAN_HELP_AFTER": "1"},
         "speculative": {"CASIM_PLAN_SPECULATIVE": "1"}}
KNOBS = ("CASIM_PLAN_HELPERS", "CASIM_PLAN_HELP_AFTER", "CASIM_PLAN_SPECULATIVE")


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


@pytest.fixture(scope="module")
def mirror():
    m = native.Mirror(0)
    yield m
    m.close()


def set_path(monkeypatch, path: str, case=None) -> str:
    """The knobs of `path` (a case's own knobs first); returns the path the call must report.
    The "-helpers" cases carry CASIM_PLAN_HELP_AFTER=1 themselves, so that they exist as named
    cases: on path "chain" they repeat their base case on "help-after-1", and on "chain1" the
    knob has no helper wave to hand a scan to.  Both repeats are harmless."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**(case.env if case else {}), **PATHS[path]}.items():
        monkeypatch.setenv(k, v)
    return "speculative" if path == "speculative" or (case is not None and case.path == "speculative") else "chain"


_ORACLE = {}


def oracle_side(oracle, name):
    """The oracle's output, pod lists and follow-up sweep of a case: computed once, shared by
    the four paths, never changed."""
    if name not in _ORACLE:
        case = CASES[name]
        o = oracle.OracleState()
        _ORACLE[name] = run_on(o, case)
        o.close()
    return _ORACLE[name]


def run_on(b, case, follow_up=True):
    try:
        case.load(b)
        out = case.plan(b)
        n = len(case.node_recs)
        lists = [b.node_pods(i) for i in range(n)]
        sweep = _follow_up_sweep(b, n, len(case.table) + len(out.moves)) if follow_up else None
    except native.CasimError as e:
        if e.status == abi.CA_EDEVICE:          # nothing more on a device that faulted
            pytest.exit(f"device error in {case.name}: {e}", returncode=3)
        raise
    return out, lists, sweep


def same(want, got, what):
    (o, on, os_), (g, gn, gs) = want, got
    _check(o, g, what)
    assert on == gn, what
    if os_ is not None:
        assert np.array_equal(os_.results, gs.results) and np.array_equal(os_.dest, gs.dest), what
        assert np.array_equal(os_.hints, gs.hints) and os_.last_index == gs.last_index, what


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_case(name, path, oracle, mirror, monkeypatch):
    case = CASES[name]
    want_path = set_path(monkeypatch, path, case)
    want = oracle_side(oracle, name)
    got = run_on(mirror, case)
    assert mirror.plan_stats()["path"] == want_path, name
    same(want, got, (name, path))


TWICE = ("sky/revert", "staging/moves-1025-last-after-1024", "lists/hinted-groups/eph", "pdb/risky-then-negative",
         "staging/C200")


@pytest.mark.parametrize("name", TWICE)
def test_twice_on_one_mirror(name, oracle, mirror, monkeypatch):
    """The same case twice, and a smaller one between: the chain's scratch buffers and its
    published-move count are reused, nothing of an earlier call may show."""
    set_path(monkeypatch, "chain", CASES[name])
    want = oracle_side(oracle, name)
    same(want, run_on(mirror, CASES[name]), (name, "first"))
    small = "lists/copy-chain"
    same(oracle_side(oracle, small), run_on(mirror, CASES[small]), (small, "between"))
    same(want, run_on(mirror, CASES[name]), (name, "second"))
    assert mirror.plan_stats()["path"] == "chain"


@pytest.mark.parametrize("path", ["chain", "speculative"])
@pytest.mark.parametrize("name", ["sky/revert", "lists/100+28-copies", "bulk/back-off/eph"])
def test_fork_and_revert(name, path, oracle, mirror, monkeypatch):
    """The call inside a fork, then Revert: the snapshot is the loaded one again, and the same
    call on it gives the same answer."""
    case = CASES[name]
    set_path(monkeypatch, path, case)
    o = oracle.OracleState()
    n = len(case.node_recs)
    outs = []
    for b in (o, mirror):
        case.load(b)
        b.fork()
        out = case.plan(b)
        b.revert()
        outs.append((out, [b.node_pods(i) for i in range(n)], _follow_up_sweep(b, n, len(case.table) + len(out.moves))))
    same(outs[0], outs[1], (name, "forked"))
    assert len(outs[1][0].moves) > 0
    assert outs[1][1] == [[int(j) for j in np.nonzero(case.node_of == i)[0]] for i in range(n)]
    again = case.plan(mirror)
    shift = int(again.moves["new_pod"].min()) - int(outs[0][0].moves["new_pod"].min())
    assert shift >= 0                    # records stored inside the fork are detached, never reused
    again.moves["new_pod"] -= shift
    again.moves["pod"][again.moves["pod"] >= len(case.table)] -= shift          # copies moved again
    blocked = again.results["blocking_pod"] >= len(case.table)
    again.results["blocking_pod"][blocked] -= shift
    _check(outs[0][0], again, (name, "after the revert"))
    o.close()


# ---------------------------------------------------------------------------
# the LDS edge of the chain's scope
# ---------------------------------------------------------------------------
_EDGE = {}


def lds_edge(mirror, eph: bool) -> int:
    """The largest node count the chain takes, by bisection on the reported path."""
    if eph not in _EDGE:
        def on_chain(n):
            case = G.lds_edge_case(n, eph)
            case.load(mirror)
            case.plan(mirror)
            return mirror.plan_stats()["path"] == "chain"
        lo, hi = 200, 8192
        assert on_chain(lo) and not on_chain(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if on_chain(mid) else (lo, mid)
        _EDGE[eph] = lo
    return _EDGE[eph]


@pytest.mark.parametrize("eph", [False, True], ids=["no-eph", "eph"])
def test_lds_edge(eph, oracle, mirror, monkeypatch, capsys):
    """N (the largest ring in the chain's scope) and N + 1 with candidates in the first block,
    in the last block and on the last node: the rows of the last, partial block sit at the
    end of the LDS image."""
    set_path(monkeypatch, "chain")
    N = lds_edge(mirror, eph)
    with capsys.disabled():
        print(f"\n[lds edge] eph_cols={eph}: largest in-scope node count {N}")
    assert 4000 < N < 8192
    for n, path in ((N, "chain"), (N + 1, "speculative")):
        cands = list(dict.fromkeys([1, 63, (n - 1) & ~63, n - 1, n - 3]))
        case = G.lds_edge_case(n, eph, cands=cands)
        o = oracle.OracleState()
        want = run_on(o, case, follow_up=False)
        o.close()
        got = run_on(mirror, case, follow_up=False)
        assert mirror.plan_stats()["path"] == path, (n, path)
        same(want, got, (n, path))
        assert int(want[0].results["removable"].sum()) == len(cands)
