"""GPU parity of ca_filter_out_schedulable and ca_try_schedule_pods on the planted cases of
tests/filtgen.py (ring geometry and lastIndex, single-shape and mixed runs, hints, shape
counts, the similar-pods cache, static classes and the LDS bound, the window sequencer's
window moves, staged rows, slot edges, ports and scalars, planted breaks), pinned on the CPU
by tests/test_filter_cases.py.

Every case runs on every kernel it declares (the bitmap walk; the window sequencer, forced
with CASIM_FO_WINDOW where the call would not take it by itself) through FilterOutSchedulable
and through TrySchedulePods with three masks, with and without the break: every output equals
the oracle's and the step-by-step reference's, integer for integer; the whole state equals
the oracle's after the call and after a second call fed the first one's hints and lastIndex;
and Mirror.filter_stats() reports the route the case was written for.  Both kernels contain
loops that do not end on inconsistent state: run this file under a time limit of its own,
and read a limit hit as a hang."""
from __future__ import annotations

import numpy as np
import pytest

import filtgen as G
import snapmodel as S
import tspgen as T
from autoscaler_amd import abi, native
from conftest import gpu_available
from test_gpu_snapshot_state import _dims

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="no HIP device")]

CASES = G.all_cases()
CALLS = ["fos"] + [f"{m}-{b}" for m in G.MASKS for b in ("all", "break")]


def group_of(name: str) -> str:
    """One test per group and kernel: a long ring is a group of its own, the ring family goes
    by ring size, the threshold cases apart from the other mixed runs, the rest by family."""
    case = CASES[name]
    if len(case.nodes) > 600:
        return name
    if name.startswith("ring/") and not name.startswith("ring/P"):
        return f"ring/n{len(case.nodes)}"
    if name.startswith(("ring/P", "mixed/threshold")):
        return name.split("-")[0].rstrip("0123456789")
    return case.family


GROUPS: dict = {}
for _name in sorted(CASES):
    for _path in CASES[_name].paths:
        GROUPS.setdefault((group_of(_name), _path), []).append(_name)


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


def call_args(case, call):
    """(match, break) of a call; None for FilterOutSchedulable."""
    if call == "fos":
        return None
    if call == "own":
        return case.match, case.brk
    m, b = call.rsplit("-", 1)
    return G.make_match(m, case), b == "break"


def masked(case, match) -> bool:
    n = len(case.nodes)
    return match is not None and n > 0 and (match[0] != abi.CA_MATCH_ALL or 0 <= match[3] < n)


def run(b, case, args, hints, L):
    """One call on a backend: the mirror's entry points, or the same through the oracle."""
    try:
        if args is None:
            return b.filter_out_schedulable(case.pending, case.order, case.class_owner, hints, L)
        if isinstance(b, native.Mirror):
            return b.try_schedule_pods(case.pending, case.order, args[0], args[1], case.class_owner, hints, L)
        return T.try_schedule_ref(b, case.pending, case.order, args[0], args[1], case.class_owner, hints, L)
    except native.CasimError as e:
        if e.status == abi.CA_EDEVICE:          # nothing more on a device that faulted
            pytest.exit(f"device error in {case.name}: {e}", returncode=3)
        raise


_REF = {}


def reference(oracle, name, call):
    """The reference outputs of the call and of the second call behind it: computed once,
    shared by the paths, never changed."""
    if (name, call) not in _REF:
        case = CASES[name]
        args = call_args(case, call)
        o = oracle.OracleState()
        case.load(o)
        r1 = run(o, case, args, case.hints, case.L0)
        r2 = run(o, case, args, r1.hints, r1.last_index)
        o.close()
        _REF[(name, call)] = (r1, r2)
    return _REF[(name, call)]


def same(got, ref, fos, what):
    if not fos:
        T.eq_try(got, ref, what)
        return
    assert np.array_equal(got.node, ref.node), (what, np.nonzero(got.node != ref.node)[0][:10])
    assert np.array_equal(got.pod_id, ref.pod_id), what
    assert np.array_equal(got.hints, ref.hints), (what, np.nonzero(got.hints != ref.hints)[0][:10])
    assert (got.placed, got.last_index, got.evals, got.n_overflowing) == \
           (ref.placed, ref.last_index, ref.evals, ref.n_overflowing), what


def replay(o, case, ref):
    """The reference's placements on an oracle: the state the call must leave."""
    k = np.nonzero(ref.node >= 0)[0]
    if len(k):
        ids = o.add_pods(case.pending, case.order[k], ref.node[k])
        assert np.array_equal(ids, ref.pod_id[k])


def check_route(case, want, call, st):
    """filter_stats() after the first call against `want` (filtgen.route for this call)."""
    assert st["path"] == want["path"], (st["path"], want)
    got = (st["block_steps"], st["ring_scans"], st["windows"])
    if want["path"] == "bitmap":
        assert (st["shapes"], st["static_classes"], st["static_in_lds"]) == \
               (want["shapes"], want["static_classes"], want["static_in_lds"]), (st, want)
    elif len(case.nodes) <= G.SQ_WIN:           # the whole ring resident: no ring scan, no window move
        assert got[1:] == (0, 0), got
    rt = case.claims.get("route", {})
    if call != "fos":
        return
    if want["path"] == "bitmap":
        if "steps" in rt:                       # (mixed-run attempts, pods they placed, one-by-one steps)
            assert got == rt["steps"], got
        if "ring_scans" in rt:
            assert got[1] == rt["ring_scans"], got
    elif "window" in rt:
        if rt["window"] == "resident":
            assert got[1:] == (0, 0), got
        elif rt["window"] == "cursor":
            assert got[1] == 0 and got[2] >= 1, got
        else:
            assert got[1] >= 1 and got[2] >= 1, got


def run_case(name, path, call, oracle, mirror, monkeypatch):
    case = CASES[name]
    args = call_args(case, call)
    msk = masked(case, args[0]) if args else False
    # the declared paths are FilterOutSchedulable's; a mask's extra LDS words can take a call of
    # the LDS-edge case off the bitmap walk by itself (route() says so): the window run covers it
    natural = G.route(case, msk)["path"]
    if path == "bitmap" and natural == "window":
        assert call != "fos" and "window" in case.paths, (name, call)
        return
    forced = path == "window" and natural == "bitmap"
    monkeypatch.delenv("CASIM_FO_WINDOW", raising=False)
    if forced:
        monkeypatch.setenv("CASIM_FO_WINDOW", "1")
    want = G.route(case, msk, forced_window=forced)
    assert want["path"] == path
    r1, r2 = reference(oracle, name, call)
    dims = _dims(case.nodes, case.resident, case.pending)
    o = oracle.OracleState()
    case.load(o)
    case.load(mirror)
    g1 = run(mirror, case, args, case.hints, case.L0)
    st = mirror.filter_stats()
    same(g1, r1, args is None, (name, path, call))
    if len(case.order):                         # (an empty order returns before any route is taken)
        check_route(case, want, call, st)
    replay(o, case, r1)
    n_pods = len(case.resident) + r1.placed
    S.assert_state_oracle(mirror, o, n_pods, f"{name} {path} {call}", **dims)
    g2 = run(mirror, case, args, g1.hints, g1.last_index)
    same(g2, r2, args is None, (name, path, call, "second call"))
    replay(o, case, r2)
    S.assert_state_oracle(mirror, o, n_pods + r2.placed, f"{name} {path} {call} second call", **dims)
    o.close()


@pytest.mark.parametrize("group,path", sorted(GROUPS), ids=[f"{g}-{p}" for g, p in sorted(GROUPS)])
def test_cases(group, path, oracle, mirror, monkeypatch):
    """Every case of the group on the kernel, through every call; every failing (case, call) is
    reported, by name."""
    failed = []
    for name in GROUPS[(group, path)]:
        for call in CALLS + (["own"] if CASES[name].match is not None else []):
            try:
                run_case(name, path, call, oracle, mirror, monkeypatch)
            except AssertionError as e:
                failed.append(f"{name} [{call}]: {str(e)[:300]}")
    assert not failed, f"{len(failed)} failing:\n" + "\n".join(failed)


def test_every_case_runs_on_its_paths():
    """Every case declares at least one kernel; a case that declares the bitmap walk takes it
    by itself for FilterOutSchedulable, one that declares only the window kernel falls to it
    by itself."""
    for name, case in CASES.items():
        assert case.paths and set(case.paths) <= {"bitmap", "window"}, name
        if len(case.order):
            assert (G.route(case)["path"] == "bitmap") == ("bitmap" in case.paths), name
    assert sorted(n for names in GROUPS.values() for n in names) == sorted(n for n, c in CASES.items() for _ in c.paths)
