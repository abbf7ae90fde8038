"""The cases of tests/pricegen.py on the CPU restatement's lists: they hold what they claim
(lengths, planted specials, groups without a sum), and the in-order float64 sum they expect
cannot be mistaken for a reordered one — a kernel that summed right to left, by per-lane
partials and a tree, or exactly (math.fsum) would fail on every list of 8 or more pods."""
import math

import numpy as np
import pytest

import pricegen as P
from autoscaler_amd import abi


@pytest.fixture(scope="module")
def oracle_state(oracle_lib):
    st = oracle_lib.OracleState()
    yield st
    st.close()


@pytest.fixture(scope="module")
def solved(oracle_state):
    """[(case, max_nodes, results, lists)] for every case and limit, computed once."""
    out = []
    for case in P.all_cases():
        enc = case.encode()
        for limit in case.limits:
            ro, lists = P.oracle_lists(oracle_state, enc, limit)
            out.append((case, limit, ro.results, lists))
    return out


def _of(solved, name, limit=0):
    return next((c, r, ls) for c, lim, r, ls in solved if c.name == name and lim == limit)


REORDERED = (("right to left", P.reversed_sum), ("64 lane partials and a tree", P.lane_tree_sum),
             ("math.fsum", P.fsum))


@pytest.fixture(scope="module")
def coincidences(solved):
    """(number of lists of at least 8 counted pods and only finite normal prices, per reordering
    the lists whose in-order sum has the same bytes)."""
    tiny = np.finfo(np.float64).tiny
    n_lists, same = 0, {name: [] for name, _ in REORDERED}
    for case, limit, _, lists in solved:
        for g, ids in enumerate(lists):
            p = case.price[ids]
            if len(ids) < 8 or not (np.isfinite(p).all() and (np.abs(p) >= tiny).all()):
                continue
            n_lists += 1
            want = P.bits(P.in_order_sum(case.price, ids))
            for name, f in REORDERED:
                if P.bits(f(case.price, ids)) == want:
                    same[name].append((case.name, limit, g, len(ids)))
    return n_lists, same


def test_in_order_sums_differ_from_reordered_sums(coincidences):
    """Every list of at least 8 counted pods and only finite normal prices: the left-to-right sum
    differs in bytes from the right-to-left sum, from 64 strided lane partials combined by a
    tree, and from math.fsum; at most 5 % of such lists may coincide with one of the three.

    Random lists do not give that: two orders of a short float64 sum meet in the same bits some
    40 % of the time.  pricegen draws each list until it shows all three reorderings and knows the
    oracle's order through ranked pods (test_generator_knows_the_lists); what is left are the two
    planted lists that sum to 2e300 and to +inf in any order."""
    n_lists, same = coincidences
    assert n_lists >= 150
    any_same = {key for hits in same.values() for key in hits}
    print({name: len(hits) for name, hits in same.items()}, len(any_same), n_lists)
    assert len(any_same) <= 0.05 * n_lists, (sorted(any_same), n_lists)
    assert {key[0] for key in any_same} <= {"specials"}


def test_generator_knows_the_lists(solved):
    """The lists the generator drew its slices for are the oracle's, id for id and in order: ranked
    pods sort by pod-set index, and a limited run on a template whose pod count binds leaves the
    first pods-per-node x max_nodes of them."""
    claimed = 0
    for case, limit, _, lists in solved:
        for (lim, g), ids in case.built.items():
            if lim == limit:
                assert lists[g] == list(ids), (case.name, limit, g)
                claimed += 1
    assert claimed >= 149 + 6 + 7 + 1 + 300


def test_edges_case_lists(solved):
    case, res, lists = _of(solved, "edges")
    assert sorted(len(ids) for ids in lists) == sorted(P.EDGE_LENGTHS)          # every pod schedules
    assert (res["status"] == abi.CA_OK).all()
    table, tm, off, idx = case.encode()
    long_ones = [int(off[g]) for g, ids in enumerate(lists) if len(ids) >= 64]
    assert {a % 4 for a in off[:-1].tolist()} == {0, 1, 2, 3}
    assert len({a % 64 for a in off[:-1].tolist()}) == 64
    assert {a % 4 for a in long_ones} == {0, 1, 2, 3}
    assert P.CHUNK <= 2048                                                      # (else: add the chunk's edges)
    for n in (P.CHUNK - 1, P.CHUNK, P.CHUNK + 1, 16 * P.CHUNK - 1, 16 * P.CHUNK, 16 * P.CHUNK + 1):
        assert n in P.EDGE_LENGTHS


def test_stale_case_lists(solved):
    case, _, full = _of(solved, "stale", 0)
    _, _, short = _of(solved, "stale", P.STALE_LIMIT)
    g = case.index
    assert [len(full[g[k]]) for k in ("a", "ten", "b")] == [700, 300, 520]
    assert [len(short[g[k]]) for k in ("a", "ten", "b")] == [110, 10, 110]
    for k in ("a", "ten", "b"):                       # the short sums differ from the long ones
        assert P.bits(P.in_order_sum(case.price, full[g[k]])) != P.bits(P.in_order_sum(case.price, short[g[k]]))


def test_slots_case_lists(solved):
    case, res, lists = _of(solved, "slots")
    g = case.index
    st = res["status"].tolist()
    assert st[g["cut"]] == abi.CA_EUNSUPPORTED and st[g["after"]] == abi.CA_ENOTRUN
    assert st[g["huge"]] == abi.CA_OK and int(res[g["huge"]]["n_scheduled"]) == 0
    for k in ("empty", "huge", "cut", "after"):
        assert lists[g[k]] == []
    assert [len(lists[g[k]]) for k in ("first", "second", "third")] == [40, 60, 9]


def test_specials_case_totals(solved):
    case, _, lists = _of(solved, "specials")
    g = case.index
    want = {k: P.in_order_sum(case.price, lists[g[k]]) for k in g}
    tiny = np.finfo(np.float64).tiny
    assert 0.0 < want["subnormal"] < tiny and want["subnormal"] == math.fsum(P.SUBNORMALS)
    assert P.bits(want["negzero"]) == P.bits(0.0)                               # +0.0 + -0.0 + -0.0
    assert math.isfinite(want["big"]) and want["big"] >= 2e300
    assert want["overflow"] == math.inf and want["pinf"] == math.inf
    assert math.isnan(want["infnan"]) and math.isnan(want["nan"])
    assert math.isfinite(want["plain"]) and want["plain"] > 0 and len(lists[g["plain"]]) == 24
    # a subnormal beside normal prices, and -0.0, change nothing that rounding keeps
    assert len(lists[g["subnormal_mixed"]]) == 11 and len(lists[g["negzero_mixed"]]) == 10


def test_many_and_uniform_case_lists(solved):
    case, res, lists = _of(solved, "many")
    assert len(lists) == 300 and sum(len(ids) <= 7 for ids in lists) >= 290
    assert max(len(ids) for ids in lists) > 3 * P.CHUNK
    case, _, lists = _of(solved, "uniform", 0)
    _, _, limited = _of(solved, "uniform", 3)
    g = case.index
    assert [len(lists[g[k]]) for k in "abcd"] == [570, 610, 430, 60]
    assert all(len(limited[g[k]]) < len(lists[g[k]]) for k in "abc")
    shapes = {(int(r["score_milli_cpu"]), int(r["score_memory"])) for r in case.encode()[0].pods}
    assert len(shapes) == 3
