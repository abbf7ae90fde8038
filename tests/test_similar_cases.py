"""The cases of tests/similargen.py on the CPU restatement's lists: what the generator claims by
construction holds, every case has the candidates that make a wrong kernel visible, and the
stale-tail case is what it says.  Keeps tests/test_gpu_similar.py from passing vacuously."""
import pytest

import similargen as S
from autoscaler_amd import abi


@pytest.fixture(scope="module")
def state(oracle_lib):
    st = oracle_lib.OracleState()
    yield st
    st.close()


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in S.all_cases()}


CASE_NAMES = [c.name for c in S.all_cases()]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_has_the_three_kinds_of_candidate(name, cases, state):
    c = cases[name]
    enc = c.encode()
    off = enc[2].tolist()
    _, lists = S.oracle_lists(state, enc, c.limits[-1])
    req = c.g(c.required)
    n_req = len(lists[req])
    assert n_req > 0
    miss = {cand: S.missing_positions(lists, req, c.g(cand)) for cand in set(c.candidates)}
    for cand, want in c.built.items():                     # the generator's claims
        assert miss[cand] == want, (name, cand)
    counts = [len(m) for m in miss.values()]
    assert 0 in counts and 1 in counts and n_req in counts, (name, sorted(counts))
    # one pod, one id: every group's pod_idx slice indexes the one table
    table = enc[0]
    assert len(table) == len(c.pods) and max(max(l, default=0) for l in lists) < len(c.pods)
    # the required list and some candidate sit at offsets that are no multiple of 4
    assert off[req] % 4 != 0 or name in ("shapes",)
    assert {off[c.g(cand)] % 4 for cand in c.candidates} - {0}


@pytest.mark.parametrize("n,res", S.TILE_CASES)
def test_tile_cases_put_the_missing_pod_on_both_sides_of_a_tile_boundary(n, res, cases, state):
    c = cases[f"tile-{n}-{res}"]
    enc = c.encode()
    off = enc[2].tolist()
    assert off[c.g("req")] % 4 == res
    singles = sorted(v[0] for k, v in c.built.items() if k.startswith("drop"))
    assert singles[0] == 0 and singles[-1] == n - 1
    # buffer position of list position p, from the tile origin (the offset rounded down to 4)
    tile_of = [(res + p) // S.TILE for p in singles]
    if res + n > S.TILE:
        assert any(tile_of[i] + 1 == tile_of[i + 1] and singles[i] + 1 == singles[i + 1] for i in range(len(singles) - 1))
        a, b = c.built["two"]
        assert (res + a) // S.TILE != (res + b) // S.TILE
    assert {off[c.g(k)] % 4 for k in c.built} >= {1, 2, 3}


@pytest.mark.parametrize("n_pods", S.WORD_SIZES)
def test_word_cases_miss_and_hold_the_word_edge_ids(n_pods, cases, state):
    c = cases[f"word-{n_pods}"]
    assert n_pods % 32 in (0, 1, 31)
    _, lists = S.oracle_lists(state, c.encode(), 0)
    req = lists[c.g("req")]
    edge = [0, 31, 32, n_pods - 1]
    for m in edge:
        have = set(lists[c.g(f"id{m}")])
        pos = S.missing_positions(lists, c.g("req"), c.g(f"id{m}"))
        assert [req[p] for p in pos] == [m]                      # the missing pod's id
        assert all(e in have for e in edge if e != m)             # the others are present ones


def test_stale_tail_case_is_what_it_claims(cases, state):
    """The pods ten's final list lacks are in ten's list of the earlier, unlimited run, at
    positions at or beyond the later run's n_scheduled: a mark kernel that does not stop at
    n_scheduled finds them in the buffer."""
    c = cases["stale"]
    enc = c.encode()
    assert c.limits == (0, S.STALE_LIMIT)
    _, long_lists = S.oracle_lists(state, enc, c.limits[0])
    ro, lists = S.oracle_lists(state, enc, c.limits[1])
    req, ten = c.g("req"), c.g("ten")
    n_ten = len(lists[ten])
    assert 0 < n_ten < len(long_lists[ten]) and long_lists[ten][:n_ten] == lists[ten]
    lacking = [lists[req][p] for p in S.missing_positions(lists, req, ten)]
    assert len(lacking) > 0
    for pod in lacking:
        assert pod in long_lists[ten] and long_lists[ten].index(pod) >= n_ten
    # with the stale tail counted as members nothing would be missing
    assert S.missing_positions([long_lists[ten] if g == ten else l for g, l in enumerate(lists)], req, ten) == []


def test_prefix_case_statuses(cases, state):
    c = cases["prefix"]
    ro, lists = S.oracle_lists(state, c.encode(), 0)
    st = ro.results["status"].tolist()
    assert st[c.g("cut")] == abi.CA_EUNSUPPORTED and st[c.g("after")] == abi.CA_ENOTRUN
    assert all(s == abi.CA_OK for s in st[:c.g("cut")])
    assert lists[c.g("cut")] == [] and lists[c.g("after")] == []


def test_slots_and_many_cases(cases, state):
    c = cases["slots"]
    _, lists = S.oracle_lists(state, c.encode(), 0)
    assert lists[c.g("empty")] == [] and lists[c.g("huge")] == [] and len(c.groups[c.g("huge")]) == 2
    assert c.candidates.count("sub") >= 2 and "req" in c.candidates
    m = cases["many"]
    assert len(set(m.candidates)) == 300 > 256
