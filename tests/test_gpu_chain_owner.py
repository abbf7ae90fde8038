"""The lean chain's wave-owned rows (k_ffd_chain<.., TB, LEAN>: 64-row block b belongs to wave
b mod 4 for the whole kernel, one barrier per row pass, the opening's copy count from the run
table) against the CPU restatement, bit-exact: results, lastIndex and scheduled pods up to
n_scheduled, in the published 32-bit, published 16-bit and device-resident modes, with
CASIM_LEAN_CHAIN 1 and 0 (test_gpu_lean_chain's _check, which also checks stats()["lean_chain"]).

The batches are built by test_gpu_lean_chain's _inputs from its shapes.  On T_ONE (3000m / 6 GiB)
one `top` fills a node up to a leftover of 1000m / 2 GiB, which holds one `s1`, two `s2`, four `s3`
or ten `bottom`; a fresh copy holds two `half` and nothing fits beside a `top` but those.  With no
existing nodes the rotation starts at row 0 after `top`'s opening (one pod per node leaves
lastIndex alone), so `s1` x m fills rows 0..m-1 and the next class meets its first row with room at
row m.  Every case first asserts its own premise on the oracle's output, so a case that no longer
reaches its edge fails instead of passing idly.
"""
import pytest

from estgen import _encode_estimate
import test_gpu_lean_chain as lc

pytestmark = pytest.mark.gpu

T_ONE, T_MID = lc.T_ONE, lc.T_MID


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


def _oracle_out(oracle, inputs, max_nodes, L0=0):
    """The oracle's results alone, for a case's premise."""
    nodes, pods, templates, groups = inputs
    table, node_recs, tm, off, pod_idx = _encode_estimate(nodes, pods, templates, groups)
    o = oracle.OracleState()
    o.clear()
    if len(node_recs):
        o.add_nodes(node_recs)
    return o.estimate(table, off, pod_idx, tm, max_nodes, L0).results


def _total(group):
    return sum(n for _, n in group)


def _run(oracle, monkeypatch, groups, templates, max_nodes=0, L0=0, n_existing=0, nodes_added=None,
         n_scheduled=None, last_index_out=None, **kw):
    """Premise on the oracle's output (per group; None: not part of the premise), then _check."""
    inputs = lc._inputs(groups, templates, n_existing=n_existing)
    ro = _oracle_out(oracle, inputs, max_nodes, L0)
    for g, grp in enumerate(groups):
        want_sched = _total(grp) if n_scheduled is None else n_scheduled[g]
        assert int(ro[g]["n_scheduled"]) == want_sched, (g, ro[g])
        if nodes_added is not None and nodes_added[g] is not None:
            assert int(ro[g]["nodes_added"]) == nodes_added[g], (g, ro[g])
        if last_index_out is not None and last_index_out[g] is not None:
            assert int(ro[g]["last_index_out"]) == last_index_out[g], (g, ro[g])
    lc._check(oracle, monkeypatch, inputs, max_nodes, L0=L0, **kw)
    return ro


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 320, 321])
def test_row_counts(n, oracle, monkeypatch):
    """n rows from one opening of n template copies (320 and 321: every wave writes full blocks of
    it): one block and one owner up to 64 rows, 65 the second owner's first row; 255 / 256 / 257
    around the ownership wrap (block 4 returns to wave 0, which then owns two blocks that are not
    adjacent), 320 / 321 a full and a one-row sixth block.  `s3` x (n + 10) goes once round every
    row and on to ten of them (room in both of wave 0's blocks), `bottom` x 30 meets two copy
    counts from row 10 on and leaves lastIndex at 40.  Chunks of 64 outputs, so tickets are pushed
    mid-chain."""
    monkeypatch.setenv("CASIM_PUB_CHUNK", "64")
    groups = [[("top", n), ("s3", n + 10), ("bottom", 30)]]
    _run(oracle, monkeypatch, groups, [T_ONE], nodes_added=[n], last_index_out=[40])


@pytest.mark.parametrize("b", [0, 1, 2, 3, 4])
def test_pick_in_each_block(b, oracle, monkeypatch):
    """321 rows; `s1` x 64 b fills blocks 0..b-1, so `s3` x 5 finds its rows with room from row
    64 b on and the pick (the fifth of them) falls in block b: lastIndex 64 b + 5.  b = 4: wave 0
    has room in its later block only; b = 0: in both."""
    monkeypatch.setenv("CASIM_PUB_CHUNK", "64")
    groups = [[("top", 321), ("s1", 64 * b), ("s3", 5)]] if b else [[("top", 321), ("s3", 5)]]
    _run(oracle, monkeypatch, groups, [T_ONE], nodes_added=[321], last_index_out=[64 * b + 5])


@pytest.mark.parametrize("j0,m,last", [(10, 70, 79), (100, 20, 119), (300, 70, 48), (70, 100, 169), (200, 1, 200)])
def test_rotation_start_and_pick_block(j0, m, last, oracle, monkeypatch):
    """Five existing nodes and the input lastIndex 5 + j0: the rotation of `s3` x m over 321 rows
    with room starts at row j0 and its last placement lands on row `last`.  The start lies in a
    block before the pick's (10 -> 79), in the pick's own block (100 -> 119), behind it (300 -> 48,
    wrapping), in a block of another wave than the pick's block (70: wave 1 -> 169: wave 2), and
    on the picked row itself."""
    assert last == (j0 + m - 1) % 321
    groups = [[("top", 321), ("s3", m)]]
    _run(oracle, monkeypatch, groups, [T_ONE], L0=5 + j0, n_existing=5, nodes_added=[321],
         last_index_out=[(5 + last + 1) % 326])


def test_back_to_back_runs_without_opening(oracle, monkeypatch):
    """Eight rows: `s2` x 6 and `s3` x 8 both end inside the rows' capacity (S >= RN: two runs in
    a row with no opening and so no barrier between them), then `bottom` x 200 finds room for 26
    (rows 0..5 hold two each, rows 6 and 7 seven) and opens six nodes for the other 174: 14 in
    all.  Group 1: the same over 70 rows in two owners' blocks (`bottom`: 64 x 2 + 6 x 7 = 170 on
    the rows, 130 more on five new nodes)."""
    groups = [
        [("top", 8), ("s2", 6), ("s3", 8), ("bottom", 200)],
        [("top", 70), ("s2", 64), ("s3", 70), ("bottom", 300)],
    ]
    _run(oracle, monkeypatch, groups, [T_ONE, T_ONE], nodes_added=[14, 75])


@pytest.mark.parametrize("n_top,n_half,first,end", [(60, 20, 60, 70), (250, 32, 250, 266), (60, 19, 60, 70)])
def test_opening_extent(n_top, n_half, first, end, oracle, monkeypatch):
    """`half` (two per fresh copy, none beside a `top`) opens rows [first, end) in one closed form:
    60..69 cross a block edge, 250..265 the ownership wrap (blocks 3 and 4: waves 3 and 0).  An odd
    count leaves the last opened row half full.  `s3` and `bottom` then read every row."""
    monkeypatch.setenv("CASIM_PUB_CHUNK", "64")
    groups = [[("top", n_top), ("half", n_half), ("s3", n_top + 9), ("bottom", 25)]]
    _run(oracle, monkeypatch, groups, [T_ONE], nodes_added=[end])


@pytest.mark.parametrize("w", [1, 2, 3])
def test_one_row_with_room(w, oracle, monkeypatch):
    """260 rows, rotation start j0 = 64 w + 11: `s1` x 259 fills every row from j0 round to
    j0 - 2, so row 64 w + 10 — in a block of wave w — is the only one with room for `s2` x 2
    (nalive == 1: its owner alone writes it) and lastIndex ends behind it, at the input value."""
    j0 = 64 * w + 11
    groups = [[("top", 260), ("s1", 259), ("s2", 2)]]
    _run(oracle, monkeypatch, groups, [T_ONE], L0=5 + j0, n_existing=5, nodes_added=[260],
         last_index_out=[5 + j0])


def test_copy_levels_across_owners(oracle, monkeypatch):
    """70 rows in two owners' blocks: `s2` x 40 and `s3` x 50 leave rows 0..19 with 250m, 20..39
    with 500m and 40..69 with 750m, i.e. 2, 5 and 7 `bottom` copies: `bottom` x 330 of the 350 that
    fit takes three levels (140 + 150 + 40) and opens nothing."""
    groups = [[("top", 70), ("s2", 40), ("s3", 50), ("bottom", 330)]]
    _run(oracle, monkeypatch, groups, [T_ONE], nodes_added=[70])


@pytest.mark.parametrize("max_nodes", [70, 72, 75])
def test_limiter_inside_opening(max_nodes, oracle, monkeypatch):
    """70 rows hold 140 `s2`; 60 more want ten nodes.  max_nodes 70: no new node at all; 72 and
    75: the limiter stops inside the closed-form opening and the run goes on to the exhausted
    path (the last opened row is full) before it stops."""
    groups = [[("top", 70), ("s2", 200), ("bottom", 45)]]
    extra = max_nodes - 70
    _run(oracle, monkeypatch, groups, [T_ONE], max_nodes=max_nodes, nodes_added=[max_nodes],
         n_scheduled=[70 + 140 + 6 * extra])


def test_single_pods_between_runs(oracle, monkeypatch):
    """A class of one pod (the per-pod path) directly after a run that ended with no barrier — an
    opening (`top`), then a run inside the rows' capacity (`s2`) — and back to runs, over 70 rows
    in two owners' blocks; group 1 on T_MID with a cpu-only class."""
    groups = [
        [("top", 70), ("s1", 1), ("s2", 30), ("s3", 1), ("bottom", 40)],
        [("s1", 30), ("s2", 1), ("conly", 12), ("s3", 1), ("bottom", 20)],
    ]
    ro = _run(oracle, monkeypatch, groups, [T_ONE, T_MID], nodes_added=[70, None])
    assert int(ro[1]["nodes_added"]) >= 1


def test_pod_that_fits_no_fresh_copy(oracle, monkeypatch):
    """`cpuh` (7000m) and `memh` (14 GiB) fit no T_ONE copy: the first `cpuh` opens a node that
    stays empty (CheckPredicates fails), the rest of its run and `memh`'s take the empty-node skip,
    and `top` x 5 then finds that one row with room and opens four more."""
    groups = [[("cpuh", 3), ("memh", 2), ("top", 5), ("s2", 10)]]
    _run(oracle, monkeypatch, groups, [T_ONE], nodes_added=[5], n_scheduled=[15])


def test_second_speculation_round(oracle, monkeypatch):
    """As test_gpu_lean_chain's: round 1 guesses the input lastIndex for group 1, group 0 (70 rows in
    two owners' blocks, an opening of twelve more) leaves another one and group 1's outcome depends
    on it."""
    groups = [[("top", 70), ("s2", 200), ("bottom", 45)], [("top", 5), ("s1", 33), ("s3", 20)]]
    inputs = lc._inputs(groups, [T_ONE, T_ONE], n_existing=5)
    lc._check(oracle, monkeypatch, inputs, 100, L0=3, min_rounds=2)
    lc._check(oracle, monkeypatch, inputs, 0, L0=123, min_rounds=2)
