"""Resident pod columns, the parts that need no device: the column rule (podcolgen.expected_columns)
against the oracle's pod lists and the snapshot model's over seeded sequences, the cases against
the CPU oracle (each holds what it claims), the library's new exports, runonce.run's argument
checks and the stand-alone host program under the host sanitizers."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import podcolgen
import snapmodel as S
import utilgen
from autoscaler_amd import abi, native, runonce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("ca_mirror_set_pod_util_rows", "ca_mirror_get_pod_util_rows", "ca_mirror_utilization_resident",
             "ca_scale_down_candidates_create_resident", "ca_mirror_fetch_pod_columns", "ca_mirror_pod_column_stats",
             "ca_mirror_pod_count")
SEEDS, STEPS = range(10), 200


def test_library_exports_the_pod_column_calls():
    lib = native.load()
    for f in NEW_CALLS:
        assert hasattr(lib, f), f
        assert f in native.exported_symbols()
    out = (C.c_int32 * 32)()
    n = lib.ca_abi_struct_sizes(out, 32)
    assert list(out[:n]) == abi.EXPECTED_SIZES                         # additive: no record changed
    assert (abi.UTIL_POD_DTYPE.itemsize, abi.UTIL_INFO_DTYPE.itemsize, C.sizeof(abi.MirrorUtilArgsC)) == (48, 48, 64)
    assert lib.ca_abi_version() == abi.CASIM_ABI_VERSION
    for name in ("set_pod_util_rows", "pod_util_rows", "pod_columns", "pod_column_stats", "pod_count"):
        assert callable(getattr(native.Mirror, name, None)), name


# ---------------------------------------------------------------------------
# the column rule over the seeded sequences
# ---------------------------------------------------------------------------
class Reordered:
    """The oracle behind a position map: it has no reorder of its own, so the model's positions
    are translated to the oracle's on the way in and back on the way out."""
    backend_name = "oracle (reordered)"

    def __init__(self, o):
        self.o, self.map, self.stack = o, [], []

    def clear(self):
        self.o.clear()
        self.map, self.stack = [], []

    def add_nodes(self, recs):
        first = self.o.add_nodes(recs)
        self.map += range(first, first + len(recs))
        return len(self.map) - len(recs)

    def add_pods(self, table, idx, pos):
        return self.o.add_pods(table, idx, [self.map[x] for x in pos])

    def remove_pod(self, pid):
        self.o.remove_pod(pid)

    def remove_node(self, pos):
        at = self.map.pop(pos)
        self.o.remove_node(at)
        self.map = [x - 1 if x > at else x for x in self.map]

    def fork(self):
        self.stack.append(list(self.map))
        self.o.fork()

    def revert(self):
        self.map = self.stack.pop()
        self.o.revert()

    def commit(self):
        self.stack.pop()
        self.o.commit()

    def reorder_nodes(self, order):
        assert not self.stack
        self.map = [self.map[k] for k in order]

    def node_count(self):
        return len(self.map)

    def node_pods(self, x):
        return self.o.node_pods(self.map[x])

    def pod_node(self, pid):
        at = self.o.pod_node(pid)
        return -1 if at < 0 else self.map.index(at)


def model_columns(model: S.SnapModel):
    return podcolgen.expected_columns([nd.pods for nd in model.nodes], len(model.pod_rec))


@pytest.fixture(scope="module")
def runs(oracle_lib):
    """Per seed: what the sequence covered.  The rule is checked after every step."""
    out = []
    for seed in SEEDS:
        o = Reordered(oracle_lib.OracleState())
        s = S.Sequence(seed)
        s.load([o])
        rng = random.Random(f"podcols/{seed}")
        cov = dict(reorder=0, remove_node=0, revert_remove_node=0, revert_moved_second=0)
        frames = []                              # per open fork: (removed a node, removed a pod that was not last)
        for _ in range(STEPS):
            before = [list(nd.pods) for nd in s.model.nodes]
            placed_before = {p: (x, l.index(p)) for x, l in enumerate(before) for p in l}
            op = podcolgen.step_with_reorder(s, [o], rng)
            if op == "fork":
                frames.append([False, False])
            elif op == "commit":
                fr = frames.pop()
                if frames:
                    frames[-1] = [a or b for a, b in zip(frames[-1], fr)]
            elif op == "revert":
                fr = frames.pop()
                cov["revert_remove_node"] += fr[0]
                cov["revert_moved_second"] += fr[1]
            elif op == "remove_node":
                cov["remove_node"] += 1
                if frames:
                    frames[-1][0] = True
            elif op == "remove_pod" and frames:
                gone = (set(placed_before) - set(s.model.placed())).pop()
                x, slot = placed_before[gone]
                frames[-1][1] |= slot != len(before[x]) - 1              # the last pod took its slot
            elif op == "reorder":
                cov["reorder"] += 1
            node, slot = model_columns(s.model)
            n = o.node_count()
            want = podcolgen.expected_columns([o.node_pods(x) for x in range(n)], len(s.model.pod_rec))
            assert np.array_equal(node, want[0]) and np.array_equal(slot, want[1]), s.ctx()
            assert node.tolist() == s.model.pod_nodes(), s.ctx()
            assert node.tolist() == [o.pod_node(i) for i in range(len(node))], s.ctx()
        out.append(cov)
    return out


def test_expected_columns_on_the_model_and_the_oracle(runs):
    assert len(runs) == len(SEEDS)


@pytest.mark.parametrize("what", ["reorder", "remove_node", "revert_remove_node", "revert_moved_second"])
def test_the_sequences_cover(what, runs):
    assert sum(c[what] for c in runs) > 0, what


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def _candidates(name):
    c = podcolgen.case(name)
    info, drain = podcolgen.expected(name, False, False)
    lists = c.node_lists()
    return c, lists, utilgen.candidates_of(info, drain, c.thr, c.gpu_thr, c.eligible, lists, c.pod_flags())


def test_case_names():
    assert list(podcolgen.all_cases()) == podcolgen.CASE_NAMES


@pytest.mark.parametrize("name", podcolgen.CASE_NAMES)
def test_case_holds_its_claims(name, oracle_lib):
    c, lists, want = _candidates(name)
    cl = c.claims
    assert len(c.removed) > 0 or len(c.pods) == 0                # every case carries removals
    node, slot = podcolgen.expected_columns(lists, len(c.pods))
    assert (node[c.removed] == -1).all() and (node >= 0).sum() == len(c.pods) - len(c.removed)
    for x, l in enumerate(lists):                                # the slot table's index is a bijection per node
        assert sorted(slot[l].tolist()) == list(range(len(l))) and (node[l] == x).all()
    if "cand" in cl:
        assert want["cand"].tolist() == cl["cand"]
        assert [len(lists[x]) for x in cl["cand"]] == cl["cand_counts"]
        assert sum(cl["cand_counts"]) == cl["table_total"]
        if cl["cand"]:                                           # the first and the last candidate next to others
            assert want["node_class"][cl["cand"][0] - 1] != abi.CA_SD_CANDIDATE
            assert want["node_class"][cl["cand"][-1] + 1] != abi.CA_SD_CANDIDATE
    # some candidate's movable pods are not in ascending id order (None: the edge rules it out)
    unordered = [int(x) for k, x in enumerate(want["cand"])
                 if np.any(np.diff(want["move_pods"][want["move_off"][k]:want["move_off"][k + 1]]) < 0)]
    if cl.get("unordered_any"):
        assert unordered
    elif cl["unordered"] is None:
        assert len(want["cand"]) == 0 or cl["table_total"] <= 1
    else:
        assert cl["unordered"] in unordered
    if "empty_list" in cl:
        k = want["cand"].tolist().index(cl["empty_list"])
        assert want["move_off"][k] == want["move_off"][k + 1] and len(lists[cl["empty_list"]]) > 0
        assert want["cand_status"][k] == abi.CA_UNREMOVABLE_BLOCKED_BY_POD
    for i in cl.get("detached_rows", []):
        assert node[i] == -1 and i in c.pod_over[0].tolist()


def test_the_cases_sit_on_the_edges():
    totals = {podcolgen.case(n).claims["table_total"] for n in podcolgen.CASE_NAMES if n.startswith("table_")}
    assert totals == {0, 1, podcolgen.TILE - 1, podcolgen.TILE, podcolgen.TILE + 1, 2 * podcolgen.TILE + 1}
    assert {len(podcolgen.case(n).claims["cand"]) for n in podcolgen.CASE_NAMES if n.startswith("cands_")} == \
        {0, 1, 1023, 1024, 1025}
    assert set(podcolgen.case("cand_counts").claims["cand_counts"]) == {1, 63, 64, 65, 255, 256, 257}
    assert {len(podcolgen.case(f"ids_{p}").pods) for p in (65535, 65536, 65537)} >= {65535, 65536, 65537}
    c = podcolgen.case("rows_all")
    assert c.pod_over[0].tolist() == list(range(len(c.pods)))
    c = podcolgen.case("rows_first_last")
    assert c.pod_over[0].tolist() == [0, len(c.pods) - 1]


def test_split_overrides_conflict_where_both_are_sent():
    c = podcolgen.case("rows_all")
    ways = podcolgen.split_overrides(c)
    assert len(ways) == 3 and ways[0][1] is None and ways[1][0] is None
    (rid, rrows), (cid, crows) = ways[2]
    at = np.searchsorted(rid, cid)
    assert len(cid) > 0 and (rrows[at]["flags"] != crows["flags"]).all()
    assert (rrows[at]["req_milli"][:, 0] != crows["req_milli"][:, 0]).all()
    assert podcolgen.split_overrides(podcolgen.case("cand_counts")) == [(None, None)]


# ---------------------------------------------------------------------------
# the callers' argument checks, and the host program
# ---------------------------------------------------------------------------
def test_runonce_scale_down_values(oracle_lib):
    w = runonce.c5_runonce(n_nodes=40, n_pending=60, n_groups=4)
    o = oracle_lib.OracleState()
    with pytest.raises(ValueError):
        runonce.run(o, oracle_lib.runonce_cpu_util, w, scale_down="gpu")
    for form in ("device", "resident"):                          # the device mirror only
        with pytest.raises(TypeError):
            runonce.run(o, oracle_lib.runonce_cpu_util, w, scale_down=form)


def test_host_program_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "podcols_host_check"
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "podcols_host_check.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert "podcols host checks ok" in done.stdout
