"""The option-matrix form of the Estimate plan, the parts that need no device: the numpy
statement of the append loop against the workloads' own lists, the cases the GPU test runs,
and the library's new entry points."""
import ctypes as C

import numpy as np

from autoscaler_amd import abi, native, workloads as W
import optgen
from optgen import T, C as CHUNK


def _exact(w):
    eg_off, eg_pod, ok = optgen.options_of(w)
    off, idx = optgen.lists_of(eg_off, eg_pod, ok)
    assert off.dtype == np.int32 and idx.dtype == np.int32
    assert np.array_equal(off, w.group_off)
    assert np.array_equal(idx, w.pod_idx)
    return eg_off, ok


def test_options_of_c2_reproduces_lists():
    w = W.c2(n_pods=5000, n_groups=12, n_existing=10)
    eg_off, ok = _exact(w)
    assert len(eg_off) - 1 == 50 and ok.shape == (12, 50)
    assert 0 < ok.sum() < ok.size                     # some pairs pass, some fail


def test_options_of_c4_reproduces_lists():
    w = W.c4(n_pods=3000, n_groups=8, n_existing=10, pods_per_controller=30)
    eg_off, ok = _exact(w)
    assert len(eg_off) - 1 == 100 and 0 < ok.sum() < ok.size


def test_lists_of_is_the_append_loop():
    eg_off = [0, 2, 2, 5]
    eg_pod = [7, 3, 9, 1, 4]
    off, idx = optgen.lists_of(eg_off, eg_pod, [[1, 1, 1], [0, 1, 0], [0, 0, 1], [5, 0, 0]])
    assert off.tolist() == [0, 5, 5, 8, 10]
    assert idx.tolist() == [7, 3, 9, 1, 4, 9, 1, 4, 7, 3]


def test_cases_hold_what_they_claim():
    cases = {c[0]: c for c in optgen.cases()}
    assert list(cases) == optgen.CASE_NAMES
    assert (T, CHUNK) == (2048, 256)
    n_base = 0
    for name, w, eg_off, eg_pod, ok, tm, claim in cases.values():
        E = len(eg_off) - 1
        assert ok.shape == (len(tm), E) and ok.dtype == np.uint8, name
        assert eg_off[0] == 0 and (np.diff(eg_off) >= 0).all() and eg_off[-1] == len(eg_pod), name
        assert eg_pod.min() >= 0 and eg_pod.max() < len(w.table), name
        assert len(np.unique(eg_pod)) == len(eg_pod), name            # disjoint groups
        off, idx = optgen.lists_of(eg_off, eg_pod, ok)
        if "lengths" in claim:
            assert np.diff(off).tolist() == claim["lengths"], name
        if "max_eg" in claim:
            assert np.diff(eg_off).max() == claim["max_eg"] > 3 * T, name
        if "n_eg" in claim:
            assert E == claim["n_eg"], name
        if "n_groups" in claim:
            assert len(tm) == claim["n_groups"], name
        if "min_classes" in claim:
            sc = np.stack([w.table.pods["score_milli_cpu"], w.table.pods["score_memory"]], 1)
            assert len(np.unique(sc, axis=0)) >= claim["min_classes"], name
        n_base += w is optgen.base()
    assert n_base == 9 and len(optgen.base().table) <= 20_000
    # the shared podset: uniform classes without a score tie on any template of the cases (the
    # plans run decoupled unless a knob forbids it), and every pod fits every template
    shapes = [(c, m) for c in optgen.BASE_CPU for m in optgen.BASE_MEM]
    assert optgen.score_ties(shapes, optgen.TEMPLATE_SHAPES) == 0
    assert optgen.score_ties([(500, 1 << 30), (1000, 2 << 30)], [(4000, 16 << 30)]) == 0
    assert optgen.score_ties([(1000, 1 << 30), (500, 3 << 30)], [(4000, 16 << 30)]) == 1
    for name, w, *_, tm, _ in cases.values():
        if w is optgen.base():
            alloc = {(int(t["node"]["alloc_milli_cpu"]), int(t["node"]["alloc_memory"])) for t in tm}
            assert alloc <= set(optgen.TEMPLATE_SHAPES), name
            assert min(a for a, _ in alloc) - 200 >= max(optgen.BASE_CPU), name
            assert min(m for _, m in alloc) - 256 * W.MI >= max(optgen.BASE_MEM), name
    # the structured rows: all zeros, all ones, alternating, first and last failing
    ok = cases[f"n_eg_{CHUNK + 1}"][4]
    assert not ok[0].any() and ok[1].all() and ok[2, 1::2].all() and not ok[2, ::2].any()
    assert ok[4, 0] == 0 and ok[4, -1] == 0 and ok[4, 1:-1].all()
    assert cases["singletons"][2][-1] == len(cases["singletons"][3]) == 3 * CHUNK + 17
    er = cases["equal_rows"]
    assert np.array_equal(er[4][0], er[4][1]) and not np.array_equal(er[4][0], er[4][4])
    assert cases["n_eg_1"][4].shape == (1, 1) and (np.diff(cases[f"n_eg_{CHUNK}"][2]) == 0).any()   # an empty group


def test_library_exports_the_option_constructor():
    lib = native.load()
    for f in ("ca_estimate_plan_create_options", "ca_estimate_plan_fetch_lists"):
        assert hasattr(lib, f), f
        assert f in native.exported_symbols()
    out = (C.c_int32 * 32)()
    n = lib.ca_abi_struct_sizes(out, 32)
    assert list(out[:n]) == abi.EXPECTED_SIZES                         # additive: no record changed
    assert lib.ca_abi_version() == abi.CASIM_ABI_VERSION
    assert callable(native.EstimatePlan.from_options) and callable(native.Mirror.estimate_options)
