"""The two-launch Go-order sort (csrc/pdqsort.h, k_pdq_sort + k_pdq_sort_parts): the first
kernel stops after a few workgroup steps and hands its pending frames to part workgroups,
each of which finishes one range of positions and raises that range's ready flag; the
publisher waits for the parts a ticket reads.

* The sort alone (ca_go_sort_ranks_fan) against the oracle's sort.Slice, at the sizes where
  the hand-off changes shape: no frame pending, a short root, one step, several parts.
* Through the plan: every output mode, consecutive runs and a second plan on the mirror (the
  flags' epochs), equal to the oracle and byte-equal to the same plan with CASIM_SORT_FAN=0.

`arange(n)[::-1] % 300` has 300 distinct ranks, more than the LDS store's 256, so the entry
must refuse it (CA_EINVAL); the same decreasing runs modulo 250 go through the sort.
"""
import numpy as np
import pytest

from autoscaler_amd import abi, gosort, native
from estgen import _encode_estimate
import test_gpu_sort_share as ts
import test_gpu_table_chain as tc

pytestmark = pytest.mark.gpu

T_SMALL_FRAME = 2048            # csrc/pdqsort.h T_SMALL
SIZES = (0, 1, 13, 2048, 2049, 4100, 9000, 20000, 50368)
DISTINCT = (1, 2, 7, 64, 250)


@pytest.fixture(scope="module")
def oracle():
    import pyoracle
    pyoracle.build()
    return pyoracle


def _random(n, nk):
    return np.random.default_rng(1000 * nk + n).integers(0, nk, n)


def _sort_cases():
    """(name, ranks, limit)"""
    cases = [(f"random-{n}-{nk}", _random(n, nk), 0) for n in SIZES for nk in DISTINCT]
    rng = np.random.default_rng(7)
    for n in (2049, 4100, 20000):
        k = rng.integers(0, 50, n)
        s = np.sort(k)
        cases += [(f"sorted-{n}", s, 0), (f"reversed-{n}", s[::-1].copy(), 0)]
        near = s.copy()
        near[rng.integers(0, n, 4)] = rng.integers(0, 50, 4)
        cases.append((f"nearly-{n}", near, 0))
        cases.append((f"runs100-{n}", np.repeat(rng.integers(0, 60, n // 100 + 1), 100)[:n], 0))
        cases.append((f"decreasing-runs-{n}", np.arange(n)[::-1] % 250, 0))
        cases.append((f"heapsort-{n}", k, 2))
    return cases


@pytest.fixture(scope="module")
def sort_cases(oracle):
    """Every input with the oracle's permutation, computed once."""
    return [(name, r, limit, oracle.go_sort_desc(-np.asarray(r, np.float64), limit=limit))
            for name, r, limit in _sort_cases()]


@pytest.mark.parametrize("top_steps", [1, 4])
@pytest.mark.parametrize("parts", [2, 8])
def test_fanned_sort_matches_oracle(parts, top_steps, sort_cases):
    for name, r, limit, want in sort_cases:
        got, n_parts = native.go_sort_ranks_fan(np.asarray(r, np.uint32), parts=parts, top_steps=top_steps, limit=limit)
        assert np.array_equal(want, got), (name, parts, top_steps)
        assert 0 <= n_parts <= parts, (name, n_parts)
        if name.startswith("random-") and name.endswith("-64") and len(r) >= 9000:
            # the input's own premise first: two frames are pending at the hand-off
            lng, short = gosort.pending_frames(r, parts, top_steps, T_SMALL_FRAME)
            assert len(lng) + len(short) >= 2, (name, parts, top_steps)
            assert n_parts >= 2, (name, parts, top_steps, n_parts)


def test_more_than_256_ranks_is_refused():
    n = 4100
    with pytest.raises(native.CasimError) as e:
        native.go_sort_ranks_fan((np.arange(n)[::-1] % 300).astype(np.uint32))
    assert e.value.status == abi.CA_EINVAL
    with pytest.raises(native.CasimError):
        native.go_sort_ranks_fan(np.zeros(50369, np.uint32))


# ---- through the plan -------------------------------------------------------------------
L2100 = [("s1", 700), ("mb", 500), ("s3", 600), ("bottom", 300)]
L5000 = [("top", 900), ("s2", 1500), ("s3", 1400), ("bottom", 1200)]
L9000 = [("s1", 2500), ("s2", 2000), ("mc", 1500), ("s3", 1800), ("bottom", 1200)]
L120 = [("s2", 50), ("ma", 40), ("bottom", 30)]
MODES = ("nodes", "host32", "device", "u16")


@pytest.fixture(scope="module")
def inputs(oracle):
    """Five groups in four sort classes: groups 1 and 4 share (same list, templates that rank
    alike).  Encoded once; the oracle's result per limiter setting."""
    ps = ts.Pods(L2100, L5000, L9000, L120)
    lists = [ps.interleaved(x) for x in (L2100, L5000, L9000, L120)]
    groups = lists + [lists[1]]
    tm = [ts._tmpl(tc.T_MID)] * 4 + [ts._tmpl(tc.T_SMALL)]
    table, node_recs, tmr, off, pod_idx = _encode_estimate([], ps.all, tm, groups)
    # the premise of the part-count assertion: with the plan's defaults (8 parts, 4 steps) the
    # lists of 5,000 pods and more have two frames pending at the hand-off
    p = table.pods
    for g in (1, 2):
        idx = pod_idx[off[g]:off[g + 1]]
        score = (p["score_milli_cpu"][idx] / float(tmr[g]["node"]["alloc_milli_cpu"]) +
                 p["score_memory"][idx] / float(tmr[g]["node"]["alloc_memory"]))
        ranks = np.unique(-score, return_inverse=True)[1]
        lng, short = gosort.pending_frames(ranks, 8, 4, T_SMALL_FRAME)
        assert len(lng) + len(short) >= 2, (g, len(lng), len(short))
    want = {}
    for max_nodes in (0, 3):
        o = oracle.OracleState()
        o.clear()
        want[max_nodes] = o.estimate(table, off, pod_idx, tmr, max_nodes, 0)
    return table, tmr, off, pod_idx, len(groups), want


def _run_modes(plan, max_nodes, fan_on, what):
    out = {}
    for mode in MODES:
        if mode == "nodes":
            g = plan.run(max_nodes, 0, want_nodes=True)
        elif mode == "host32":
            g = plan.run(max_nodes, 0, want_nodes=False)
        elif mode == "device":
            g = plan.run(max_nodes, 0, device_results=True)
            g.sched_pod = plan.fetch()
        else:
            g = plan.run_u16(max_nodes, 0)
        st = plan.stats()
        assert st["decoupled"], (what, mode)
        assert st["sorts"] == 4, (what, mode, st)
        if mode in ("host32", "u16"):
            assert st["results_path"] == "published", (what, mode, st)
        if fan_on:
            assert st["sort_parts"] > st["sorts"], (what, mode, st)
        else:
            assert st["sort_parts"] == st["sorts"], (what, mode, st)
        out[mode] = g
    return out


@pytest.mark.parametrize("chunk", ["512", None])
@pytest.mark.parametrize("max_nodes", [0, 3])
def test_plan_with_fanned_sorts(max_nodes, chunk, inputs, monkeypatch):
    table, tm, off, pod_idx, G, want = inputs
    ro = want[max_nodes]
    monkeypatch.setenv("CASIM_SORT_FAN_MIN", "0")
    if chunk:
        monkeypatch.setenv("CASIM_PUB_CHUNK", chunk)         # tickets straddle part bounds
    m = native.Mirror(0)
    m.clear()
    raw = {}
    for fan in ("1", "0"):
        monkeypatch.setenv("CASIM_SORT_FAN", fan)            # (read when the plan is created)
        runs = []
        with native.EstimatePlan(m, table, off, pod_idx, tm) as plan:
            for r in range(3):
                runs.append(_run_modes(plan, max_nodes, fan == "1", (fan, r, max_nodes, chunk)))
            with native.EstimatePlan(m, table, off, pod_idx, tm) as second:    # a second plan, same mirror
                runs.append(_run_modes(second, max_nodes, fan == "1", (fan, "second", max_nodes, chunk)))
        for r, modes in enumerate(runs):
            for mode, g in modes.items():
                what = (fan, r, max_nodes, chunk, mode)
                tc._same(ro, g, off, G, what, nodes=mode == "nodes", u16=mode == "u16")
                blob = (g.results.tobytes(), np.asarray(g.sched_pod).tobytes(),
                        g.sched_node.tobytes() if mode == "nodes" else b"", g.last_index)
                if fan == "1":
                    raw[(r, mode)] = blob
                else:
                    assert raw[(r, mode)] == blob, what + ("fan off differs",)
    m.close()
