"""bench.py's plain form and --dump-outputs: the helper on the CPU (a made-up result), and on
the GPU one small plain run whose line carries the headline alone and whose dumped arrays are
the CPU restatement's Estimate of the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from autoscaler_amd import abi, native
from autoscaler_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def _made_up(n_sched, off, sched, last_index):
    res = np.zeros(len(n_sched), abi.ESTIMATE_RESULT_DTYPE)
    res["n_scheduled"] = n_sched
    res["evals"] = np.arange(len(n_sched)) + (1 << 40)        # past float32's integers
    return native.EstimateOutput(res, sched, None, last_index), np.asarray(off, np.int32)


def test_dump_outputs_files(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    sched = np.array([7, 8, 0xFFFF, 0xFFFF, 0xFFFF, 1, 2, 3, 9], np.uint16)   # [8]: past group 2's count
    out, off = _made_up([2, 0, 3], [0, 4, 5, 9], sched, 17)
    bench.dump_outputs(str(tmp_path), out, off)
    got = _load(tmp_path)
    assert set(got) == {"results_" + f for f in abi.ESTIMATE_RESULT_DTYPE.names} | {"sched_pod", "last_index"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["sched_pod"].tolist() == [7, 8, -1, -1, -1, 1, 2, 3, -1]
    assert got["results_evals"].tolist() == [(1 << 40), (1 << 40) + 1, (1 << 40) + 2]
    assert got["last_index"].tolist() == [17]
    assert sched[8] == 9                                      # the caller's buffer is left alone
    # 32-bit pod ids give the same file
    out32, _ = _made_up([2, 0, 3], off, np.array([7, 8, -1, -1, -1, 1, 2, 3, 9], np.int32), 17)
    bench.dump_outputs(str(tmp_path / "i32"), out32, off)
    assert np.array_equal(_load(tmp_path / "i32")["sched_pod"], got["sched_pod"])


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 << 20)
    n = 1 << 20                                               # 8 MB as float64: over the limit
    out, off = _made_up([n], [0, n], np.arange(n, dtype=np.int32), 0)
    bench.dump_outputs(str(tmp_path / "a"), out, off)
    bench.dump_outputs(str(tmp_path / "b"), out, off)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 4 << 20
    assert 0 < a["sched_pod"].size < n and np.all(np.diff(a["sched_pod"]) > 0)
    assert all(np.array_equal(a[k], b[k]) for k in a) and a["results_evals"].tolist() == [1 << 40]


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, oracle_lib):
    size = dict(n_pods=2000, n_groups=8, n_existing=40, max_nodes=1000)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--pods", "2000", "--groups", "8", "--existing", "40", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "evals/s" and d["higher_is_better"] is True
    assert d["dtype"] == "int64" and d["ms_per_step"] > 0
    # the headline alone: nothing that takes runs of its own
    assert d["roofline"] is None and d["cpu_baseline"] is None
    assert set(d["extra"]) == {"estimate_latency_ms", "items_per_s", "evals_per_step", "rank0_groups"}

    w = W.c2(seed=42, **size)                                 # the batch bench.py builds from these arguments
    o = oracle_lib.OracleState()
    W.load_estimate(o, w)
    ro = o.estimate(w.table, w.group_off, w.pod_idx, w.templates, w.max_nodes, 0)
    got = _load(tmp_path)
    for f in abi.ESTIMATE_RESULT_DTYPE.names:
        assert np.array_equal(got["results_" + f], ro.results[f].astype(np.float64)), f
    assert got["last_index"].tolist() == [ro.last_index]
    assert d["extra"]["evals_per_step"] == int(ro.results["evals"].sum())
    assert d["value"] == pytest.approx(d["extra"]["evals_per_step"] / (d["ms_per_step"] / 1e3), rel=1e-9)
    assert len(got["sched_pod"]) == int(w.group_off[-1])
    for g in range(len(w.templates)):
        a, n, b = int(w.group_off[g]), int(ro.results[g]["n_scheduled"]), int(w.group_off[g + 1])
        assert np.array_equal(got["sched_pod"][a:a + n], ro.sched_pod[a:a + n]), g
        assert np.all(got["sched_pod"][a + n:b] == -1), g
