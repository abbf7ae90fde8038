"""The multi-GPU Estimate plan from the option matrix, without a device: the library's exports,
and shard.option_blocks (the Python statement of ca_multi_estimate_plan_create_options' split:
row totals of the matrix, their prefix sums, split_blocks of them) against the lists of
optgen.lists_of on every optgen case and on planted matrices."""
import ctypes as C

import numpy as np
import pytest

import optgen
from autoscaler_amd import abi, native, runonce, shard

WORLDS = (1, 2, 3, 5, 8)


def test_library_exports_the_sharded_option_constructors():
    lib = native.load()
    for f in ("ca_multi_estimate_plan_create_options", "ca_multi_estimate_plan_create_groups",
              "ca_multi_estimate_plan_fetch_lists", "ca_multi_estimate_plan_lists_ms"):
        assert hasattr(lib, f), f
        assert f in native.exported_symbols()
    out = (C.c_int32 * 32)()
    n = lib.ca_abi_struct_sizes(out, 32)
    assert list(out[:n]) == abi.EXPECTED_SIZES                         # additive: no record changed
    assert lib.ca_abi_version() == abi.CASIM_ABI_VERSION
    for name in ("from_options", "from_groups", "fetch_lists", "lists_ms"):
        assert callable(getattr(native.MultiEstimatePlan, name, None)), name
    # looked up on the class, as runonce.run does (the instance forwards unknown names to its mirror)
    for name in ("estimate_options", "build_pod_groups"):
        assert callable(getattr(runonce.ShardedMirror, name, None)), name


@pytest.mark.parametrize("name", optgen.CASE_NAMES)
def test_option_blocks_are_the_blocks_of_the_lists(name):
    _, _, eg_off, eg_pod, ok, _, _ = optgen.case(name)
    want_off, _ = optgen.lists_of(eg_off, eg_pod, ok)
    for world in WORLDS:
        group_off, blocks = shard.option_blocks(eg_off, ok, world)
        assert group_off.dtype == np.int32 and group_off.tobytes() == want_off.tobytes(), (name, world)
        assert blocks == shard.split_blocks(np.diff(want_off), world), (name, world)
        assert len(blocks) == world + 1 and blocks[0] == 0 and blocks[-1] == len(ok)


def _check(eg_off, ok, world, want_off, want_blocks):
    group_off, blocks = shard.option_blocks(eg_off, ok, world)
    assert group_off.tolist() == want_off
    assert blocks == want_blocks
    assert blocks == shard.split_blocks(np.diff(np.asarray(want_off)), world)


def test_option_blocks_on_planted_matrices():
    eg_off = np.array([0, 1, 1, 3], np.int32)                # groups of 1, 0 and 2 pods
    # all rows zero: every group is empty and weighs 1
    _check(eg_off, np.zeros((6, 3), np.uint8), 3, [0] * 7, [0, 2, 4, 6])
    # leading rows zero: block 0 holds empty groups only
    ok = np.zeros((6, 3), np.uint8)
    ok[4] = [1, 1, 0]                                        # 1 item
    ok[5] = [1, 0, 1]                                        # 3 items
    _check(eg_off, ok, 2, [0, 0, 0, 0, 0, 1, 4], [0, 4, 6])
    _check(eg_off, ok, 3, [0, 0, 0, 0, 0, 1, 4], [0, 3, 6, 6])
    # a flat matrix and a boolean one mean the same
    _check(eg_off, ok.reshape(-1), 2, [0, 0, 0, 0, 0, 1, 4], [0, 4, 6])
    _check(eg_off, ok.astype(bool), 2, [0, 0, 0, 0, 0, 1, 4], [0, 4, 6])
    # any nonzero verdict byte passes
    _check(eg_off, ok * 200, 2, [0, 0, 0, 0, 0, 1, 4], [0, 4, 6])
    # one node group under 5 ranks: one block, four empty ones behind it
    _check(eg_off, np.array([[1, 0, 1]], np.uint8), 5, [0, 3], [0, 1, 1, 1, 1, 1])
    # n_eg = 0
    _check(np.zeros(1, np.int32), np.zeros((4, 0), np.uint8), 2, [0, 0, 0, 0, 0], [0, 2, 4])
    # no node groups
    _check(eg_off, np.zeros((0, 3), np.uint8), 3, [0], [0, 0, 0, 0])


def test_option_blocks_refuses_a_total_beyond_int32():
    with pytest.raises(ValueError):
        shard.option_blocks(np.array([0, 70_000], np.int32), np.ones((40_000, 1), np.uint8), 2)


def test_sharded_mirror_does_not_gather_sched_node():
    sm = runonce.ShardedMirror(None, None, 0, 2)
    with pytest.raises(NotImplementedError):
        sm.estimate(None, [0], [], [], 0, want_nodes=True)
    with pytest.raises(NotImplementedError):
        sm.estimate_options(None, [0], [], [], [], 0, want_nodes=True)
