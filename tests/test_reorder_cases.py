"""The reorder cases can show the bug they are for, checked on the oracle without a device.

A reorder that did nothing (or a gather that forgot a column) would leave a scan answering for
the node that used to be at a position.  So for every non-identity case the FitsAnyNode
answers on an oracle loaded in the new order must differ, for some probe, from the answers on
the old order mapped through the permutation; and in the three planted clusters the field
that decides a probe lands in one device column only (NodeHot, NodeExt, NodeStatic)."""
import numpy as np
import pytest

import reordergen as R
import snapmodel as S
from autoscaler_amd import abi


def _mapped(old: list, inv: np.ndarray) -> list:
    """The old order's answers as the same scan would give them in the new order if the node
    order did not matter: the node through the permutation, the rest as it is."""
    return [(int(inv[a[0]]) if a[0] >= 0 else -1,) + tuple(a[1:]) for a in old]


def _answers(oracle_lib, c: R.Case, order, probes: abi.PodTable) -> list:
    o = oracle_lib.OracleState()
    R.load_fresh(o, c, order)
    out = R.probe_answers(o, probes, c.n)
    o.close()
    return out


@pytest.mark.parametrize("n", R.SIZES)
def test_cases_depend_on_the_order(n, oracle_lib):
    c = R.cluster(n)
    m = R.ReorderModel(c.table)
    R.load_fresh(oracle_lib.OracleState(), c, np.arange(n), m)
    probes = R.sample_probes(m)
    old = _answers(oracle_lib, c, np.arange(n), probes)
    assert any(a[0] >= 0 for a in old)
    seen = 0
    for kind in R.PERM_KINDS:
        net = R.compose(R.permutation(kind, n))
        if R.is_identity(net):
            continue
        seen += 1
        new = _answers(oracle_lib, c, net, probes)
        assert new != _mapped(old, R.inverse(net)), f"n={n} {kind}: no probe tells the orders apart"
    assert seen >= (8 if n > 65 else 5 if n >= 3 else n - 1)


@pytest.mark.parametrize("column", ["hot", "ext", "static"])
def test_planted_case_is_decided_by_one_column(column, oracle_lib):
    c, probes, fld = R.planted(column)
    n = c.n
    # the nodes are equal apart from that field and their name
    same = c.nodes.copy()
    for f in (fld if isinstance(fld, tuple) else (fld,)) + ("name_id",):
        same[f] = same[f][0]
    assert all(same[i].tobytes() == same[0].tobytes() for i in range(n))
    differs = c.nodes.copy()
    differs["name_id"] = 0
    assert len({differs[i].tobytes() for i in range(n)}) > 1
    # ... which is a field of that column alone (casim_internal.h: NodeHot holds the free cpu /
    # memory / ephemeral-storage / slots and the flags, NodeExt the extended resources and the
    # ports, NodeStatic taints, labels and the name); the flags of NodeHot are equal because
    # every node has an extended resource and a taint
    where = {"alloc_milli_cpu": "hot", "alloc_scalar": "ext", "taints": "static", "label_pairs": "static"}
    assert {where[f] for f in (fld if isinstance(fld, tuple) else (fld,))} == {column}
    assert (c.nodes["alloc_scalar"][:, S.SCALAR_COL] != 0).all() and (c.nodes["taints"] != 0).all()
    # every probe picks its node by that field: some probe has exactly one fitting node, and the
    # answers follow the permutation's positions, not the old ones
    old = _answers(oracle_lib, c, np.arange(n), probes)
    o = oracle_lib.OracleState()
    R.load(o, c)
    fits = S.backend_fits(o, S.Probes([probes.pods], [("pin", "pin")] * len(probes)), n)
    assert (fits.sum(axis=1) == 1).any() and fits.min() == 0
    for kind in ("reverse", "rot1", "rand0"):
        net = R.compose(R.permutation(kind, n))
        new = _answers(oracle_lib, c, net, probes)
        assert new != old, f"{column} {kind}: a column left in the old order gives the same answers"
        # the single-fit probes name the same node (by name) in both orders
        moved = 0
        for p in np.nonzero(fits.sum(axis=1) == 1)[0]:
            x = int(np.nonzero(fits[p])[0][0])
            got = new[int(p) * len(R.last_indexes(n))][0]
            assert got == int(R.inverse(net)[x])
            moved += int(got != x)
        assert moved > 0
