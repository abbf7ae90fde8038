"""Planner cases planted at the structures the device chain (csrc/plan_chain.hip) is built
around, from raw ABI records: every free value, slot count, flag and hint is chosen.

A `Ring` holds the rows as the chain sees them (free cpu / memory / ephemeral storage / pod
slots per node, the unschedulable flag, taints, podDestinations); pods are put on nodes and
candidates list them; `build` turns that into node records whose allocatable is free + the
residents' requests (a ballast pod carries what a negative free value needs), so the rows
the kernel loads are the rows written here.  Every case has a name, the path it must take
("chain" / "speculative"), environment knobs it needs, and `claims`: what it is placed at,
in terms tests/test_chain_cases.py checks from numpy and the oracle's output alone:

  reasons {ci: reason}      dest {pod: node | -1}       n_placed {ci: k}
  evals_visible {ci: (L, x | None)}   evals of a one-pod candidate = visible nodes of the
                            ring walk from L to x (None: the whole ring), the candidate excluded
  last_index_in {ci: L}     last_index L                hints {pod: node}
  advance {ci: k}           ring distance a scan-only candidate moved lastIndex (n or n + 1)
  pareto {block: k}         distinct Pareto points of the block's visible rows with a free slot
  first_move {ci: k}        moves committed before the candidate (the staged-move totals)
  total_moves k             stops_at ci (the first NOT_RUN)
  blocking {ci: pod}        risky [ci]                  allowed [budgets afterwards]
  copies_moved k            moves whose pod is itself a copy made by this call

Most cases exist twice: with no ephemeral-storage request anywhere (EPH_COLS = false: the
per-block `eph` bit plane) and, named ".../eph", with one such pod in a move list
(EPH_COLS = true: the ephemeral column in LDS)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from autoscaler_amd import abi
from autoscaler_amd import workloads as W
from plangen import PlanCase

MI = 1 << 20
NO_PLACE, BLOCKED, UNEXPECTED = (abi.CA_UNREMOVABLE_NO_PLACE, abi.CA_UNREMOVABLE_BLOCKED_BY_POD,
                                 abi.CA_UNREMOVABLE_UNEXPECTED_ERROR)
OUT_OF_SCOPE, NOT_RUN = abi.CA_UNREMOVABLE_OUT_OF_SCOPE, abi.CA_UNREMOVABLE_NOT_RUN
INT32_MAX = (1 << 31) - 1
MAX_MOVED_PODS = 128               # include/casim.h CA_MAX_MOVED_PODS
FAIL = "fail"


@dataclass
class ChainCase(PlanCase):
    name: str = ""
    claims: dict = field(default_factory=dict)
    path: str = "chain"
    env: dict = field(default_factory=dict)


class Ring:
    def __init__(self, n: int, cpu: int = 0, mem: int = 0, slots: int = 0, eph: bool = False):
        self.n, self.eph = n, eph
        self.cpu = [cpu] * n
        self.mem = [mem] * n
        self.slots = [slots] * n
        self.ephfree = [(1 << 30) if eph else 0] * n
        self.flags = [0] * n
        self.taints = [0] * n
        self.scalar0 = [0] * n
        self.mask = np.ones(n, np.uint8)
        self.pods = []                 # dicts
        self.cands = []                # [node, pod ids | None, status]

    def row(self, i, cpu, mem, slots, eph=None, unsched=False, taint=0):
        self.cpu[i], self.mem[i], self.slots[i] = cpu, mem, slots
        if eph is not None:
            self.ephfree[i] = eph
        if unsched:
            self.flags[i] |= abi.CA_NODE_UNSCHEDULABLE
        self.taints[i] = taint

    def pod(self, node, cpu=0, mem=0, hint=-1, eph=0, tol=0, tol_unsched=False, pdbs=(), port=False,
            ext=False) -> int:
        self.pods.append(dict(node=node, cpu=cpu, mem=mem, hint=hint, eph=eph, tol=tol, tol_unsched=tol_unsched,
                              pdbs=sorted(pdbs), port=port, ext=ext))
        return len(self.pods) - 1

    def cand(self, node, pods=None, status=0) -> int:
        self.cands.append([node, pods, status])
        return len(self.cands) - 1

    def evict(self, node, shapes, **kw):
        """A candidate `node` whose pods to move are new pods of the given (cpu, mem) shapes."""
        ids = [self.pod(node, c, m, **kw) for c, m in shapes]
        return self.cand(node, ids), ids

    def build(self, name, claims, path="chain", L0=0, limit=0, allowed=(), env=None) -> ChainCase:
        n, pods = self.n, self.pods
        P = len(pods)
        off, moves = [0], []
        for node, ids, _ in self.cands:
            ids = [i for i, p in enumerate(pods) if p["node"] == node] if ids is None else ids
            moves.extend(ids)
            off.append(len(moves))
        if self.eph and moves:                      # one pod to move requests ephemeral storage
            first = next((i for i in moves if pods[i]["cpu"] > 0), moves[0])
            pods[first]["eph"] = 1
        used = np.zeros((n, 3), object)
        count = [0] * n
        for p in pods:
            used[p["node"]] += np.array([p["cpu"], p["mem"], p["eph"]], object)
            count[p["node"]] += 1
        ballast = []                                # (node, cpu, mem, eph)
        for i in range(n):
            need = [max(0, -(f + u)) for f, u in zip((self.cpu[i], self.mem[i], self.ephfree[i]), used[i])]
            k = max(0, -(self.slots[i] + count[i]), 1 if any(need) else 0)
            for b in range(k):
                ballast.append((i,) + tuple(need if b == 0 else [0, 0, 0]))
            if k:
                used[i] += np.array(need, object)
                count[i] += k
        nodes = abi.empty_nodes(n)
        for i in range(n):
            nodes[i]["alloc_milli_cpu"] = self.cpu[i] + used[i][0]
            nodes[i]["alloc_memory"] = self.mem[i] + used[i][1]
            nodes[i]["alloc_ephemeral"] = self.ephfree[i] + used[i][2]
            nodes[i]["alloc_pods"] = self.slots[i] + count[i]
            nodes["alloc_scalar"][i, 0] = self.scalar0[i]
            nodes[i]["flags"] = self.flags[i]
            nodes[i]["taints"] = self.taints[i]
            nodes[i]["name_id"] = i
        T = P + len(ballast)
        col = lambda k: np.array([p[k] for p in pods] + [0] * len(ballast), np.int64)      # noqa: E731
        cpu, mem, eph = col("cpu"), col("mem"), col("eph")
        for k, (_, c, m, e) in enumerate(ballast):
            cpu[P + k], mem[P + k], eph[P + k] = c, m, e
        rec = W.resource_pods(cpu, mem)
        rec["req_ephemeral"] = eph
        for i, p in enumerate(pods):
            rec["tolerated_taints"][i] = p["tol"]
            if p["tol_unsched"]:
                rec["flags"][i] |= abi.CA_POD_TOLERATES_UNSCHED
            if p["port"]:
                rec["port_conflict"][i, 0] = 1
                rec["port_use"][i, 0] = 1
            if p["ext"]:
                rec["req_scalar"][i, 0] = 1
                rec["flags"][i] |= abi.CA_POD_HAS_SCALAR_KEYS | abi.CA_POD_HAS_NONTPU_SCALAR_KEYS
        node_of = np.array([p["node"] for p in pods] + [b[0] for b in ballast], np.int32)
        hints = np.array([p["hint"] for p in pods] + [-1] * len(ballast), np.int32)
        pdb_off, pdb_pod = [0], []
        for i in range(T):
            pdb_pod.extend(pods[i]["pdbs"] if i < P else [])
            pdb_off.append(len(pdb_pod))
        if self.eph:
            name += "/eph"
        return ChainCase(nodes, abi.PodTable(rec), node_of, np.array([c[0] for c in self.cands], np.int32),
                         self.mask.copy(), np.array([c[2] for c in self.cands], np.int32), np.array(off, np.int32),
                         np.array(moves, np.int32), hints, L0, limit, np.array(allowed, np.int32),
                         np.array(pdb_off, np.int32), np.array(pdb_pod, np.int32), name=name, claims=claims,
                         path=path, env=dict(env or {}))


# ---------------------------------------------------------------------------
# ring and scan
# ---------------------------------------------------------------------------
POD = (100, 100 * MI)


def ring_fit(n: int, L0: int, x: int, eph: bool) -> ChainCase:
    """n >= 2 visible nodes with free slots and no room; node x has room for exactly POD.
    Candidate 0 is x itself with a larger pod: after its RemovePods x is the only row that
    fits it and x is excluded, so it fails after evaluating every other node and lastIndex
    stays the raw L0.  Candidate 1 (the next node) moves POD: the scan walks from L0 % n to x."""
    r = Ring(n, slots=4, eph=eph)
    r.row(x, *POD, 4)
    c0, _ = r.evict(x, [(150, 150 * MI)])
    y = (x + 1) % n
    c1, (p1,) = r.evict(y, [POD])
    L = L0 % n
    claims = dict(reasons={c0: NO_PLACE, c1: 0}, dest={p1: x}, n_placed={c0: 0, c1: 1},
                  evals_visible={c0: (L, None), c1: (L, x)}, last_index_in={c0: L0, c1: L0},
                  last_index=(x + 1) % n, structure=f"n={n} L0={L0} only fit at {x} (block {x >> 6} lane {x & 63})")
    return r.build(f"ring/n{n}-L{L0}-x{x}", claims, L0=L0)


RING_SIZES = (2, 63, 64, 65, 127, 128, 129)


def ring_points(n: int) -> list:
    """(L0, x): the only fit exactly at L and at L - 1 (the wrap block) for every L0 of the
    issue's list, node n - 1 of the (partial) last block, node 0 with L in the last block,
    and lanes 0 and 63 of a middle block."""
    pts = []
    for L0 in (0, 1, 63, 64, n - 1, n, n + 1, 3 * n - 1, INT32_MAX):
        L = L0 % n
        for x in (L, (L - 1) % n):
            if (L0, x) not in pts:
                pts.append((L0, x))
    pts += [(n - 1, 0), (0, n - 1), (1, n - 1)]
    if n >= 129:
        pts += [(1, 64), (1, 127), (n - 1, 64), (n - 1, 127)]
    return [p for i, p in enumerate(pts) if p not in pts[:i]]


def ring_single(eph: bool, moved: bool) -> ChainCase:
    """n = 1: the only node is the candidate.  An empty list is removable; a pod has no
    node to go to (NO_PLACE without one evaluation)."""
    r = Ring(1, cpu=1000, mem=1000 * MI, slots=4, eph=eph)
    if moved:
        c, (p,) = r.evict(0, [POD])
        return r.build("ring/n1-pod", dict(reasons={c: NO_PLACE}, evals={c: 0}, dest={p: -1}), L0=5)
    c = r.cand(0, [])
    return r.build("ring/n1-empty", dict(reasons={c: 0}, evals={c: 0}, total_moves=0), L0=5)


def ring_invisible(eph: bool) -> ChainCase:
    """vis != dest: nodes outside podDestinations and unschedulable nodes that would fit
    lie before the true fit; a pod that tolerates unschedulable nodes is hinted to one and
    takes it; a pod hinted to a node outside podDestinations is evaluated there and scans."""
    n = 130
    r = Ring(n, slots=4, eph=eph)
    for i in (3, 64, 65, 127, 128):
        r.row(i, 1000, 1000 * MI, 4)
    for i in (5, 66, 129):
        r.row(i, 1000, 1000 * MI, 4, unsched=True)
    r.mask[[3, 64, 65, 127, 7, 8, 63]] = 0
    c0, (p0,) = r.evict(10, [POD])                               # from 1: first visible fit is 128
    c1, (p1,) = r.evict(11, [POD], hint=66, tol_unsched=True)    # hinted to an unschedulable node: taken
    c2, (p2,) = r.evict(12, [POD], hint=64)                      # fits 64, which is no destination: scans
    c3, (p3,) = r.evict(13, [POD], hint=5)                       # does not tolerate: scans
    c4, (p4,) = r.evict(14, [POD], tol_unsched=True)             # unhinted: unschedulable nodes are not scanned
    claims = dict(reasons={c: 0 for c in (c0, c1, c2, c3, c4)}, dest={p0: 128, p1: 66, p2: 128, p3: 128, p4: 128},
                  evals_visible={c0: (1, 128)}, hints={p1: 66, p2: 128, p3: 128})
    return r.build("ring/invisible", claims, L0=1)


# ---------------------------------------------------------------------------
# probes against one block's skyline
# ---------------------------------------------------------------------------
CATCH = 128
FILL = (1, 1 << 54)


def probe_case(name, rows, probes, eph, claims=None, env=None, hosts=None) -> ChainCase:
    """192 nodes: block 0 hosts the candidates (rows without room or slots), block 1 holds
    `rows` ({node: (cpu, mem, slots[, eph])}), block 2 starts with the catch-all node 128 that
    fits everything.  Every probe is a candidate of its own: a list of (cpu, mem, expect[, hint])
    with expect a node, CATCH or FAIL (the candidate reverts).  A warm-up pod first walks the
    whole ring (every skyline gets built), and after every probe a filler that only the
    catch-all fits takes lastIndex back to 129: each probe's scan starts in block 2, loads
    block 0 (unknown: the candidate's own block) and meets block 1 through its skyline."""
    r = Ring(192, eph=eph)
    for i, v in rows.items():
        r.row(i, v[0], v[1], v[2], eph=v[3] if len(v) > 3 else None)
    r.row(CATCH, 1 << 40, 1 << 61, 4000)
    claims = dict(claims or {})
    dest, reasons = {}, {}
    host = 0

    def add(plist, at=None):
        nonlocal host
        if at is None:
            at, host = host, host + 1
        ids = [r.pod(at, p[0], p[1], hint=p[3] if len(p) > 3 else -1) for p in plist]
        c = r.cand(at, ids)
        failed = any(p[2] == FAIL for p in plist)
        reasons[c] = NO_PLACE if failed else 0
        for i, p in zip(ids, plist):
            dest[i] = -1 if failed else p[2]
        return c

    add([FILL + (CATCH,)])
    for k, plist in enumerate(probes):
        add(plist, (hosts or {}).get(k))
        add([FILL + (CATCH,)])
    assert host <= 64, name
    claims.update(dest=dest, reasons=reasons)
    return r.build(name, claims, L0=129, env=env)


def staircase(k: int, eph: bool) -> ChainCase:
    """Block 1 holds k Pareto points (cpu (i + 1) * 100, memory (k - i) * 100 MiB).  Probes:
    one unit above a point in each dimension (no fit), the hollow between two neighbouring
    middle points (under the bounding point once k >= 7: loaded, no fit, on to the catch-all),
    then the exact points (fit)."""
    pt = lambda i: ((i + 1) * 100, (k - i) * 100 * MI)      # noqa: E731
    rows = {64 + i: pt(i) + (2,) for i in range(k)}
    # (every point up to k = 7.  Of 64, block 0's 64 hosts allow 8: the five the builder keeps
    # exact (63, 0, 62, 1 and 61, the last one extracted one-ended), and three under the bound)
    idx = list(range(k)) if k <= 7 else [0, 1, 2, k // 2, k - 4, k - 3, k - 2, k - 1]
    probes = []
    for i in idx:
        c, m = pt(i)
        probes += [[(c + 1, m, CATCH)], [(c, m + 1, CATCH)]]
    if k >= 2:
        a, b = k // 2 - 1, k // 2
        probes.append([(pt(a)[0] + 50, pt(b)[1] + 50 * MI, CATCH)])
    probes += [[pt(i) + (64 + i,)] for i in idx]
    return probe_case(f"sky/stairs-{k}", rows, probes, eph, claims=dict(pareto={1: k}))


def skyline_cases(eph: bool) -> list:
    E31 = 1 << 31
    out = [staircase(k, eph) for k in (1, 2, 4, 5, 6, 7, 64)]
    big = (500, 500 * MI)
    out += [
        probe_case("sky/duplicates", {64: (300, 300 * MI, 1), 65: (300, 300 * MI, 1), 66: (100, 500 * MI, 1)},
                   [[(300, 300 * MI, 64)], [(300, 300 * MI, 65)], [(300, 300 * MI, CATCH)], [(100, 500 * MI, 66)]],
                   eph, claims=dict(pareto={1: 2})),
        probe_case("sky/front-is-back", {64: (100, 100 * MI, 2), 65: (500, 500 * MI, 2), 66: (200, 50 * MI, 2)},
                   [[(501, 80 * MI, CATCH)], [(150, 80 * MI, 65)], [(150, 20 * MI, 65)], [(150, 20 * MI, 66)]],   # (65: 2 slots)
                   eph, claims=dict(pareto={1: 1})),
        probe_case("sky/mem-round", {70: (10, 5 * MI + 1, 4)},
                   [[(10, 5 * MI + 2, CATCH)], [(10, 5 * MI + 1, 70)]], eph),
        probe_case("sky/mem-sign", {64: (1000, -1, 4), 65: (1000, 0, 4), 66: (1000, 1, 4)},
                   [[(10, 2, CATCH)], [(10, 1, 66)], [(10, 0, 65)], [(0, 0, 64)]], eph),
        probe_case("sky/cpu-2^31", {64: (E31 - 1, MI, 4), 65: (E31, MI, 4), 66: (E31 + 5, MI, 4)},
                   [[(E31 + 6, 1, CATCH)], [(E31 + 1, 1, 66)], [(E31, 1, 65)], [(E31 - 1, 1, 64)], [(E31 - 1, 1, CATCH)]],
                   eph),
        probe_case("sky/mem-2^51", {64: (10, (1 << 51) + MI, 4), 65: (10, (1 << 53) + 1, 4)},
                   [[(1, (1 << 53) + 2, CATCH)], [(1, (1 << 53) + 1, 65)], [(1, (1 << 51) + MI + 1, CATCH)],
                    [(1, (1 << 51) + MI, 64)]], eph),
        probe_case("sky/key-0", {64: (-E31, 1000 * MI, 4), 65: (-E31 - 7, 1000 * MI, 4)},
                   [[(0, MI, CATCH)], [(0, 0, 64)]], eph),
        probe_case("sky/no-slots", {64: (1000, 1000 * MI, 0), 65: (1000, 1000 * MI, -2)},
                   [[(0, 0, CATCH)], [(1, 1, CATCH)]], eph, claims=dict(pareto={1: 0})),
        probe_case("sky/negative-free-with-slots", {64: (1000, 1000 * MI, 0), 66: (-5, -5, 3)},
                   [[(0, 0, 66)], [(0, 1, CATCH)]], eph),
        # free ephemeral storage below 0 on a row that otherwise fits: the eph bit plane
        # (no ephemeral column) or the column itself rejects it
        probe_case("sky/eph-negative", {64: big + (4, -1), 65: big + (4,)}, [[big + (65,)]], eph),
        # an AddPod shrinks the block's only fitting row: the next pod of that shape passes the
        # stale point, loads the block, fails and rebuilds it; the third is skipped
        probe_case("sky/stale-add", {70: big + (4,)}, [[big + (70,)], [big + (CATCH,)], [big + (CATCH,)]], eph),
        # a committed removal whose node was its block's skyline front
        probe_case("sky/front-removed", {70: (900, 900 * MI, 4), 71: (50, 50 * MI, 4)},
                   [[(10, 10 * MI, 70)], [FILL + (CATCH,)], [(800, 800 * MI, CATCH)], [(10, 10 * MI, 71)]], eph,
                   hosts={1: 70}),
    ]
    # Revert: A is hinted onto row 70 (it shrinks), B passes 70's stale point, loads the block
    # without a fit and rebuilds it, C fits nowhere: the candidate reverts and row 70 grows back.
    # The next candidate's pod fits only row 70.
    revert = [[(100, 100 * MI, FAIL, 70), big + (FAIL,), (1 << 50, MI, FAIL)], [big + (70,)]]
    out.append(probe_case("sky/revert", {70: big + (4,)}, revert, eph))
    out.append(probe_case("sky/revert-helpers", {70: big + (4,)}, revert, eph, env={"CASIM_PLAN_HELP_AFTER": "1"}))
    return out


# ---------------------------------------------------------------------------
# the large ring: 67 blocks, a second skip window, both dirty words
# ---------------------------------------------------------------------------
def large_ring(eph: bool, help_after: bool = False) -> ChainCase:
    """4 225 nodes (67 blocks, the last of one node), lastIndex 69 (block 1).  The first
    three pods fit only in rotated block 64, rotated block 65 (a second skip window) and the
    last block.  Then a candidate hints two pods onto rows in blocks 63 and 64 (the last bit
    of dirty0, the first of dirty1), a third passes both stale points, rebuilds both blocks
    and lands in block 65, and a fourth fits nowhere: Revert grows the rows back.  The next
    candidate's pods fit only those rows."""
    n = 4225
    r = Ring(n, slots=2, eph=eph)
    # shapes no row of another shape fits
    s0, s1, s2, big, tiny = (300, 10 * MI), (200, 20 * MI), (100, 30 * MI), (500, 5 * MI), (100, MI)
    x63, x64, y = 63 * 64 + 3, 64 * 64, 65 * 64 + 9
    for i, shape in ((65 * 64 + 7, s0), (63 * 64 + 60, s1), (4224, s2), (x63, big), (x64, big), (y, big)):
        r.row(i, shape[0], shape[1], 2)
    c0, (p0,) = r.evict(10, [s0])                 # L 69 (block 1): rotated block 64 = block 65
    c1, (p1,) = r.evict(11, [s1])                 # L 4168 (block 65): rotated block 65 = block 63
    c2, (p2,) = r.evict(12, [s2])                 # L in block 63: the last block, lastIndex wraps to 0
    c3, ids = r.evict(13, [tiny, tiny, big, (1 << 50, MI)])
    r.pods[ids[0]]["hint"], r.pods[ids[1]]["hint"] = x63, x64
    c4, (d0, d1, d2) = r.evict(14, [big, big, big])
    claims = dict(reasons={c0: 0, c1: 0, c2: 0, c3: NO_PLACE, c4: 0},
                  dest={p0: 65 * 64 + 7, p1: 63 * 64 + 60, p2: 4224, d0: x63, d1: x64, d2: y, ids[2]: -1},
                  n_placed={c3: 3}, last_index_in={c3: 0}, rotated={p0: 64, p1: 65}, evals_visible={c0: (69, 65 * 64 + 7)})
    env = {"CASIM_PLAN_HELP_AFTER": "1"} if help_after else None
    return r.build("large/ring-4225" + ("-helpers" if help_after else ""), claims, L0=69, env=env)


# ---------------------------------------------------------------------------
# lists, copies, commit
# ---------------------------------------------------------------------------
SMALL = (1, MI)


def list_lengths(eph: bool) -> ChainCase:
    """Caller lists of 0, 1, 63, 64, 65, 127 and 128 pods, all removable."""
    r = Ring(192, eph=eph)
    for i in range(64, 192):
        r.row(i, 4, 4 * MI, 4)
    reasons, first, tot = {}, {}, 0
    for k, m in enumerate((0, 1, 63, 64, 65, 127, 128)):
        c, _ = r.evict(k, [SMALL] * m)
        reasons[c], first[c] = 0, tot
        tot += m
    return r.build("lists/lengths", dict(reasons=reasons, first_move=first, total_moves=tot), L0=70)


def list_129(eph: bool) -> ChainCase:
    r = Ring(192, eph=eph)
    for i in range(64, 192):
        r.row(i, 4, 4 * MI, 4)
    c0, _ = r.evict(0, [SMALL] * 5)
    c1, _ = r.evict(1, [SMALL] * 129)
    c2, _ = r.evict(2, [SMALL] * 2)
    c3, _ = r.evict(3, [])
    claims = dict(reasons={c0: 0, c1: OUT_OF_SCOPE, c2: NOT_RUN, c3: NOT_RUN}, stops_at=c2, last_index=69,
                  last_index_in={c1: 69, c2: 69, c3: 69}, total_moves=5)
    return r.build("lists/129", claims, L0=64)


def list_copies(eph: bool, copies: int) -> ChainCase:
    """100 caller pods on a node that an earlier commit gave 28 copies (128: in scope) or
    29 (the prefix cut)."""
    r = Ring(192, eph=eph)
    T = 5
    r.row(T, 40, 40 * MI, 40)
    for i in range(64, 192):
        r.row(i, 4, 4 * MI, 4)
    c0, _ = r.evict(0, [SMALL] * copies, hint=T)
    ids = [r.pod(T, *SMALL) for _ in range(100)]
    c1 = r.cand(T, ids)
    c2, _ = r.evict(1, [SMALL])
    if copies + 100 <= MAX_MOVED_PODS:
        claims = dict(reasons={c0: 0, c1: 0, c2: 0}, first_move={c1: copies}, total_moves=2 * copies + 101,
                      copies_moved=copies, n_placed={c1: 100 + copies})
    else:
        claims = dict(reasons={c0: 0, c1: OUT_OF_SCOPE, c2: NOT_RUN}, total_moves=copies, stops_at=c2)
    return r.build(f"lists/100+{copies}-copies", claims, L0=64)


def copy_chain(eph: bool) -> ChainCase:
    """A copy moved three times, A -> B -> C -> D; the returned hints cover the caller's pods."""
    r = Ring(8, slots=4, eph=eph)
    for i in (1, 2, 3):
        r.row(i, *POD, 4)
    ca, (p,) = r.evict(0, [POD], hint=1)
    cb, cc = r.cand(1, []), r.cand(2, [])
    claims = dict(reasons={ca: 0, cb: 0, cc: 0}, copies_moved=2, total_moves=3, hints={p: 1},
                  move_nodes=[1, 2, 3], n_placed={cb: 1, cc: 1})
    return r.build("lists/copy-chain", claims, L0=2)


def hinted_groups(eph: bool) -> ChainCase:
    """64 pods hinted to one node, and pods 60 to 70 of a list hinted to one node (the group
    straddles the two register halves); both nodes are candidates later, so the copies'
    slots are read back."""
    r = Ring(192, eph=eph)
    for i in range(64, 192):
        r.row(i, 4, 4 * MI, 4)
    r.row(70, 200, 200 * MI, 100)
    r.row(80, 200, 200 * MI, 100)
    c0, _ = r.evict(0, [SMALL] * 64, hint=70)
    c1, ids = r.evict(1, [SMALL] * 100)
    for t in range(60, 71):
        r.pods[ids[t]]["hint"] = 80
    c2, c3 = r.cand(70, []), r.cand(80, [])
    # (node 70's 64 copies scan on from 189, one node each: one of them lands on 80 and moves again)
    claims = dict(reasons={c0: 0, c1: 0, c2: 0, c3: 0}, copies_moved=76, n_placed={c2: 64, c3: 12},
                  dest={ids[t]: 80 for t in range(60, 71)})
    return r.build("lists/hinted-groups", claims, L0=100)


def odd_hints(eph: bool) -> ChainCase:
    """Hints to the candidate itself, outside podDestinations, to a node removed earlier in
    the call, to n and to n + 5 (the last two: unhinted, no evaluation)."""
    n = 70
    r = Ring(n, slots=4, eph=eph)
    for i in (30, 40, 66):
        r.row(i, 1000, 1000 * MI, 8)
    r.row(20, *POD, 1)
    r.mask[30] = 0
    c0, (a,) = r.evict(40, [POD])                          # node 40 leaves podDestinations
    c1, ids = r.evict(2, [POD] * 5)
    for t, h in enumerate((2, 30, 40, n, n + 5)):
        r.pods[ids[t]]["hint"] = h
    # from L0 = 10 pod a lands on 20; the hints to the candidate itself, to 30 and to 40 cost one
    # evaluation each and cannot be taken, n and n + 5 cost none.  The first scan walks 21 .. 66
    # (44 visible nodes: 30 and 40 are none) and every later one starts at 67 and walks the ring
    # round to 66 (3 + 67 nodes less the candidate, 30 and 40: 67).
    claims = dict(reasons={c0: 0, c1: 0}, dest={a: 20, **{i: 66 for i in ids}},
                  evals={c1: 3 + 44 + 4 * 67}, hints={i: 66 for i in ids})
    return r.build("lists/odd-hints", claims, L0=10)


def advance(eph: bool, extra: int) -> ChainCase:
    """A scan-only candidate whose lastIndex advance is exactly n (distinct destinations: the
    second pod lands one node before the start) or n + 1 (both pods on one node without any
    hint: the commit must group them).  A destination is the next candidate, so the copies'
    slots are read back: with both copies on node 0 its list is the two of them, the one that
    tolerates node 5's taint moves there and the other has no place (n_placed 1); with one
    copy on node 1, that copy moves to node 5."""
    n = 8
    r = Ring(n, slots=4, eph=eph)
    r.row(5, *POD, 4, taint=1)
    if extra:
        r.row(0, 200, 200 * MI, 4)
    else:
        r.row(1, *POD, 4)
        r.row(0, *POD, 4)
    c0, (p1, p2) = r.evict(4, [POD, POD])
    r.pods[p1]["tol"] = 1
    L0 = 0 if extra else 1
    c1 = r.cand(0 if extra else 1, [])
    dest = {p1: 0, p2: 0} if extra else {p1: 1, p2: 0}
    claims = dict(reasons={c0: 0, c1: NO_PLACE if extra else 0}, dest=dest, advance={c0: n + extra},
                  n_placed={c1: 1})
    return r.build(f"lists/advance-n+{extra}", claims, L0=L0)


def exact_slots(eph: bool) -> ChainCase:
    """A destination that receives exactly its free slots and is skipped from then on."""
    r = Ring(20, eph=eph)
    r.row(3, 1000, 1000 * MI, 3)
    r.row(9, 5, 5 * MI, 50)
    c0, ids = r.evict(0, [(10, 10 * MI)] * 3 + [SMALL] * 2)      # the first three fit only node 3
    c1, (q,) = r.evict(1, [SMALL])
    claims = dict(reasons={c0: 0, c1: 0}, dest={**{i: 3 for i in ids[:3]}, ids[3]: 9, ids[4]: 9, q: 9})
    return r.build("lists/exact-slots", claims, L0=2)


def twice(eph: bool) -> ChainCase:
    """The same candidate listed twice: it left podDestinations the first time."""
    r = Ring(20, eph=eph)
    r.row(9, 1000, 1000 * MI, 50)
    c0, _ = r.evict(4, [SMALL] * 2)
    c1 = r.cand(4, [])
    c2, _ = r.evict(5, [SMALL])
    return r.build("lists/twice", dict(reasons={c0: 0, c1: UNEXPECTED, c2: 0}), L0=0)


def twice_not_removed(eph: bool) -> ChainCase:
    """Candidates listed again after a first listing that did not remove them.  Node 6 takes a
    copy (hinted), then fails with its own pod, which fits nowhere; listed again with no pods
    of the caller's its list is that copy, which moves on to node 9; a third time it is no
    destination any more.  Node 7 is blocked by its status the first time and removable, with
    nothing to move, the second."""
    r = Ring(20, eph=eph)
    r.row(9, 1000, 1000 * MI, 50)
    r.row(6, *POD, 4)
    c0, (p,) = r.evict(4, [POD], hint=6)
    c1, (q,) = r.evict(6, [(1 << 40, MI)])
    c2 = r.cand(6, [])
    c3, _ = r.evict(7, [SMALL])
    r.cands[c3][2] = BLOCKED
    c4, c5 = r.cand(7, []), r.cand(6, [])
    claims = dict(reasons={c0: 0, c1: NO_PLACE, c2: 0, c3: BLOCKED, c4: 0, c5: UNEXPECTED}, dest={p: 6, q: -1},
                  n_placed={c1: 0, c2: 1, c4: 0}, copies_moved=1, move_nodes=[6, 9], first_move={c2: 1, c4: 2})
    return r.build("lists/twice-not-removed", claims, L0=0)


# ---------------------------------------------------------------------------
# scope edges
# ---------------------------------------------------------------------------
def scope_cases(eph: bool) -> list:
    out = []
    for slots, path in ((65535, "chain"), (65536, "speculative")):
        r = Ring(10, eph=eph)
        r.row(7, 1000, 1000 * MI, slots)
        c, _ = r.evict(0, [SMALL] * 3)
        out.append(r.build(f"scope/slots-{slots}", dict(reasons={c: 0}), path=path))
    r = Ring(10, eph=eph)
    r.row(7, 1000, 1000 * MI, 50)
    c0, ids = r.evict(0, [SMALL] * 3)
    c1 = r.cand(1, [ids[0]], status=BLOCKED)              # (never simulated: listing the pod is enough)
    out.append(r.build("scope/pod-under-two-candidates", dict(reasons={c0: 0, c1: BLOCKED}), path="speculative"))
    for kind in ("port", "ext"):
        r = Ring(10, eph=eph)
        r.row(7, 1000, 1000 * MI, 50)
        r.scalar0 = [100] * 10
        c0, ids = r.evict(0, [SMALL] * 3)
        r.pods[ids[1]][kind] = True
        out.append(r.build(f"scope/{kind}-pod", dict(reasons={c0: 0}), path="speculative"))
    return out


def lds_edge_case(n: int, eph: bool, cands=None) -> ChainCase:
    """n nodes with room everywhere, one one-pod candidate per listed node (default: node 0):
    the call the GPU test bisects the chain's LDS bound with, and runs on both sides of it."""
    cands = [0] if cands is None else cands
    r = Ring(n, cpu=1000, mem=1000 * MI, slots=8, eph=eph)
    reasons = {}
    for node in cands:
        c, _ = r.evict(node, [POD])
        reasons[c] = 0
    return r.build(f"scope/lds-{n}", dict(reasons=reasons), L0=n - 2)


# ---------------------------------------------------------------------------
# staging of results and moves
# ---------------------------------------------------------------------------
def staging_candidates(C: int, eph: bool, limit_at: int = 0, cut_at: int = -1) -> ChainCase:
    """C one-pod candidates on 200 nodes with mixed outcomes (a status, a pod that fits
    nowhere, an invalid node, removable).  limit_at: max_removable is chosen so that the
    loop stops at candidate limit_at; cut_at: that candidate lists 129 pods."""
    n = 200
    r = Ring(n, slots=0, eph=eph)
    r.row(n - 1, 1 << 30, 1 << 50, 4000)
    reasons, removed, limit = {}, 0, 0
    for c in range(C):
        node = c % (n - 1)
        if c >= n - 1:                                  # (C = 200: node 0 again, removed as candidate 0)
            r.cand(node, [])
            reasons[c] = UNEXPECTED if reasons[node] == 0 else reasons[node]
            continue
        if c == cut_at:
            r.evict(node, [SMALL] * 129)
            reasons[c] = OUT_OF_SCOPE
        elif c % 7 == 3:
            r.evict(node, [SMALL])
            r.cands[-1][2] = BLOCKED
            reasons[c] = BLOCKED
        elif c % 5 == 1:
            r.evict(node, [(1 << 40, MI)])
            reasons[c] = NO_PLACE
        else:
            r.evict(node, [SMALL] * (1 + c % 3))
            reasons[c] = 0
            removed += 1
        if c + 1 == limit_at:
            limit = removed
    claims = dict(reasons=reasons)
    name = f"staging/C{C}"
    if limit_at:
        assert reasons[limit_at - 1] == 0
        for c in range(limit_at, C):
            reasons[c] = NOT_RUN
        claims["stops_at"] = limit_at
        name += f"-limit-stops-at-{limit_at}"
    if cut_at >= 0:
        for c in range(cut_at + 1, C):
            reasons[c] = NOT_RUN
        claims["stops_at"] = cut_at + 1
        name += f"-cut-at-{cut_at}"
    return r.build(name, claims, L0=3, limit=limit)


def staging_moves(lists, eph: bool) -> ChainCase:
    """Candidates with the given list lengths, all removable: the staged moves stand at
    sum(lists[:-1]) before the last candidate."""
    n = 200
    r = Ring(n, eph=eph)
    for i in range(len(lists), n):
        r.row(i, 8, 8 * MI, 8)
    first, tot = {}, 0
    for k, m in enumerate(lists):
        c, _ = r.evict(k, [SMALL] * m)
        first[c] = tot
        tot += m
    claims = dict(reasons={c: 0 for c in range(len(lists))}, first_move=first, total_moves=tot)
    return r.build(f"staging/moves-{tot}-last-after-{tot - lists[-1]}", claims, L0=50)


# ---------------------------------------------------------------------------
# PDBs
# ---------------------------------------------------------------------------
def pdb_cases(eph: bool) -> list:
    out = []

    def ring():
        r = Ring(12, eph=eph)
        r.row(9, 1000, 1000 * MI, 200)
        r.row(10, 1000, 1000 * MI, 200)
        return r

    r = ring()                                            # a budget of 0 from the start
    c0, ids = r.evict(0, [SMALL] * 3)
    r.pods[ids[1]]["pdbs"] = [0]
    out.append(r.build("pdb/zero-budget", dict(reasons={c0: BLOCKED}, blocking={c0: ids[1]}, allowed=[0]),
                       allowed=[0]))
    r = ring()                                            # a budget of exactly the list's count
    c0, ids = r.evict(0, [SMALL] * 4, pdbs=[0])
    out.append(r.build("pdb/exact-budget", dict(reasons={c0: 0}, risky=[], allowed=[0]), allowed=[4]))
    r = ring()                                            # the lowest blocked PDB, not the first pod
    c0, ids = r.evict(0, [SMALL] * 3)
    r.pods[ids[0]]["pdbs"] = [1]
    r.pods[ids[2]]["pdbs"] = [0, 1]
    out.append(r.build("pdb/lowest-index", dict(reasons={c0: BLOCKED}, blocking={c0: ids[2]}), allowed=[0, 0]))
    r = ring()                                            # in two PDBs, only the lower one blocked
    c0, ids = r.evict(0, [SMALL] * 3)
    r.pods[ids[1]]["pdbs"] = [0, 1]
    out.append(r.build("pdb/two-pdbs-lower-blocked", dict(reasons={c0: BLOCKED}, blocking={c0: ids[1]}),
                       allowed=[0, 5]))
    r = ring()                                            # the blocking pod in the second half
    c0, ids = r.evict(0, [SMALL] * 70)
    r.pods[ids[66]]["pdbs"] = [1]
    r.pods[ids[69]]["pdbs"] = [1]
    out.append(r.build("pdb/second-half", dict(reasons={c0: BLOCKED}, blocking={c0: ids[66]}), allowed=[3, 0]))
    r = ring()                                            # the blocking pod is a copy (membership through orig)
    c0, (p,) = r.evict(0, [SMALL], hint=10, pdbs=[0])
    c1 = r.cand(10, [])
    out.append(r.build("pdb/copy-blocks", dict(reasons={c0: 0, c1: BLOCKED}, blocking_is_copy={c1: p}, allowed=[0]),
                       allowed=[1]))
    r = ring()                                            # two pods of one PDB, budget 1: risky; then negative
    c0, ids = r.evict(0, [SMALL] * 3)
    r.pods[ids[0]]["pdbs"] = [0]
    r.pods[ids[2]]["pdbs"] = [0]
    c1, (q,) = r.evict(1, [SMALL], pdbs=[0])
    c2, _ = r.evict(2, [SMALL])
    out.append(r.build("pdb/risky-then-negative",
                       dict(reasons={c0: 0, c1: BLOCKED, c2: 0}, risky=[c0], blocking={c1: q}, allowed=[-1]),
                       allowed=[1]))
    return out


# ---------------------------------------------------------------------------
# the bulk step
# ---------------------------------------------------------------------------
def bulk_case(name, n, L0, node, m, eph, edit=None, tol=0, claims=None) -> ChainCase:
    """Every node fits exactly one SMALL pod; candidate `node` moves m of them from L0."""
    r = Ring(n, cpu=1, mem=MI, slots=1, eph=eph)
    r.row(node, 0, 0, 0)
    if edit:
        edit(r)
    c, ids = r.evict(node, [SMALL] * m, tol=tol)
    cl = dict(reasons={c: 0})
    cl.update(claims(ids) if claims else {})
    return r.build("bulk/" + name, cl, L0=L0)


def bulk_cases(eph: bool) -> list:
    out = [bulk_case(f"places-{m}", 192, 64, 0, m, eph,
                     claims=lambda ids: dict(dest={p: 64 + t for t, p in enumerate(ids)})) for m in (1, 63, 64)]

    def miss(r):
        r.row(74, 0, 0, 1)
    out.append(bulk_case("miss-in-the-middle", 192, 64, 0, 30, eph, edit=miss,
                         claims=lambda ids: dict(dest={p: 64 + t + (t >= 10) for t, p in enumerate(ids)})))

    def two(r):
        for i in range(1, 40):
            r.row(i, 2, 2 * MI, 2)
    out.append(bulk_case("n-below-64", 40, 35, 0, 50, eph, edit=two,
                         claims=lambda ids: dict(dest={ids[0]: 35, ids[4]: 39, ids[5]: 1, ids[43]: 39, ids[44]: 1})))
    out.append(bulk_case("wraps-the-ring-end", 130, 120, 3, 30, eph,
                         claims=lambda ids: dict(dest={ids[9]: 129, ids[10]: 0, ids[12]: 2, ids[13]: 4})))
    out.append(bulk_case("window-holds-the-candidate", 192, 60, 63, 20, eph,
                         claims=lambda ids: dict(dest={ids[2]: 62, ids[3]: 64})))

    def invisible(r):
        r.mask[[66, 67]] = 0
        r.row(70, 1, MI, 1, unsched=True)
    out.append(bulk_case("window-holds-invisible-nodes", 192, 64, 0, 20, eph, edit=invisible,
                         claims=lambda ids: dict(dest={ids[1]: 65, ids[2]: 68, ids[3]: 69, ids[4]: 71})))

    def tainted(r):
        r.row(70, 1, MI, 1, taint=1)
    for tol, what in ((0, "not-tolerated"), (1, "tolerated"), ((1 << 64) - 1, "tolerates-all")):
        out.append(bulk_case(f"tainted-node-{what}", 192, 64, 0, 20, eph, edit=tainted, tol=tol,
                             claims=lambda ids, tol=tol: dict(dest={ids[5]: 69, ids[6]: 70 if tol else 71})))
    out.append(bulk_backoff(eph))
    return out


def bulk_backoff(eph: bool) -> ChainCase:
    """Candidates 0 and 1: bulk steps that place pods (open nodes 0..9).  Candidates 2 to 36 move
    one pod each over nodes 10..79, where full nodes alternate with open ones: lastIndex always
    stands on a full node, so 2, 3 and 4 start with a bulk step that places nothing and 5 to 36
    (32 candidates) skip it.  Candidate 37 is the first after the back-off: lastIndex 80 starts
    a stretch of open nodes and its re-armed bulk step places all 5 pods; 38 places 3 more.
    Node 88 is full: 39 misses again and places its 4 pods by a plain run, 40 hits again.
    `bulk` states this per candidate; the CPU test derives it from the oracle's output."""
    n = 200
    shape = (10, 10 * MI)
    r = Ring(n, slots=1, eph=eph)
    hosts = list(range(150, 200))
    open_nodes = list(range(0, 10)) + list(range(11, 80, 2)) + list(range(80, 88)) + list(range(89, 150))
    for i in open_nodes:
        r.row(i, *shape, 1)
    dest, reasons = {}, {}
    nxt = iter(open_nodes)
    sizes = [5, 5] + [1] * 35 + [5, 3, 4, 6]
    for k, m in enumerate(sizes):
        c, ids = r.evict(hosts[k], [shape] * m)
        reasons[c] = 0
        for p in ids:
            dest[p] = next(nxt)
    bulk = ["hit", "hit"] + ["miss"] * 3 + ["skipped"] * 32 + ["hit", "hit", "miss", "hit"]
    return r.build("bulk/back-off", dict(reasons=reasons, dest=dest, bulk=bulk), L0=0)


# ---------------------------------------------------------------------------
def _both(fn, *a, **kw) -> list:
    out = []
    for eph in (False, True):
        v = fn(*a, eph=eph, **kw)
        out.extend(v if isinstance(v, list) else [v])
    return out


def small_cases() -> list:
    """Every case of at most 200 nodes."""
    out = []
    for n in RING_SIZES:
        for L0, x in ring_points(n):
            out += _both(ring_fit, n, L0, x)
    out += _both(ring_single, moved=False) + _both(ring_single, moved=True) + _both(ring_invisible)
    out += _both(skyline_cases)
    out += _both(list_lengths) + _both(list_129) + _both(list_copies, copies=28) + _both(list_copies, copies=29)
    out += _both(copy_chain) + _both(hinted_groups) + _both(odd_hints) + _both(advance, extra=0)
    out += _both(advance, extra=1) + _both(exact_slots) + _both(twice) + _both(twice_not_removed)
    out += _both(scope_cases)
    for C in (1, 63, 64, 65, 128, 129, 200):
        out += _both(staging_candidates, C)
    for stop in (63, 64, 65):
        out += _both(staging_candidates, 130, limit_at=stop)
    for cut in (63, 64):
        out += _both(staging_candidates, 130, cut_at=cut)
    for lists in ([128, 128, 127, 128], [128, 128, 128, 128], [128, 128, 64, 65, 128], [128] * 8 + [1]):
        out += _both(staging_moves, lists)
    out += _both(pdb_cases) + _both(bulk_cases)
    return out


def large_cases() -> list:
    return [large_ring(False), large_ring(False, help_after=True), large_ring(True)]


_CACHE = {}


def all_cases() -> dict:
    """name -> case, built once (the tests only read them)."""
    if not _CACHE:
        for c in small_cases() + large_cases():
            assert c.name not in _CACHE, c.name
            _CACHE[c.name] = c
    return _CACHE
