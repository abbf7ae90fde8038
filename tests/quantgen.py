"""Estimate batches at the numeric edges the chain is built around, from raw ABI records.

Every case is a named batch: per group a template (alloc and used_* chosen so the free
values sit where the case wants them) and a list of (pod shape, count); the group's pods
get their own records, are shuffled with the case's own random.Random, and the batch is
run against a few existing nodes with a limiter and a starting lastIndex.

  quot-boundary  free = q*req - 1, q*req, q*req + 1 in one dimension (cpu, memory,
                 ephemeral-storage), q in {1, 2, 7, 109}, requests that are no powers of two
  quot-low       the same with requests whose float64 quotient is one short at q*req
  near-2^53      requests and free values 2^53 - 1, 2^53, 2^53 + 1: the first group stays on
                 the float64 quotient (every value below 2^53), the later ones leave it
  huge           free ~2^62, requests 2^40 .. 2^55 (uncapped quotients far above the cap);
                 every sum stays below 2^62
  zero-dim       free == 0 / free < 0 in a dimension the pod does not request, all-zero pods
                 on an overcommitted template, alloc_pods < used_pods
  pod-slots      alloc_pods 1 and 2^40; the slot limit binding before / after the resources
  score-edges    a score dimension skipped (alloc 0), scores one ulp apart, different
                 integers with equal float64 scores
  long-run       one run of 2^20 + 77 identical pods on two ~600k-pod nodes
  long-run-rows  a run of 2^20 + 777 pods that meets open rows, and one cut by the limiter

The same node shapes as mirror nodes (`row_cluster`) feed the kernels that apply AddPod
arithmetic to rows.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

import numpy as np

from autoscaler_amd import abi
from autoscaler_amd import workloads as W

E53 = 1 << 53
CPU_REQ, MEM_REQ, EPH_REQ = 333, (1 << 30) + 12345, 3 * (1 << 30) + 7      # no powers of two
# Requests r for which the float64 quotient falls short at free = q * r for every q used here:
# floor(fl(q * r) * fl(1 / r)) == q - 1, so the closed form needs its one step up
# (tests/test_edges_oracle.py checks this property of the numbers).
LOW_REQS = dict(cpu=347, mem=1261058521, eph=3221225491)
EXAMPLE_REQS = dict(cpu=CPU_REQ, mem=MEM_REQ, eph=EPH_REQ)
# Requests R just below 2^53 / q for which it overshoots at free = q * R - 1:
# floor(fl(q * R - 1) * fl(1 / R)) == q, one step down (q = 3 and 5)
HIGH_R3, HIGH_R5 = 3002399751579326, 1801439850947196
DIMS = ("cpu", "mem", "eph")
QS = (1, 2, 7, 109)


@dataclass
class Shape:
    cpu: int = 0
    mem: int = 0
    eph: int = 0
    score_cpu: int | None = None       # default: the requests (single-container pods)
    score_mem: int | None = None


@dataclass
class Group:
    template: np.ndarray               # one TEMPLATE_DTYPE record
    shapes: list                       # [(Shape, count)]
    reject: bool = False               # nothing of this group can be scheduled
    tag: str = ""


@dataclass
class QuantCase:
    name: str
    table: abi.PodTable
    group_off: np.ndarray
    pod_idx: np.ndarray
    templates: np.ndarray
    existing: np.ndarray
    max_nodes: int
    L0: int
    shape_of: np.ndarray               # per pod record: index into `shapes`
    shapes: list                       # every Shape of the batch
    groups: list = field(default_factory=list)

    def load(self, b) -> None:
        b.clear()
        if len(self.existing):
            b.add_nodes(self.existing)

    def args(self):
        return (self.table, self.group_off, self.pod_idx, self.templates, self.max_nodes, self.L0)


def template(free_cpu, free_mem, free_eph=0, slots=110, used=(100, 128 * W.MI, 1 << 30, 2), name_id=-1000):
    """A template whose free values (alloc - used_*) are the given ones."""
    ucpu, umem, ueph, upods = used
    upods = max(upods, -slots)                   # alloc_pods stays >= 0 when slots < 0
    t = W.make_template(free_cpu + ucpu, free_mem + umem, slots + upods, name_id=name_id)
    t["node"]["alloc_ephemeral"] = free_eph + ueph
    t["used_milli_cpu"], t["used_memory"], t["used_ephemeral"], t["used_pods"] = ucpu, umem, ueph, upods
    return t[0]


def existing_nodes(n: int) -> np.ndarray:
    e = abi.empty_nodes(n)
    e["alloc_milli_cpu"] = 8000
    e["alloc_memory"] = 32 << 30
    e["alloc_pods"] = 110
    e["name_id"] = np.arange(n)
    return e


def build_case(name: str, groups: list, n_existing: int = 3, max_nodes: int = 0, L0: int = 0, seed: int = 0,
               shuffle: bool = True) -> QuantCase:
    rng = random.Random(f"quantgen/{name}/{seed}")
    shapes, shape_of, off = [], [], [0]
    for g in groups:
        ids = []
        for s, count in g.shapes:
            shapes.append(s)
            ids.extend([len(shapes) - 1] * count)
        if shuffle:
            rng.shuffle(ids)
        shape_of.extend(ids)
        off.append(len(shape_of))
    shape_of = np.array(shape_of, np.int64)
    col = lambda f: np.array([f(s) for s in shapes], np.int64)[shape_of]      # noqa: E731
    pods = W.resource_pods(col(lambda s: s.cpu), col(lambda s: s.mem))
    pods["req_ephemeral"] = col(lambda s: s.eph)
    pods["score_milli_cpu"] = col(lambda s: s.cpu if s.score_cpu is None else s.score_cpu)
    pods["score_memory"] = col(lambda s: s.mem if s.score_mem is None else s.score_mem)
    pods["similar_class"] = shape_of                   # one controller per shape: uniform score classes
    templates = np.zeros(len(groups), abi.TEMPLATE_DTYPE)
    for i, g in enumerate(groups):
        templates[i] = g.template
        templates[i]["node"]["name_id"] = -1000 - i
    return QuantCase(name, abi.PodTable(pods), np.array(off, np.int32), np.arange(len(pods), dtype=np.int32),
                     templates, existing_nodes(n_existing), max_nodes, L0, shape_of, shapes, groups)


# ---------------------------------------------------------------------------
# quot-boundary
# ---------------------------------------------------------------------------
def boundary_free(q: int, dim: str, delta: int, req: dict = EXAMPLE_REQS) -> dict:
    """Template free values: q * req + delta in `dim`, room for q + 3 copies (and change)
    in the other two."""
    free = {d: (q + 3) * r + 17 for d, r in req.items()}
    free[dim] = q * req[dim] + delta
    return free


def quot_boundary(q: int, dim: str, req: dict = EXAMPLE_REQS) -> QuantCase:
    """Groups -1 / 0 / +1 over the same shapes: the boundary shape (shape 0 of each group,
    the highest score, requests in all three dimensions) fits q - 1, q, q times per node;
    two small fillers (one with a zero request in `dim`) take what is left."""
    n_big = {1: 230, 2: 300, 7: 700, 109: 2400}[q]
    groups = []
    for delta in (-1, 0, 1):
        f = boundary_free(q, dim, delta, req)
        fill = Shape(cpu=7, mem=1000003, eph=12347)
        setattr(fill, dim, 0)
        # (q == 1: the -1 variant schedules only the fillers; 100 slots make them open a second node)
        groups.append(Group(template(f["cpu"], f["mem"], f["eph"], slots=100 if q == 1 else 400),
                            [(Shape(req["cpu"], req["mem"], req["eph"]), n_big), (fill, 90), (Shape(5, 70001, 11), 60)],
                            tag=f"{delta:+d}"))
    name = "quot-boundary" if req is EXAMPLE_REQS else "quot-low"
    return build_case(f"{name}-q{q}-{dim}", groups, max_nodes=0, L0=(0, 5, 123)[q % 3], seed=q)


# ---------------------------------------------------------------------------
# near 2^53 and far above it
# ---------------------------------------------------------------------------
def near_2_53() -> QuantCase:
    third = (E53 - 1) // 3                       # 3 copies leave 1; third + 1 fits twice
    small = [(Shape(1 << 52, 12345), 70), (Shape((1 << 52) - 1, (1 << 52) - 1), 90), (Shape(E53 - 1, 1), 40),
             (Shape(third, third + 1, third), 120), (Shape(77, E53 - 1, 5), 30)]
    at = [(Shape(E53, 3), 40), (Shape(5, E53), 40), (Shape(third, 9, E53), 30)]
    above = [(Shape(E53 + 1, 3), 40), (Shape(5, E53 + 1, E53 + 1), 40)]
    u = (1, 1, 1, 0)                             # used_*: alloc = free + 1
    groups = [
        Group(template(E53 - 1, E53 - 1, E53 - 1, used=u), small, tag="f64"),             # every value < 2^53
        Group(template(E53, E53, E53, used=u), small + at, tag="bound==2^53"),            # leaves it: the bound
        Group(template(E53 + 1, E53 + 1, E53 + 1, used=u), small + at + above, tag="bound>2^53"),
        Group(template(E53 - 1, E53 - 1, E53 - 1, used=u), small + at + above, tag="req>=2^53"),   # per run
        Group(template(E53 - 1, 1 << 40, E53 + 1, used=u), [(Shape(third, 1 << 20, third), 200),
                                                            (Shape((1 << 52) + 1, 3, 1 << 52), 60)], tag="eph-bound"),
        # free = 3 R - 1 and 5 R - 1 below 2^53: the float64 quotient says 3 and 5, 2 and 4 fit
        Group(template(3 * HIGH_R3 - 1, 5 * HIGH_R5 - 1, 1 << 40, used=u),
              [(Shape(HIGH_R3, 7), 120), (Shape(9, HIGH_R5), 160), (Shape(HIGH_R3, HIGH_R5, 5), 40)], tag="f64 overshoot"),
    ]
    return build_case("near-2^53", groups, max_nodes=0, L0=7, seed=53)


def huge() -> QuantCase:
    big = (1 << 62) - (1 << 43) - 12345       # alloc = free + used stays below 2^62
    shapes = [(Shape((1 << 55) + 5, (1 << 40) + 3), 500), (Shape((1 << 40) + 3, (1 << 54) + 1), 700),
              (Shape((1 << 47) + 11, (1 << 47) + 13, (1 << 50) + 1), 400), (Shape(0, 0, (1 << 53) + 9), 300)]
    u = ((1 << 40) + 1, (1 << 41) + 1, 3, 1)
    groups = [
        Group(template(big, big >> 1, big, slots=1 << 40, used=u), shapes, tag="slots 2^40"),
        Group(template(big, big >> 1, big >> 3, slots=300, used=u), shapes, tag="slots 300"),
        Group(template(big >> 2, big, big, slots=4000, used=u), shapes[:2], tag="cpu 2^60"),
    ]
    return build_case("huge", groups, max_nodes=0, L0=3, seed=62)


# ---------------------------------------------------------------------------
# zero requests, zero and negative free values, pod slots
# ---------------------------------------------------------------------------
def zero_dim() -> QuantCase:
    cpu_only = [(Shape(cpu=300), 260), (Shape(cpu=70), 120)]
    zero = [(Shape(), 400)]
    groups = [
        Group(template(2000, 0, 0, slots=20), cpu_only, tag="free mem == 0"),
        Group(template(2000, -1, 0, slots=20), cpu_only, reject=True, tag="free mem == -1"),
        Group(template(2000, 0, -5, slots=20), cpu_only, reject=True, tag="free eph == -5"),
        Group(template(-100, -1, -7, slots=7), zero, tag="all-zero, overcommitted"),
        Group(template(-100, 4 << 30, 0, slots=7), zero + [(Shape(mem=1 << 20), 200)], tag="all-zero + mem-only"),
        Group(template(2000, 4 << 30, 0, slots=-3), cpu_only + zero, reject=True, tag="alloc_pods < used_pods"),
        Group(template(0, 3 * MEM_REQ, 0, slots=50), [(Shape(mem=MEM_REQ), 230), (Shape(eph=0, mem=12345), 90)],
              tag="free cpu == 0"),
    ]
    return build_case("zero-dim", groups, max_nodes=0, L0=1, seed=0)


def pod_slots() -> QuantCase:
    shapes = [(Shape(CPU_REQ, MEM_REQ), 180), (Shape(100, 1 << 20), 120)]
    nou = (0, 0, 0, 0)
    groups = [
        Group(template(50 * CPU_REQ, 50 * MEM_REQ, slots=1, used=nou), shapes[:1] + [(Shape(100, 1 << 20), 40)],
              tag="alloc_pods 1"),
        Group(template(50 * CPU_REQ, 50 * MEM_REQ, slots=1 << 40, used=nou), shapes, tag="alloc_pods 2^40"),
        Group(template(50 * CPU_REQ, 50 * MEM_REQ, slots=10), shapes, tag="slots bind first"),
        Group(template(10 * CPU_REQ + 5, 50 * MEM_REQ, slots=100), shapes, tag="resources bind first"),
        Group(template(1 << 40, 1 << 50, slots=(1 << 31) + 5, used=(0, 0, 0, 1 << 31)),
              [(Shape(1 << 30, 1 << 40), 2600)], tag="alloc_pods, used_pods > 2^31"),
    ]
    return build_case("pod-slots", groups, max_nodes=0, L0=0, seed=40)


# ---------------------------------------------------------------------------
# score edges
# ---------------------------------------------------------------------------
def score_skip() -> QuantCase:
    """alloc_milli_cpu == 0 (resp. alloc_memory == 0): the dimension adds nothing to the
    score (binpacking_estimator.go:176-185); free is 0 there, so only zero requests fit."""
    t_cpu0 = W.make_template(0, 64 << 30, 110)[0]
    t_mem0 = W.make_template(16000, 0, 110)[0]
    mem_only = [(Shape(mem=MEM_REQ, score_cpu=900), 300), (Shape(mem=3 * MEM_REQ, score_cpu=5), 200),
                (Shape(mem=1 << 28, score_cpu=100000), 150)]
    cpu_only = [(Shape(cpu=CPU_REQ, score_mem=1 << 40), 300), (Shape(cpu=3 * CPU_REQ, score_mem=7), 200),
                (Shape(cpu=50, score_mem=1 << 50), 150)]
    return build_case("score-skip", [Group(t_cpu0, mem_only, tag="alloc cpu 0"),
                                     Group(t_mem0, cpu_only, tag="alloc mem 0"),
                                     Group(t_cpu0, cpu_only, reject=True, tag="alloc cpu 0, cpu pods")],
                      max_nodes=0, L0=2, seed=1)


def score_ulp() -> QuantCase:
    """alloc_milli_cpu 2^52: score_milli_cpu 2^52 and 2^52 + 1 score 1.0 and 1.0 + 2^-52."""
    t = template(4000, 16 << 30, used=((1 << 52) - 4000, 0, 0, 0))
    assert int(t["node"]["alloc_milli_cpu"]) == 1 << 52
    shapes = [(Shape(500, 1 << 30, score_cpu=1 << 52, score_mem=0), 300),
              (Shape(700, 1 << 29, score_cpu=(1 << 52) + 1, score_mem=0), 300),
              (Shape(300, 1 << 28, score_cpu=(1 << 52) - 1, score_mem=0), 200)]
    return build_case("score-ulp", [Group(t, shapes), Group(t, shapes[::-1])], max_nodes=0, L0=0, seed=2)


def score_tie() -> QuantCase:
    """score_milli_cpu 2^53 and 2^53 + 1: different integers, one float64, so two classes
    tie on every template and Go's pdqsort mixes their pods."""
    t = template(4000, 16 << 30, used=((1 << 60) - 4000, 0, 0, 0))
    shapes = [(Shape(500, 1 << 30, score_cpu=E53, score_mem=0), 700),
              (Shape(700, 1 << 29, score_cpu=E53 + 1, score_mem=0), 700),
              (Shape(300, 1 << 28, score_cpu=E53 + 2, score_mem=0), 300),
              (Shape(900, 1 << 27, score_cpu=E53 - 1, score_mem=0), 300)]
    t2 = template(6000, 8 << 30, used=(0, 0, 0, 0))
    return build_case("score-tie", [Group(t, shapes), Group(t2, shapes)], max_nodes=0, L0=5, seed=3)


# ---------------------------------------------------------------------------
# long-run
# ---------------------------------------------------------------------------
LONG_RUN_PODS = (1 << 20) + 77


def long_run(max_nodes: int) -> QuantCase:
    """2^20 + 77 identical pods (cpu 1, mem 3), each with its own record, on a template that
    holds 600000 of them (cpu 700001, mem 1800002, 2^20 pod slots).  The group is one run
    that starts with no node open: the closed-form opening computes the template's copy
    count with more than 2^20 pods left (the integer path) and opens two nodes (one under
    max_nodes 1), and the group is longer than 2^20 (the sort's global-store mode)."""
    t = template(700001, 1800002, slots=1 << 20, used=(0, 0, 0, 0))
    return build_case("long-run", [Group(t, [(Shape(1, 3), LONG_RUN_PODS)])], n_existing=2, max_nodes=max_nodes,
                      L0=1, shuffle=False)


LONG_ROWS_PODS = (1 << 20) + 777
LONG_ROWS_MAX_NODES = 4


def long_run_rows() -> QuantCase:
    """A run longer than 2^20 that meets open rows, under a limiter of 4 nodes per group.

    Group 0: three pods of (cpu 400000, mem 3) score highest and open one node each (one fits
    a node); the run of 2^20 + 777 pods of (cpu 1, mem 3) then starts with three rows that
    have room for 300001 copies each and all of it still to place: the scan over rows with
    more than 2^20 pods left (integer copy counts, their 64-bit sum, several rows alive).
    Group 1: the same run alone on a template that holds 50: the limiter lets the run open
    four nodes at once (200 pods), more than 2^20 are left, and the check of the last row
    runs with every other row exhausted.  Both groups list the same pod records."""
    n = LONG_ROWS_PODS
    pods = W.resource_pods(np.concatenate([np.full(3, 400000), np.ones(n, np.int64)]), np.full(n + 3, 3))
    shape_of = np.concatenate([np.zeros(3, np.int64), np.ones(n, np.int64)])
    pods["similar_class"] = shape_of
    big = template(700001, 1800002, slots=1 << 20, used=(0, 0, 0, 0))
    small = template(50, 1800002, slots=1 << 20, used=(0, 0, 0, 0))
    templates = np.zeros(2, abi.TEMPLATE_DTYPE)
    templates[0], templates[1] = big, small
    templates["node"]["name_id"] = [-1000, -1001]
    pod_idx = np.concatenate([np.arange(n + 3), np.arange(3, n + 3)]).astype(np.int32)
    shapes = [Shape(400000, 3), Shape(1, 3)]
    groups = [Group(big, [(shapes[0], 3), (shapes[1], n)], tag="open rows"),
              Group(small, [(shapes[1], n)], tag="limiter cut")]
    return QuantCase("long-run-rows", abi.PodTable(pods), np.array([0, n + 3, 2 * n + 3], np.int32), pod_idx, templates,
                     existing_nodes(2), LONG_ROWS_MAX_NODES, 1, shape_of, shapes, groups)


def small_cases() -> dict:
    """name -> builder of every case but long-run."""
    cases = {f"quot-boundary-q{q}-{d}": (lambda q=q, d=d: quot_boundary(q, d)) for q in QS for d in DIMS}
    cases.update({f"quot-low-q{q}-{d}": (lambda q=q, d=d: quot_boundary(q, d, LOW_REQS)) for q in QS for d in DIMS})
    cases.update({"near-2^53": near_2_53, "huge": huge, "zero-dim": zero_dim, "pod-slots": pod_slots,
                  "score-skip": score_skip, "score-ulp": score_ulp, "score-tie": score_tie})
    return cases


# ---------------------------------------------------------------------------
# the same node shapes as mirror rows
# ---------------------------------------------------------------------------
@dataclass
class RowCluster:
    nodes: np.ndarray                  # NODE_DTYPE
    table: abi.PodTable                # residents first (placed in order), then the pending pods
    n_resident: int
    node_of: np.ndarray                # node position of every resident
    templates: np.ndarray              # the same shapes as templates (ca_check_templates)

    def load(self, b) -> None:
        b.clear()
        b.add_nodes(self.nodes)
        b.add_pods(self.table, np.arange(self.n_resident, dtype=np.int32), self.node_of)

    @property
    def pending(self) -> np.ndarray:
        return np.arange(self.n_resident, len(self.table), dtype=np.int32)


def row_cluster(seed: int = 0) -> RowCluster:
    """At most 64 nodes and 400 pods: the quot-boundary, zero-dim and near-2^53 node shapes,
    each node's used_* carried by one resident pod, and pending pods of the shapes that sit
    on the boundaries (in runs, so several land on one row one after another)."""
    rng = random.Random(f"quantgen/rows/{seed}")
    specs = []                                    # (free cpu, mem, eph, slots)
    for q in (1, 2, 7):
        for d in DIMS:
            for delta in (-1, 0, 1):
                f = boundary_free(q, d, delta, LOW_REQS)
                specs.append((f["cpu"], f["mem"], f["eph"], 40))
    specs += [(2000, 0, 0, 20), (2000, -1, 0, 20), (2000, 0, -5, 20), (-100, -1, -7, 7), (0, 3 * MEM_REQ, 0, 50),
              (2000, 4 << 30, 0, -1), (2000, 4 << 30, 0, 0),
              (E53 - 1, E53 - 1, E53 - 1, 30), (E53, E53, E53, 30), (E53 + 1, E53 + 1, E53 + 1, 30),
              (E53 - 1, 1 << 40, E53 + 1, 30)]
    rng.shuffle(specs)
    n = len(specs)
    assert n <= 64
    used = (100, 128 * W.MI, 1 << 30)
    nodes = abi.empty_nodes(n)
    templates = np.zeros(n, abi.TEMPLATE_DTYPE)
    res = W.resource_pods(np.full(n, used[0]), np.full(n, used[1]))
    res["req_ephemeral"] = used[2]
    for i, (fc, fm, fe, slots) in enumerate(specs):
        # the resident is the node's one pod: slots -1 is alloc_pods 0 below used_pods 1
        templates[i] = template(fc, fm, fe, slots=slots, used=used + (1,), name_id=-1000 - i)
        nodes[i] = templates[i]["node"]
        nodes[i]["name_id"] = i
    third = (E53 - 1) // 3
    lo = LOW_REQS
    pend_shapes = [Shape(lo["cpu"], lo["mem"], lo["eph"])] * 6 + [
        Shape(cpu=300), Shape(), Shape(mem=MEM_REQ), Shape(cpu=lo["cpu"], eph=lo["eph"]), Shape(7, 0, 12347),
        Shape(1 << 52, 12345), Shape((1 << 52) - 1, (1 << 52) - 1), Shape(E53 - 1, 1), Shape(E53, 3),
        Shape(5, E53 + 1, E53 + 1), Shape(third, third + 1, third), Shape(third, 9, E53)]
    seq = []
    while len(seq) < 400 - n:
        seq.extend([rng.randrange(len(pend_shapes))] * rng.choice([1, 2, 3, 8]))
    seq = seq[:400 - n]
    col = lambda f: np.array([f(pend_shapes[s]) for s in seq], np.int64)      # noqa: E731
    pend = W.resource_pods(col(lambda s: s.cpu), col(lambda s: s.mem))
    pend["req_ephemeral"] = col(lambda s: s.eph)
    pend["similar_class"] = np.array(seq)
    return RowCluster(nodes, abi.PodTable(np.concatenate([res, pend])), n, np.arange(n, dtype=np.int32), templates)


def filled_rows(seed: int = 0, frac: float = 0.55) -> RowCluster:
    """row_cluster with the first `frac` of its pending pods already placed (first fit in
    plain integers, NodeResourcesFit's rule), so the rows' free values sit between the
    boundaries and 0: the state the scale-down kernels move pods between."""
    rc = row_cluster(seed)
    n = len(rc.nodes)
    p = rc.table.pods
    free = [[int(rc.nodes[i][f]) - u for f, u in zip(("alloc_milli_cpu", "alloc_memory", "alloc_ephemeral"),
                                                      (100, 128 * W.MI, 1 << 30))] + [int(rc.nodes[i]["alloc_pods"]) - 1]
            for i in range(n)]
    k = rc.n_resident + int(frac * (len(p) - rc.n_resident))
    keep, node_of = list(range(rc.n_resident)), list(range(n))
    rest = []
    for i in range(rc.n_resident, len(p)):
        req = [int(p[i]["req_milli_cpu"]), int(p[i]["req_memory"]), int(p[i]["req_ephemeral"])]
        dest = -1
        if i < k:
            for j in range(n):
                f = free[j]
                if f[3] >= 1 and (not any(req) or all(r <= x for r, x in zip(req, f))):
                    dest = j
                    break
        if dest < 0:
            rest.append(i)
            continue
        for d in range(3):
            free[dest][d] -= req[d]
        free[dest][3] -= 1
        keep.append(i)
        node_of.append(dest)
    order = keep + rest
    return RowCluster(rc.nodes, abi.PodTable(p[order]), len(keep), np.array(node_of, np.int32), rc.templates)
