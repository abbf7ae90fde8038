"""Cases for ca_estimate_plan_option_price_sums (the price expander's totalPodPrice on the
resident Estimate lists).  As in tests/similargen.py every case is ONE pod table shared by all
its groups; a case also carries one price per pod of the table.

The expected totals are the in-order Python float sums over the CPU restatement's lists
(`in_order_sum`: a Python loop, one IEEE add per pod — np.sum is pairwise and would not do).

The cases are built so that a reordered sum shows.  Two orders of a float64 sum meet in the same
bits a good part of the time (the rounding errors of n adds walk some sqrt(n / 12) ulp apart:
about 40 % of random 8-pod lists, still a few per cent at 1000 pods), so random lists alone
cannot tell a kernel that adds in another order from one that adds in list order.  Hence:
  - the pods are "ranked" (similargen.ranked: pod i requests top - i milli cpu), so the Estimate
    score sort puts a group's pods in ascending pod-set index and the generator knows every list
    (and, on templates whose pod-count limit binds, every limited run's prefix of it);
  - each list of 8 or more pods is a seeded slice of a permutation, the first one drawn whose
    left-to-right sum differs in bytes from its right-to-left sum, from 64 strided lane partials
    combined by a tree, and from math.fsum (`pick_list`).
The uniform-class case cannot be built that way (its order among equal pods is Go's sort order);
its seed is chosen.  tests/test_price_cases.py checks all of it on the CPU restatement's lists.

Shared by the CPU test of the cases and the GPU test of the kernel.
"""
import copy
import math
import random
from dataclasses import dataclass, field

import numpy as np

import similargen as S
from autoscaler_amd import k8s, native
from estgen import _encode_estimate

GI, MI = S.GI, S.MI
CHUNK = native.PRICE_SUMS_CHUNK
SEED = 20261019

# list lengths of the edge case: every short length, and both sides of the powers of two up to
# 4096 (the kernel hands its chain native.PRICE_SUMS_CHUNK = 256 positions at a time, cut at
# multiples of 256 from the group's offset rounded down to 4)
EDGE_LENGTHS = list(range(0, 131)) + [191, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048,
                                      2049, 4095, 4096, 4097]
EDGE_PODS = 4100

# (templates whose pod-count limit binds for ranked pods: 110 x 4500 milli cpu fit one node)
T_WIDE = ("wide", 1000000, 4096 * GI, 110)
T_TEN = ("ten", 1000000, 4096 * GI, 10)
T_MID = ("mid", 8000, 16 * GI, 110)
T_SMALL = ("small", 4000, 8 * GI, 10)


@dataclass
class PriceCase:
    name: str
    pods: list
    templates: list                  # [(Node, [])] per group
    groups: list                     # [[Pod]] per group
    price: np.ndarray                # float64 per pod of `pods`
    index: dict                      # group name -> group index (named groups only)
    limits: tuple = (0,)             # max_nodes of the runs, in order
    built: dict = field(default_factory=dict)     # what the generator claims: (max_nodes, group index) -> list of ids

    def encode(self):
        """(table, templates, group_off, pod_idx)."""
        table, _, tm, off, idx = _encode_estimate([], self.pods, self.templates, self.groups)
        return table, tm, off, idx


def random_prices(rng, n):
    """Seeded random mantissas times 2^e, e uniform in [-20, 20]."""
    return np.array([math.ldexp(1.0 + rng.random(), rng.randint(-20, 20)) for _ in range(n)], np.float64)


def small_pods(n, prefix="p"):
    """n pods of a few hundred request shapes, all far below any template here."""
    return [k8s.build_test_pod(f"{prefix}{i}", 10 + i % 37, 16 * MI + (i % 11) * MI) for i in range(n)]


def _wide(n):
    return [(k8s.build_test_node(*T_WIDE), []) for _ in range(n)]


def shows_reordering(price, ids) -> bool:
    """A list the discrimination test counts (8 or more pods, only finite normal prices) must
    differ in bytes from all three reordered sums; any other list passes."""
    tiny = np.finfo(np.float64).tiny
    if len(ids) < 8 or not all(math.isfinite(price[i]) and abs(price[i]) >= tiny for i in ids):
        return True
    want = bits(in_order_sum(price, ids))
    return all(bits(f(price, ids)) != want for f in (reversed_sum, lane_tree_sum, fsum))


def pick_list(rng, price, pool, n, prefixes=()):
    """n ids of `pool` in ascending order (the list order of ranked pods): the first seeded slice
    of a permutation that shows a reordering, as a whole and cut to each length in `prefixes`
    (the list a limited run leaves)."""
    price = [float(x) for x in price]
    for _ in range(10000):
        ids = sorted(rng.sample(pool, n))
        if all(shows_reordering(price, ids[:k]) for k in (n,) + tuple(prefixes)):
            return ids
    raise AssertionError("no list of %d pods shows a reordering" % n)


def edges_case(seed=SEED):
    """One plan with every chunk edge: lists of length 0..130 and around every power of two up
    to 4096, each a slice of a seeded permutation of a 4100-pod table (pick_list), on templates
    that take 110 pods a node (every pod schedules).  The lengths are shuffled, so the groups'
    offsets take every residue mod 4 and mod 64."""
    rng = random.Random(seed)
    pods = S.ranked(EDGE_PODS)
    price = random_prices(rng, EDGE_PODS)
    while True:                                  # (a shuffle whose offsets take all 64 residues)
        lengths = list(EDGE_LENGTHS)
        rng.shuffle(lengths)
        offs = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        if len(set((offs % 64).tolist())) == 64 and len({int(a) % 4 for a, n in zip(offs, lengths) if n >= 64}) == 4:
            break
    built = {(0, g): pick_list(rng, price, range(EDGE_PODS), n) for g, n in enumerate(lengths)}
    groups = [[pods[i] for i in built[0, g]] for g in range(len(lengths))]
    index = {f"len{n}": g for g, n in enumerate(lengths)}
    return PriceCase("edges", pods, _wide(len(groups)), groups, price, index, built=built)


def _named_case(name, rng, pods, price, specs, fill, limits=(0,)):
    """specs: [(group name, pool of pod indices, n, template, wanted offset residue or None)];
    lists by pick_list, which also covers the prefix each limited run leaves (pods per node x
    max_nodes, on templates whose pod-count limit binds)."""
    named, picked = [], {}
    for gname, pool, n, tmpl, res in specs:
        prefixes = [tmpl[3] * lim for lim in limits if lim and tmpl[3] * lim < n]
        picked[gname] = pick_list(rng, price, pool, n, prefixes)
        named.append((gname, [pods[i] for i in picked[gname]], tmpl, res))
    groups, templates, index = S.layout(named, fill)
    built = {}
    for gname, ids in picked.items():
        tmpl = next(t for k, _, _, t, _ in specs if k == gname)
        for lim in limits:
            built[lim, index[gname]] = ids[:tmpl[3] * lim] if lim else ids
    return PriceCase(name, pods, templates, groups, price, index, limits=limits, built=built)


STALE_LIMIT = 1


def stale_case(seed=SEED + 1):
    """An unlimited run, then max_nodes = 1: lists of 700, 300 and 520 ids shrink to 110, 10 and
    110; behind them the buffer keeps the first run's ids."""
    rng = random.Random(seed)
    pods = S.ranked(800, top=1000)
    price = random_prices(rng, len(pods))
    specs = [("a", range(790), 700, T_WIDE, 1), ("ten", range(400), 300, T_TEN, 3), ("b", range(100, 790), 520, T_WIDE, 2)]
    return _named_case("stale", rng, pods, price, specs, pods[790:], limits=(0, STALE_LIMIT))


def slots_case(seed=SEED + 2):
    """Groups without a sum: an empty one, one whose pods fit no node (n_scheduled 0), one cut by
    the prefix protocol (CA_EUNSUPPORTED: a DoNotSchedule spread constraint) and the one after
    it (CA_ENOTRUN) — between groups that have one."""
    rng = random.Random(seed)
    pods = S.ranked(90, top=1000)
    huge = [k8s.build_test_pod(f"huge{i}", 9000000, 64 * MI) for i in range(2)]
    bad = k8s.build_test_pod("spread", 300, 64 * MI)
    bad.topology_spread.append(k8s.TopologySpreadConstraint(1, "kubernetes.io/hostname", "DoNotSchedule", {"app": "x"}))
    every = pods + huge + [bad]
    price = random_prices(rng, len(every))
    n = len(pods)
    specs = [("first", range(80), 40, T_WIDE, 1), ("empty", [], 0, T_WIDE, None), ("second", range(10, 80), 60, T_WIDE, None),
             ("huge", [n, n + 1], 2, T_WIDE, None), ("third", range(80), 9, T_WIDE, None),
             ("cut", [0, n + 2], 2, T_WIDE, None), ("after", range(80), 30, T_WIDE, None)]
    case = _named_case("slots", rng, every, price, specs, pods[80:])
    for k in ("huge", "cut", "after"):           # (no list: fits no node, out of scope, not run)
        case.built[0, case.index[k]] = []
    return case


# the planted specials: pod name -> price
SUBNORMALS = [5e-324, 1e-310, 2.5e-310]
SPECIALS = {
    "sub0": SUBNORMALS[0], "sub1": SUBNORMALS[1], "sub2": SUBNORMALS[2],
    "negzero0": -0.0, "negzero1": -0.0,
    "big0": 1e300, "big1": 1e300, "max0": 1e308, "max1": 1e308,      # 1e300 twice stays finite; with 1e308 twice: +inf
    "pinf": math.inf, "ninf": -math.inf,
    "nan": math.nan,
}


def specials_case(seed=SEED + 3):
    """Planted prices on pods that are scheduled: subnormals alone (the total stays subnormal)
    and beside normal prices, -0.0 alone (the total is +0.0), 1e300 twice (finite) and with 1e308
    twice (+inf), +inf and -inf in one list (NaN), a NaN, and a plain list.  (`big` and `overflow`
    hold only finite normal prices and give 2e300 and +inf in any order: the two lists of the
    cases that cannot show a reordering.)"""
    rng = random.Random(seed)
    normal = S.ranked(40, top=1000)
    special = {k: k8s.build_test_pod(k, 20, 16 * MI) for k in SPECIALS}
    sp = lambda *names: [special[k] for k in names]                                 # noqa: E731
    price = np.concatenate([random_prices(rng, len(normal)), np.array(list(SPECIALS.values()), np.float64)])
    plain = pick_list(rng, price, range(30), 24)
    named = [("subnormal", sp("sub0", "sub1", "sub2"), T_WIDE, 1),
             ("subnormal_mixed", normal[:9] + sp("sub1", "sub0"), T_WIDE, 2),
             ("negzero", sp("negzero0", "negzero1"), T_WIDE, 3),
             ("negzero_mixed", sp("negzero0") + normal[3:12], T_WIDE, None),
             ("big", sp("big0", "big1") + normal[:10], T_WIDE, None),
             ("overflow", sp("big0", "big1", "max0", "max1") + normal[:10], T_WIDE, None),
             ("infnan", sp("pinf", "ninf") + normal[:12], T_WIDE, None),
             ("pinf", sp("pinf") + normal[:12], T_WIDE, None),
             ("nan", sp("nan") + normal[10:30], T_WIDE, None),
             ("plain", [normal[i] for i in plain], T_WIDE, None)]
    groups, templates, index = S.layout(named, normal[30:])
    pods = normal + list(special.values())
    return PriceCase("specials", pods, templates, groups, price, index, built={(0, index["plain"]): plain})


def many_case(seed=SEED + 4, n_groups=300):
    """More options than a block or the launch's first blocks hold, most of them short (1 to 7
    pods), a few of several chunks spread among them."""
    rng = random.Random(seed)
    pods = S.ranked(1200, top=1500)
    price = random_prices(rng, len(pods))
    built = {}
    for g in range(n_groups):
        n = (3 * CHUNK + 17 + g) if g % 61 == 7 else 1 + (g * 5) % 7
        built[0, g] = pick_list(rng, price, range(len(pods)), n)
    groups = [[pods[i] for i in built[0, g]] for g in range(n_groups)]
    return PriceCase("many", pods, _wide(n_groups), groups, price, {}, built=built)


SHAPES = {"s2": k8s.build_test_pod("s2", 500, 1 * GI), "s3": k8s.build_test_pod("s3", 250, 512 * MI),
          "s1": k8s.build_test_pod("s1", 1000, 2 * GI)}


UNIFORM_SEED = SEED + 14     # (chosen: the eight lists of the case's two runs all show a reordering)


def uniform_case(seed=UNIFORM_SEED):
    """Pods of three shapes, deep-copied (uniform score classes: the run takes the decoupled Go
    order unless CASIM_GO_DECOUPLE=0): the list order among equal pods is Go's sort order, and
    the total follows it."""
    rng = random.Random(seed)
    by = {}
    for s, n in (("s2", 330), ("s3", 280), ("s1", 60)):
        by[s] = []
        for r in range(n):
            q = copy.deepcopy(SHAPES[s])
            q.name = q.uid = f"{s}-{r}"
            by[s].append(q)
    pods = [p for s in by for p in by[s]]
    named = [("a", by["s2"][:300] + by["s3"][:270], T_MID, 1), ("b", by["s3"] + by["s2"], T_MID, 2),
             ("c", by["s2"][40:] + by["s3"][::2], T_SMALL, 3), ("d", by["s1"], T_MID, None)]
    groups, templates, index = S.layout(named, by["s1"])
    return PriceCase("uniform", pods, templates, groups, random_prices(rng, len(pods)), index, limits=(0, 3))


def all_cases():
    return [edges_case(), stale_case(), slots_case(), specials_case(), many_case(), uniform_case()]


# -- the expected values and the sums they must differ from -----------------------------------
oracle_lists = S.oracle_lists


def in_order_sum(price, ids) -> float:
    """The reference's loop: totalPodPrice := 0.0; totalPodPrice += podPrice, left to right."""
    total = 0.0
    for i in ids:
        total += float(price[i])
    return total


def expected(price, lists) -> np.ndarray:
    return np.array([in_order_sum(price, ids) for ids in lists], np.float64)


def reversed_sum(price, ids) -> float:
    return in_order_sum(price, list(ids)[::-1])


def lane_tree_sum(price, ids, lanes=64) -> float:
    """64 strided per-lane partials combined by a shuffle-down tree."""
    part = [0.0] * lanes
    for k, i in enumerate(ids):
        part[k % lanes] += float(price[i])
    o = lanes // 2
    while o:
        for lane in range(o):
            part[lane] += part[lane + o]
        o //= 2
    return part[0]


def fsum(price, ids) -> float:
    try:
        return math.fsum(float(price[i]) for i in ids)
    except OverflowError:                       # (an intermediate sum past the largest float64)
        return math.inf


def bits(x) -> bytes:
    return np.float64(x).tobytes()
