"""A model of the positions a publisher ticket waits for (csrc/estimate.hip, k_publish).

A chain walks its group's stream forwards.  A run of identical pods places a prefix of the
run in closed form and records one segment (dst, src, len): outputs [dst, dst + len) are
stream positions [src, src + len).  A pod stepped alone writes its own output (a single
placement) and records nothing.  Output chunk [a, b) of a group is published by a ticket that
carries the group's progress at the push (segments, pods scheduled, whether any pod was
stepped alone so far); the ticket waits for the sort parts that overlap the Go-order
positions [s0, s1) it reads:

* old rule: every position, [0, INT32_MAX);
* new rule: with no single step so far, from the first position read through the first
  segment that ends after `a` to the last read through the last segment that starts before
  min(b, n_sched); every position otherwise; nothing for a chunk past n_sched.

The model restates the kernel's two 64-probe searches and the range, and checks that the
range covers every position the chunk reads, is never wider than the old one (as a range
and as a mask of parts), and is exact at both ends.
"""
import numpy as np
import pytest

INT32_MAX = 2**31 - 1


def seg_lower(segs, nseg, key, from_dst):
    """k_publish's seg_lower: first segment of segs[:nseg] that ends after key (from_dst
    False) or starts at or after it (True); 64 evenly spaced probes per step."""
    lo, hi = 0, nseg
    while hi - lo > 0:
        span = hi - lo
        step = (span + 63) // 64
        f = -1
        for lane in range(64):
            i = lo + lane * step
            if i < hi:
                dst, _, ln = segs[i]
                if (dst >= key) if from_dst else (dst + ln > key):
                    f = lane
                    break
        if step == 1:
            return lo + f if f >= 0 else hi
        nlo = lo + (f - 1) * step + 1 if f > 0 else (lo if f == 0 else lo + ((span - 1) // step) * step + 1)
        hi = lo + f * step if f >= 0 else hi
        lo = nlo
    return lo


def ticket_range(segs, nseg, single, ns, a, b):
    """[s0, s1) of a segment ticket under the new rule."""
    end = min(b, ns)
    if single:
        return 0, INT32_MAX
    if end <= a:
        return 0, 0
    q0 = seg_lower(segs, nseg, a, False)
    q1 = seg_lower(segs, nseg, end, True)
    if q0 >= q1:
        return 0, INT32_MAX
    fd, fs, _ = segs[q0]
    ld, ls, ll = segs[q1 - 1]
    return fs - fd + max(a, fd), ls - ld + min(end, ld + ll)


def need_mask(lo, s0, s1):
    return sum(1 << j for j in range(len(lo) - 1) if lo[j] < s1 and lo[j + 1] > s0)


def walk(rng, n_pos, singles, short_runs):
    """A forward walk over n_pos stream positions: (segments, reads, first single output)."""
    segs, reads = [], []
    pos = 0
    first_single = None
    while pos < n_pos:
        if singles and rng.random() < 0.15:
            if rng.random() < 0.7:                          # placed: output len(reads) reads pos
                if first_single is None:
                    first_single = len(reads)
                reads.append(pos)
            elif first_single is None:
                first_single = len(reads)                   # stepped alone, not placed
            pos += 1
            continue
        run = int(rng.integers(1, 6 if short_runs else 400))
        run = min(run, n_pos - pos)
        placed = run if rng.random() < 0.5 else int(rng.integers(0, run + 1))
        if placed:
            segs.append((len(reads), pos, placed))
            reads.extend(range(pos, pos + placed))
        pos += run
    return segs, reads, first_single


def check_chunk(segs, reads, ns, lo, a, b, single, seen, what):
    end = min(b, ns)
    s0, s1 = ticket_range(segs, len(segs), single, ns, a, b)
    mine = reads[a:end]
    if not mine:
        seen["empty"] += 1
        if not single:
            assert (s0, s1) == (0, 0), what
        return
    assert s0 <= min(mine) and max(mine) < s1, (what, s0, s1, min(mine), max(mine))
    assert 0 <= s0 and s1 <= INT32_MAX                               # never wider than the old range
    old, new = need_mask(lo, 0, INT32_MAX), need_mask(lo, s0, s1)
    assert new & ~old == 0, what
    for pos in mine:                                                  # every position's part is needed
        j = max(k for k in range(len(lo) - 1) if lo[k] <= pos)
        assert lo[j + 1] > pos and new >> j & 1, (what, pos, lo, s0, s1)
    if single:
        assert new == old, what
        seen["every"] += 1
    else:
        assert s0 == mine[0] and s1 == mine[-1] + 1, what             # exact at both ends
        seen["exact"] += 1
        seen["narrower"] += new != old
        q0, q1 = seg_lower(segs, len(segs), a, False), seg_lower(segs, len(segs), end, True)
        seen["one"] += q1 - q0 == 1
    if end == ns and ns < b:
        seen["tail"] += 1


@pytest.mark.parametrize("singles", [False, True])
@pytest.mark.parametrize("short_runs", [False, True])
def test_range_covers_reads_and_is_never_wider(singles, short_runs):
    seen = {"empty": 0, "one": 0, "tail": 0, "exact": 0, "narrower": 0, "searched": 0, "every": 0}
    for seed in range(120):
        rng = np.random.default_rng(1000 * seed + 10 * singles + short_runs)
        n_pos = int(rng.integers(1, 5000))
        segs, reads, first_single = walk(rng, n_pos, singles, short_runs)
        count = n_pos
        ns = len(reads)
        pch = int(rng.choice([16, 64, 512]))
        parts = int(rng.integers(1, 17))
        lo = [0] + sorted(int(x) for x in rng.integers(0, n_pos + 1, parts - 1)) + [n_pos]
        if len(segs) > 64:
            seen["searched"] += 1
        for a in range(0, count, pch):
            b = min(count, a + pch)
            # the single-step flag a ticket can carry: set at the least when a pod was stepped
            # alone before the chunk was complete (the push comes after it), at the most
            # whenever the group steps one at all (a push delayed to the end of the chain)
            end = min(b, ns)
            at_end = end <= a or (end == ns and ns < b)               # pushed when the chain ends
            least = first_single is not None and (first_single < end or at_end)
            for single in sorted({least, first_single is not None}):
                check_chunk(segs, reads, ns, lo, a, b, single, seen, (seed, a, single))
    if not singles:
        assert min(seen[k] for k in ("empty", "one", "tail", "exact", "narrower")) > 0, seen
        if short_runs:
            assert seen["searched"] > 0, seen
    else:
        assert seen["empty"] and seen["tail"] and seen["every"] and seen["exact"], seen


def test_search_against_linear_scan():
    rng = np.random.default_rng(5)
    for nseg in (0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 5000):
        dst, segs = 0, []
        for _ in range(nseg):
            ln = int(rng.integers(1, 9))
            segs.append((dst, 3 * dst + 1, ln))
            dst += ln + int(rng.integers(0, 3))                      # (gaps: single placements)
        for key in sorted(set([0, 1, dst, dst + 1] + [int(x) for x in rng.integers(0, dst + 2, 60)])):
            ends = next((i for i, (d, _, ln) in enumerate(segs) if d + ln > key), nseg)
            starts = next((i for i, (d, _, ln) in enumerate(segs) if d >= key), nseg)
            assert seg_lower(segs, nseg, key, False) == ends, (nseg, key)
            assert seg_lower(segs, nseg, key, True) == starts, (nseg, key)
