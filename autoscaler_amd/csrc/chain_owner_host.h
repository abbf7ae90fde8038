// Index arithmetic of the lean Estimate chain (estimate.hip, k_ffd_chain<.., TB, LEAN>) that needs
// no GPU to be checked: which wave owns a 64-row block, the rows of a closed-form opening that a
// wave writes, the t-th qualifying row from per-block counts, the rotated-order rank as a
// row-order rank, and the float64 copy count of a resource-only pod on a row (the run table's
// fresh-copy constant).  Compiles for host and device; tests/host/chain_owner_host_check.cpp
// builds it with the host sanitizers and runs it on a CPU.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CASIM_HD __host__ __device__ inline
#else
#define CASIM_HD inline
#endif

namespace casim {

// ---- ownership: 64-row block b belongs to wave b & (cw - 1) for the whole kernel (cw: the
// workgroup's waves, a power of two), whatever the row count k is ----
CASIM_HD int32_t co_blocks(int32_t k) { return (k + 63) >> 6; }
CASIM_HD int co_owner(int32_t b, int cw) { return (int)(b & (cw - 1)); }
// the i-th block of wave wv (i = 0, 1, ...), and how many of the blocks of k rows it owns
CASIM_HD int32_t co_wave_block(int wv, int32_t i, int cw) { return wv + i * cw; }
CASIM_HD int32_t co_wave_blocks(int32_t k, int wv, int cw) {
    const int32_t nb = co_blocks(k);
    return nb > wv ? (nb - wv + cw - 1) / cw : 0;
}
// the first block >= bmin that wave wv owns
CASIM_HD int32_t co_first_block(int32_t bmin, int wv, int cw) { return bmin + ((wv - bmin) & (cw - 1)); }
// rows of the opening [k0, k0 + n) that lie in block b: [lo, hi), empty when hi <= lo.  A wave
// writes these for b = co_first_block(k0 >> 6, wv, cw), + cw, ... while b * 64 < k0 + n.
CASIM_HD void co_open_rows(int32_t k0, int32_t n, int32_t b, int32_t& lo, int32_t& hi) {
    const int32_t b0 = b << 6, e = k0 + n;
    lo = k0 > b0 ? k0 : b0;
    hi = e < b0 + 64 ? e : b0 + 64;
}

// ---- the t-th qualifying row (t >= 1) in row order from per-block counts: block b holds it iff
// excl(b) < t <= incl(b) with incl the inclusive prefix of the counts; it is the
// (t - excl(b))-th qualifying row of that block ----
CASIM_HD bool co_block_holds(int32_t incl, int32_t cnt, int32_t t) { return incl - cnt < t && t <= incl; }
CASIM_HD int32_t co_rank_in_block(int32_t incl, int32_t cnt, int32_t t) { return t - (incl - cnt); }
// the same over an array (the kernel: one lane per block, incl from a scan over the lanes);
// -1 when fewer than t rows qualify
CASIM_HD int32_t co_find_block(const int32_t* cnt, int32_t nb, int32_t t, int32_t& rank) {
    int32_t incl = 0;
    for (int32_t b = 0; b < nb; b++) {
        incl += cnt[b];
        if (co_block_holds(incl, cnt[b], t)) { rank = co_rank_in_block(incl, cnt[b], t); return b; }
    }
    return -1;
}

// ---- rotation: na qualifying rows, s of them before the rotation start j0; the m-th (1-based)
// in rotated order (from j0, wrapping) is the co_row_rank-th in row order ----
CASIM_HD int32_t co_row_rank(int32_t m, int32_t na, int32_t s) {
    const int32_t hi_n = na - s;          // qualifying rows >= j0
    return m <= hi_n ? s + m : m - hi_n;
}

// ---- float64 copy counts (every free value and request below 2^53) ----
// floor(free/req) capped at cap with full-rate float64 ops only: below 2^53 the conversions are
// exact, the quotient is within one of the exact floor, and fma(-q, req, free) = free - q*req is an
// integer below 2^53 in magnitude, so it is computed exactly and one step each way makes q exact
// (no 64-bit integer multiply).  rd = (double)req, rcpd = 1/rd.
CASIM_HD int32_t co_dim_copies_f64(int64_t free_, double rd, double rcpd, int32_t cap) {
    const double fd = (double)(free_ < 0 ? 0 : free_);
    const double cp = (double)cap;
    double q = fmin(floor(fd * rcpd), cp);              // NaN (0 * inf) -> cap
    const double t = fma(-q, rd, fd);
    q += ((t >= rd) & (q < cp)) ? 1.0 : 0.0;
    q -= (t < 0.0) ? 1.0 : 0.0;
    return free_ < 0 ? 0 : (int32_t)q;
}
// copies of a resource-only pod that fit a row one after another, capped at cap: min(pods, cap,
// floor(free/req) per requested dimension); a zero request only needs free >= 0.  reqd / rcpd:
// the three requests and their reciprocals in float64; zero: the pod requests nothing.
CASIM_HD int32_t co_copies_f64(int64_t cpu, int64_t mem, int64_t eph, int32_t pods, const double* reqd,
                               const double* rcpd, bool zero, int32_t cap) {
    int32_t c = pods < cap ? pods : cap;
    if (c < 0) c = 0;
    if (!zero) {
        const int32_t cp = c > 1 ? c : 1;
        const int32_t q0 = reqd[0] != 0.0 ? co_dim_copies_f64(cpu, reqd[0], rcpd[0], cp) : (cpu < 0 ? 0 : cp);
        const int32_t q1 = reqd[1] != 0.0 ? co_dim_copies_f64(mem, reqd[1], rcpd[1], cp) : (mem < 0 ? 0 : cp);
        const int32_t q2 = reqd[2] != 0.0 ? co_dim_copies_f64(eph, reqd[2], rcpd[2], cp) : (eph < 0 ? 0 : cp);
        const int32_t q = q0 < q1 ? (q0 < q2 ? q0 : q2) : (q1 < q2 ? q1 : q2);
        c = c < q ? c : q;
    }
    return c;
}
// The run table's constant of a class on a fresh template copy: the copies capped at the group's
// pod count n.  For every 1 <= rem <= n, min(co_fresh_copies(.., n), rem) == co_copies_f64(.., rem):
// the cap only clips a minimum (pods <= 0: both 0).
CASIM_HD int32_t co_fresh_copies(int64_t cpu, int64_t mem, int64_t eph, int32_t pods, const double* reqd,
                                 const double* rcpd, bool zero, int32_t n) {
    return co_copies_f64(cpu, mem, eph, pods, reqd, rcpd, zero, n > 1 ? n : 1);
}

}  // namespace casim
