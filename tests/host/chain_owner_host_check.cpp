// Stand-alone check of the lean Estimate chain's index arithmetic and fresh-copy constant
// (autoscaler_amd/csrc/chain_owner_host.h, the functions the kernel itself calls).  Host code
// only; build it with the host sanitizers and run it on a CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/host/chain_owner_host_check.cpp -o chain_owner_host_check && ./chain_owner_host_check
// The copy-count arithmetic lives in the header (the kernel's dim_copies_f64 and k_run_table call
// it), so it is checked here against exact integer arithmetic rather than restated.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>
#include "../../autoscaler_amd/csrc/chain_owner_host.h"

using namespace casim;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

constexpr int CW = 4;
constexpr int KMAX = 4160;

// the owned blocks partition the rows
static void partition() {
    for (int k = 0; k <= KMAX; k++) {
        std::vector<int> seen(k, 0);
        int blocks = 0;
        for (int wv = 0; wv < CW; wv++) {
            const int nbw = co_wave_blocks(k, wv, CW);
            blocks += nbw;
            for (int i = 0; i < nbw; i++) {
                const int b = co_wave_block(wv, i, CW);
                CHECK(b < co_blocks(k) && co_owner(b, CW) == wv);
                for (int j = b * 64; j < b * 64 + 64 && j < k; j++) seen[j]++;
            }
            // one past the wave's last block lies beyond the rows
            CHECK(co_wave_block(wv, nbw, CW) >= co_blocks(k));
        }
        CHECK(blocks == co_blocks(k));
        for (int j = 0; j < k; j++) CHECK(seen[j] == 1);
    }
    for (int bmin = 0; bmin < 80; bmin++)
        for (int wv = 0; wv < CW; wv++) {
            const int b = co_first_block(bmin, wv, CW);
            CHECK(b >= bmin && b < bmin + CW && co_owner(b, CW) == wv);
        }
}

// the opening [k0, k0 + n) is written exactly once, each row by the owner of its block
static void opening() {
    const int ns[] = {1, 2, 3, 9, 10, 16, 62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 321, 700};
    std::vector<int> seen;
    for (int k0 = 0; k0 <= KMAX; k0++) {
        for (int n : ns) {
            if (k0 + n > KMAX + 64) continue;
            seen.assign(n, 0);
            for (int wv = 0; wv < CW; wv++) {
                for (int b = co_first_block(k0 >> 6, wv, CW); b * 64 < k0 + n; b += CW) {
                    CHECK(co_owner(b, CW) == wv);
                    int32_t lo, hi;
                    co_open_rows(k0, n, b, lo, hi);
                    CHECK(lo < hi);                       // every block visited holds opened rows
                    for (int j = lo; j < hi; j++) {
                        CHECK(j >= k0 && j < k0 + n && (j >> 6) == b);
                        seen[j - k0]++;
                    }
                }
            }
            for (int i = 0; i < n; i++) CHECK(seen[i] == 1);
        }
    }
    // a block outside the opening gets an empty range
    int32_t lo, hi;
    co_open_rows(60, 10, 2, lo, hi);
    CHECK(hi <= lo);
    co_open_rows(130, 10, 1, lo, hi);
    CHECK(hi <= lo);
}

// the t-th qualifying row from per-block counts against a walk over the rows
static void check_pick(const std::vector<char>& q, int k) {
    const int nb = co_blocks(k);
    std::vector<int32_t> cnt(nb, 0), rows;
    for (int j = 0; j < k; j++)
        if (q[j]) { cnt[j >> 6]++; rows.push_back(j); }
    const int na = (int)rows.size();
    int32_t rank = -7;
    CHECK(co_find_block(cnt.data(), nb, na + 1, rank) == -1);
    if (na == 0) return;
    const int ts[] = {1, 2, na / 2, na - 1, na};
    for (int t : ts) {
        if (t < 1 || t > na) continue;
        const int b = co_find_block(cnt.data(), nb, t, rank);
        CHECK(b >= 0 && b < nb && cnt[b] > 0 && rank >= 1 && rank <= cnt[b]);
        // the rank-th qualifying row of block b (the kernel: one ballot over the block's counts)
        int found = -1, seen = 0;
        for (int j = b * 64; j < b * 64 + 64 && j < k; j++)
            if (q[j] && ++seen == rank) { found = j; break; }
        CHECK(found == rows[t - 1]);
    }
}
static void pick() {
    std::mt19937 rng(12345);
    for (int k = 0; k <= KMAX; k++) {
        const int nb = co_blocks(k);
        std::vector<char> q(k, 0);
        check_pick(q, k);                                             // nothing qualifies
        for (int j = 0; j < k; j++) q[j] = 1;
        check_pick(q, k);                                             // every row
        for (int j = 0; j < k; j++) q[j] = (rng() & 7) == 0;
        check_pick(q, k);                                             // random, sparse
        for (int j = 0; j < k; j++) q[j] = (rng() & 3) != 0;
        check_pick(q, k);                                             // random, dense
        if (nb == 0) continue;
        const int bs[] = {0, nb / 2, nb - 1};
        for (int b1 : bs) {                                           // all in one block
            for (int j = 0; j < k; j++) q[j] = (j >> 6) == b1;
            check_pick(q, k);
        }
        for (int j = 0; j < k; j++) q[j] = (j & 63) == ((j >> 6) * 7 & 63) || j == k - 1;
        check_pick(q, k);                                             // one per block
        for (int j = 0; j < k; j++) q[j] = ((j >> 6) & 1) == 0 && (j & 5) == 0;
        check_pick(q, k);                                             // empty blocks between
        for (int j = 0; j < k; j++) q[j] = ((j >> 6) % 3) == 2 || j == 0;
        check_pick(q, k);                                             // two empty blocks between, row 0
        for (int j = 0; j < k; j++) q[j] = j == 0 || j == k - 1;
        check_pick(q, k);                                             // each end only
    }
}

// rotated-order rank -> row-order rank for every rotation start, against a walk from j0
static void rotation() {
    std::mt19937 rng(777);
    for (int k = 1; k <= KMAX; k++) {
        // every rotation start of every k against the list of qualifying rows read from its s-th
        // entry on, wrapping; and against a row-by-row walk from j0 for every start up to 330 rows
        // (the block and ownership edges the GPU tests plant) and a stride of starts at the block
        // edges beyond
        const bool every_j0 = k <= 330;
        const bool edge = (k & 63) <= 1 || (k & 63) == 63;
        std::vector<char> q(k);
        std::vector<int32_t> rows;
        for (int j = 0; j < k; j++) {
            q[j] = (rng() % 5) == 0 || j == (k * 3) / 4;
            if (q[j]) rows.push_back(j);
        }
        const int na = (int)rows.size();
        int s = 0;                                                   // qualifying rows before j0
        const int wstep = 1 + (int)(rng() % 97);
        for (int j0 = 0; j0 <= k; j0++) {
            if (j0 > 0 && q[j0 - 1]) s++;
            if (j0 == k) continue;
            const bool walk_all = every_j0 || (edge && (j0 % wstep == 0 || j0 == k - 1));
            const int ms[] = {1, na - s, na - s + 1, na, 1 + (int)(rng() % na)};
            for (int m : ms) {
                if (m < 1 || m > na) continue;
                const int t = co_row_rank(m, na, s);
                CHECK(t >= 1 && t <= na);
                if (walk_all) {
                    int j = j0, seen = 0;
                    for (;;) {                                        // the m-th qualifying row from j0, wrapping
                        if (q[j] && ++seen == m) break;
                        j = j + 1 == k ? 0 : j + 1;
                    }
                    CHECK(rows[t - 1] == j);
                } else {
                    CHECK(rows[t - 1] == rows[(s + m - 1) % na]);
                }
            }
        }
    }
}

// exact min(pods, cap, floor(free / req) per requested dimension)
static int64_t exact_copies(const int64_t fr[3], int32_t pods, const int64_t req[3], bool zero, int64_t cap) {
    int64_t c = pods < cap ? pods : cap;
    if (c <= 0) return 0;
    if (!zero)
        for (int i = 0; i < 3; i++) {
            const int64_t q = fr[i] < 0 ? 0 : req[i] == 0 ? c : fr[i] / req[i];
            c = q < c ? q : c;
        }
    return c;
}
static void fresh_copies() {
    const int64_t GI = 1ll << 30, E53 = 1ll << 53;
    const int64_t frees[][3] = {
        {4000, 8 * GI, 0}, {91200, 729 * GI, 100 * GI}, {0, 0, 0}, {1, 1, 1}, {E53 - 1, E53 - 1, E53 - 1},
        {-5, 8 * GI, 0}, {4000, -1, 0}, {999, 8 * GI, 7}, {1000, 3 * GI - 1, 0}, {E53 - 1, 3, 0}, {64000, 7, E53 - 2},
    };
    const int64_t reqs[][3] = {
        {1000, 2 * GI, 0}, {1, 1, 0}, {0, 0, 0}, {150, 0, 0}, {0, GI, 0}, {0, 0, 1}, {3, 7, 11}, {4001, 1, 0},
        {E53 - 1, 0, 0}, {1, E53 - 1, 1}, {1000, 3 * GI, 0}, {333, 1 + GI / 3, 5},
    };
    const int32_t podss[] = {110, 1, 0, -3, 10, 1 << 20, std::numeric_limits<int32_t>::max()};
    const int32_t counts[] = {1, 2, 3, 7, 64, 300, 1 << 20};
    std::mt19937 rng(99);
    for (const auto& fr : frees)
        for (const auto& rq : reqs)
            for (int32_t pods : podss)
                for (int zf = 0; zf < 2; zf++) {
                    const bool all0 = rq[0] == 0 && rq[1] == 0 && rq[2] == 0;
                    if (zf && !all0) continue;             // SF_ZERO is only set for a pod with no request
                    const bool zero = zf != 0;
                    double rd[3], rc[3];
                    for (int i = 0; i < 3; i++) {
                        rd[i] = (double)rq[i];
                        rc[i] = rq[i] > 0 ? 1.0 / (double)rq[i] : std::numeric_limits<double>::infinity();
                    }
                    for (int32_t n : counts) {
                        const int32_t rct = co_fresh_copies(fr[0], fr[1], fr[2], pods, rd, rc, zero, n);
                        CHECK(rct == exact_copies(fr, pods, rq, zero, n));
                        CHECK(rct >= 0 && rct <= n);
                        for (int32_t i = 0; i < 400; i++) {
                            // every rem2 of a small group; both ends, rct's neighbourhood and a sample of a large one
                            int32_t rem2;
                            if (n <= 300) { rem2 = i + 1; if (rem2 > n) break; }
                            else if (i < 100) rem2 = i + 1;
                            else if (i < 200) rem2 = n - (i - 100);
                            else if (i < 210) rem2 = rct - 5 + (i - 200);
                            else rem2 = 1 + (int32_t)(rng() % (uint32_t)n);
                            if (rem2 < 1 || rem2 > n) continue;
                            const int32_t capped = co_copies_f64(fr[0], fr[1], fr[2], pods, rd, rc, zero, rem2);
                            CHECK((rct < rem2 ? rct : rem2) == capped);
                            CHECK(capped == exact_copies(fr, pods, rq, zero, rem2));
                        }
                    }
                }
}

int main() {
    partition();
    opening();
    pick();
    rotation();
    fresh_copies();
    std::printf("chain owner host checks ok\n");
    return 0;
}
