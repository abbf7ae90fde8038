// Stand-alone check of scaledown.hip's host-only parts (autoscaler_amd/csrc/scaledown_host.h):
// the override validation, the move-list builder and the candidate subset selection, against
// plain restatements on seeded random inputs and the argument edges.  Host code only; build it
// with the host sanitizers and run it on a CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/host/scaledown_host_check.cpp -o scaledown_host_check && ./scaledown_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include "../../autoscaler_amd/csrc/scaledown_host.h"

using namespace casim;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static ca_mirror_util_args args_of(const std::vector<int32_t>& npos, const std::vector<ca_util_node>& nrows,
                                   const std::vector<int32_t>& pids, const std::vector<ca_util_pod>& prows) {
    ca_mirror_util_args a{};
    a.node_pos = npos.data(); a.node_rows = nrows.data(); a.n_node_rows = (int32_t)npos.size();
    a.pod_ids = pids.data(); a.pod_rows = prows.data(); a.n_pod_rows = (int32_t)pids.size();
    return a;
}

static void validation() {
    const std::vector<ca_util_node> nr(4);
    const std::vector<ca_util_pod> pr(4);
    auto st = [&](std::vector<int32_t> np, std::vector<int32_t> pp, int64_t nn, int64_t npods) {
        const std::vector<ca_util_node> n2(np.size());
        const std::vector<ca_util_pod> p2(pp.size());
        ca_mirror_util_args a = args_of(np, n2, pp, p2);
        return check_util_args(&a, nn, npods);
    };
    CHECK(st({}, {}, 0, 0) == CA_OK);
    CHECK(st({0, 9}, {0, 99}, 10, 100) == CA_OK);
    CHECK(st({0, 10}, {}, 10, 100) == CA_EINVAL);            // out of range
    CHECK(st({-1}, {}, 10, 100) == CA_EINVAL);
    CHECK(st({}, {5, 100}, 10, 100) == CA_EINVAL);
    CHECK(st({}, {5, 5}, 10, 100) == CA_EINVAL);             // duplicate
    CHECK(st({}, {6, 5}, 10, 100) == CA_EINVAL);             // unsorted
    CHECK(st({3, 2}, {}, 10, 100) == CA_EINVAL);
    CHECK(st({0}, {}, 0, 0) == CA_EINVAL);                   // an empty mirror takes no override
    CHECK(check_util_args(nullptr, 1, 1) == CA_EINVAL);
    ca_mirror_util_args a{};
    a.n_pod_rows = 2;                                        // a count without rows
    CHECK(check_util_args(&a, 1, 5) == CA_EINVAL);
    const int32_t ids[2] = {1, 2};
    a.pod_ids = ids;
    CHECK(check_util_args(&a, 1, 5) == CA_EINVAL);
    a.pod_rows = pr.data();
    CHECK(check_util_args(&a, 1, 5) == CA_OK);
    a.n_node_rows = -1;
    CHECK(check_util_args(&a, 1, 5) == CA_EINVAL);
}

static void lists(unsigned seed) {
    std::mt19937 rng(seed);
    const int32_t n_nodes = 1 + (int32_t)(rng() % 40), n_pods = (int32_t)(rng() % 400);
    std::vector<std::vector<int32_t>> pods_of((size_t)n_nodes);
    std::vector<uint32_t> pflags((size_t)n_pods);
    for (int32_t i = 0; i < n_pods; i++) {
        pflags[i] = (rng() % 5 == 0) ? CA_POD_DAEMONSET : 0;
        if (rng() % 7) pods_of[rng() % n_nodes].push_back(i);                // (some ids are on no node)
    }
    for (auto& l : pods_of) std::shuffle(l.begin(), l.end(), rng);           // NodeInfo.Pods order is not id order
    std::vector<int32_t> pids;
    std::vector<ca_util_pod> prows;
    for (int32_t i = 0; i < n_pods; i++)
        if (rng() % 4 == 0) {
            ca_util_pod r{};
            const uint32_t kinds[4] = {CA_UPOD_MOVABLE, CA_UPOD_BLOCKING, CA_UPOD_MIRROR, CA_UPOD_MOVABLE | CA_UPOD_DELETED};
            r.flags = kinds[rng() % 4];
            pids.push_back(i);
            prows.push_back(r);
        }
    const std::vector<int32_t> npos;
    const std::vector<ca_util_node> nrows;
    const ca_mirror_util_args a = args_of(npos, nrows, pids, prows);
    CHECK(check_util_args(&a, n_nodes, n_pods) == CA_OK);
    std::vector<int32_t> cand, cand_of((size_t)n_nodes, -1);
    for (int32_t x = 0; x < n_nodes; x++)
        if (rng() % 2) { cand_of[x] = (int32_t)cand.size(); cand.push_back(x); }
    std::vector<int32_t> off, moves;
    build_move_lists(
        &a, cand, [&](int32_t nd) -> const std::vector<int32_t>& { return pods_of[nd]; },
        [&](int32_t id) { return pflags[id]; }, off, moves);
    CHECK(off.size() == cand.size() + 1 && off[0] == 0 && off.back() == (int32_t)moves.size());
    for (size_t c = 0; c < cand.size(); c++) {                               // the rule, restated
        std::vector<int32_t> want;
        for (int32_t id : pods_of[cand[c]]) {
            uint32_t f = (pflags[id] & CA_POD_DAEMONSET) ? CA_UPOD_DAEMONSET : CA_UPOD_MOVABLE;
            for (size_t k = 0; k < pids.size(); k++)
                if (pids[k] == id) f = prows[k].flags;
            if (f & CA_UPOD_MOVABLE) want.push_back(id);
        }
        CHECK(std::vector<int32_t>(moves.begin() + off[c], moves.begin() + off[c + 1]) == want);
    }
    // the subset selection: a shuffled subset, then every refusal
    std::vector<int32_t> status(cand.size());
    for (auto& s : status) s = (rng() % 3 == 0) ? CA_UNREMOVABLE_BLOCKED_BY_POD : 0;
    std::vector<int32_t> sel = cand;
    std::shuffle(sel.begin(), sel.end(), rng);
    sel.resize(sel.size() / 2);
    std::vector<int32_t> s2, o2, m2;
    CHECK(select_candidates(sel.data(), (int32_t)sel.size(), cand_of, status, off, moves, s2, o2, m2) == CA_OK);
    CHECK(s2.size() == sel.size() && o2.size() == sel.size() + 1);
    for (size_t k = 0; k < sel.size(); k++) {
        const int32_t c = cand_of[sel[k]];
        CHECK(s2[k] == status[c] && o2[k + 1] - o2[k] == off[c + 1] - off[c]);
        CHECK(std::equal(m2.begin() + o2[k], m2.begin() + o2[k + 1], moves.begin() + off[c]));
    }
    CHECK(select_candidates(nullptr, 0, cand_of, status, off, moves, s2, o2, m2) == CA_OK && o2.size() == 1);
    for (int32_t bad : {-1, n_nodes, n_nodes + 7}) {
        CHECK(select_candidates(&bad, 1, cand_of, status, off, moves, s2, o2, m2) == CA_EINVAL);
    }
    for (int32_t x = 0; x < n_nodes; x++)
        if (cand_of[x] < 0) CHECK(select_candidates(&x, 1, cand_of, status, off, moves, s2, o2, m2) == CA_EINVAL);
    if (!cand.empty()) {
        const int32_t twice[2] = {cand[0], cand[0]};
        CHECK(select_candidates(twice, 2, cand_of, status, off, moves, s2, o2, m2) == CA_EINVAL);
    }
}

int main() {
    validation();
    for (unsigned seed = 0; seed < 200; seed++) lists(seed);
    std::puts("scaledown host checks ok");
    return 0;
}
