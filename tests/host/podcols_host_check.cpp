// Stand-alone check of the resident pod columns' host-only parts
// (autoscaler_amd/csrc/podcols_host.h): the dirty set, the choice between a full upload and a
// staged scatter, the staging builders, the row table and the argument checks, against plain
// restatements on seeded random mutation sequences.  A model device column is kept beside the
// host lists and brought up to date exactly as sync_pod_cols does it (tail ranges, staged
// entries or a full fill); after every sync it has to equal the lists.  Host code only; build
// it with the host sanitizers and run it on a CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/host/podcols_host_check.cpp -o podcols_host_check && ./podcols_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include "../../autoscaler_amd/csrc/podcols_host.h"

using namespace casim;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static void argument_checks() {
    const int32_t ok[3] = {0, 4, 9}, dup[2] = {3, 3}, down[2] = {4, 3}, high[1] = {10}, neg[1] = {-1};
    CHECK(check_pod_row_ids(ok, 3, 10) == CA_OK);
    CHECK(check_pod_row_ids(nullptr, 0, 10) == CA_OK);
    CHECK(check_pod_row_ids(nullptr, 1, 10) == CA_EINVAL);
    CHECK(check_pod_row_ids(ok, -1, 10) == CA_EINVAL);
    CHECK(check_pod_row_ids(dup, 2, 10) == CA_EINVAL);
    CHECK(check_pod_row_ids(down, 2, 10) == CA_EINVAL);
    CHECK(check_pod_row_ids(high, 1, 10) == CA_EINVAL);
    CHECK(check_pod_row_ids(neg, 1, 10) == CA_EINVAL);
    CHECK(check_pod_row_ids(ok, 3, 9) == CA_EINVAL);
    CHECK(check_pod_row_ids(ok, 1, 0) == CA_EINVAL);              // an empty mirror takes no row
    // a slot is written only inside its node's list
    CHECK(podcol_slot_ok(0, 1) && podcol_slot_ok(256, 257));
    CHECK(!podcol_slot_ok(-1, 5) && !podcol_slot_ok(5, 5) && !podcol_slot_ok(0, 0) && !podcol_slot_ok(INT32_MAX, 7));
}

static void full_or_staged() {
    CHECK(podcol_full_limit(0) == 1024 && podcol_full_limit(4096) == 1024 && podcol_full_limit(4100) == 1025);
    CHECK(podcol_full_limit(317177) == 79294);
    for (size_t P : {(size_t)100, (size_t)5000, (size_t)40000}) {
        PodColDirty d;
        CHECK(d.plan(P) == PodColDirty::SYNC_FULL);              // born all-dirty
        d.mark(3);                                                // (nothing to remember while full)
        CHECK(d.ids.empty());
        d.done(P);
        CHECK(d.plan(P) == PodColDirty::SYNC_NONE && d.synced == P);
        const size_t lim = podcol_full_limit(P), n = std::min(P, lim + 1);
        for (size_t i = 0; i < n; i++) {
            d.mark((int32_t)i);
            d.mark((int32_t)i);                                   // no id twice
            CHECK(d.ids.size() == i + 1);
            CHECK(d.plan(P) == (i + 1 > lim ? PodColDirty::SYNC_FULL : PodColDirty::SYNC_STAGED));
        }
        d.mark((int32_t)P);                                       // the tail is never marked
        d.mark((int32_t)P + 5);
        d.mark(-1);
        CHECK(d.ids.size() == n);
        d.done(P + 7);
        CHECK(d.ids.empty() && d.synced == P + 7 && d.plan(P + 7) == PodColDirty::SYNC_NONE);
        for (uint8_t f : d.flag) CHECK(f == 0);
        d.mark((int32_t)P + 6);                                   // below the new synced count
        CHECK(d.ids.size() == 1);
        d.mark_full();
        CHECK(d.ids.empty() && d.plan(P + 7) == PodColDirty::SYNC_FULL);
        for (uint8_t f : d.flag) CHECK(f == 0);
    }
}

// the lists, as the mirror keeps them
struct Model {
    std::vector<std::vector<int32_t>> node_pods;
    std::vector<int32_t> pod_node;
    PodColDirty dirty;
    std::vector<int32_t> d_node, d_slot;          // the "device" columns
    int64_t full = 0, staged = 0, tail = 0;

    void add(int32_t x) {
        const int32_t id = (int32_t)pod_node.size();
        pod_node.push_back(x);
        node_pods[x].push_back(id);
        dirty.mark(id);                           // ignored: a new id is the tail
    }
    void remove(int32_t id) {
        auto& l = node_pods[pod_node[id]];
        const int32_t s = podcol_slot_of(l, id);
        CHECK(s >= 0);
        l[s] = l.back();
        l.pop_back();
        pod_node[id] = -1;
        dirty.mark(id);
        if ((size_t)s < l.size()) dirty.mark(l[s]);
    }
    void reattach(int32_t id, int32_t x, int32_t slot) {   // a reverted RemovePod
        auto& l = node_pods[x];
        if ((size_t)slot == l.size()) {
            l.push_back(id);
        } else {
            l.push_back(l[slot]);
            l[slot] = id;
            dirty.mark(l.back());
        }
        pod_node[id] = x;
        dirty.mark(id);
    }
    void remove_node(int32_t x) {
        for (int32_t id : node_pods[x]) pod_node[id] = -1;
        node_pods.erase(node_pods.begin() + x);
        for (auto& v : pod_node) if (v > x) v--;
        dirty.mark_full();
    }
    void reorder(const std::vector<int32_t>& order) {
        std::vector<int32_t> inv(order.size());
        std::vector<std::vector<int32_t>> moved;
        for (size_t k = 0; k < order.size(); k++) { inv[order[k]] = (int32_t)k; moved.push_back(node_pods[order[k]]); }
        node_pods.swap(moved);
        for (auto& v : pod_node) if (v >= 0) v = inv[v];
        if (!dirty.full)                                          // the device permutes what it holds
            for (size_t i = 0; i < dirty.synced; i++) if (d_node[i] >= 0 && (size_t)d_node[i] < inv.size()) d_node[i] = inv[d_node[i]];
    }
    void sync() {
        const size_t P = pod_node.size();
        auto node_of = [&](int32_t id) { return pod_node[id]; };
        auto pods_of = [&](int32_t x) -> const std::vector<int32_t>& { return node_pods[x]; };
        const int plan = dirty.plan(P);
        d_node.resize(P, -7);
        d_slot.resize(P, -7);
        if (plan == PodColDirty::SYNC_FULL) {
            std::vector<int32_t> n(P), s(P);
            podcol_fill_full(P, node_pods.size(), pods_of, n.data(), s.data());
            d_node = n;
            d_slot = s;
            full++;
        } else {
            const size_t lo = dirty.synced;
            std::vector<int32_t> n(P - lo), s(P - lo);
            podcol_fill_range(lo, P, node_of, pods_of, n.data(), s.data());
            std::copy(n.begin(), n.end(), d_node.begin() + lo);
            std::copy(s.begin(), s.end(), d_slot.begin() + lo);
            tail += (int64_t)(P - lo);
            if (plan == PodColDirty::SYNC_STAGED) {
                std::vector<PodColEntry> e(dirty.ids.size());
                podcol_build_stage(dirty.ids, node_of, pods_of, e.data());
                std::set<int32_t> once;
                for (const PodColEntry& v : e) {
                    CHECK(once.insert(v.id).second && (size_t)v.id < lo);
                    d_node[v.id] = v.node;
                    d_slot[v.id] = v.slot;
                }
                staged++;
            }
        }
        dirty.done(P);
        // the columns are the lists
        std::vector<int32_t> wn(P, -1), ws(P, -1);
        for (size_t x = 0; x < node_pods.size(); x++)
            for (size_t s = 0; s < node_pods[x].size(); s++) { wn[node_pods[x][s]] = (int32_t)x; ws[node_pods[x][s]] = (int32_t)s; }
        for (size_t i = 0; i < P; i++) {
            CHECK(d_node[i] == wn[i] && wn[i] == pod_node[i]);
            if (wn[i] >= 0) CHECK(d_slot[i] == ws[i] && podcol_slot_ok(d_slot[i], (int32_t)node_pods[wn[i]].size()));
        }
    }
};

static void sequences(unsigned seed) {
    std::mt19937 rng(seed);
    Model m;
    m.node_pods.resize(4 + rng() % 12);
    struct Removed { int32_t id, node, slot; };
    std::vector<Removed> undo;                    // removals a "revert" puts back, newest first
    const int steps = 150 + (int)(rng() % 150);
    for (int t = 0; t < steps; t++) {
        const unsigned op = rng() % 100;
        std::vector<int32_t> placed;
        for (size_t i = 0; i < m.pod_node.size(); i++) if (m.pod_node[i] >= 0) placed.push_back((int32_t)i);
        if (op < 45 || placed.empty()) {
            const int k = 1 + (int)(rng() % (seed % 3 == 0 ? 300 : 6));   // (some seeds cross the 1024 limit)
            for (int j = 0; j < k; j++) m.add((int32_t)(rng() % m.node_pods.size()));
            undo.clear();
        } else if (op < 70) {
            const int32_t id = placed[rng() % placed.size()], x = m.pod_node[id];
            undo.push_back({id, x, podcol_slot_of(m.node_pods[x], id)});
            m.remove(id);
        } else if (op < 80 && !undo.empty()) {
            while (!undo.empty()) {               // in reverse, as the journal does
                m.reattach(undo.back().id, undo.back().node, undo.back().slot);
                undo.pop_back();
            }
        } else if (op < 84 && m.node_pods.size() > 3) {
            m.remove_node((int32_t)(rng() % m.node_pods.size()));
            undo.clear();
        } else if (op < 90) {
            std::vector<int32_t> order(m.node_pods.size());
            for (size_t k = 0; k < order.size(); k++) order[k] = (int32_t)k;
            std::shuffle(order.begin(), order.end(), rng);
            m.reorder(order);
            undo.clear();                         // (positions in it are the old order's)
        } else if (seed % 3 == 0 && op < 93 && placed.size() > 1100) {
            for (size_t j = 0; j < placed.size(); j += 2) m.remove(placed[j]);   // past max(1024, P/4): a full upload
            undo.clear();
        }
        if (rng() % 4 == 0) m.sync();
    }
    m.sync();
    CHECK(m.full >= 1);
    if (seed % 3 != 0) CHECK(m.staged > 0 && m.tail > 0);
}

static void row_table() {
    PodRowTable t;
    ca_util_pod r{};
    r.req_milli[0] = 5;
    r.flags = CA_UPOD_BLOCKING;
    CHECK(!t.has_row(0) && !t.has_row(1000) && t.entry(7).has == 0 && t.entry(7).id == 7);
    CHECK(!t.set(3, nullptr));                    // clearing what has no row changes nothing
    CHECK(t.set(3, &r) && t.has_row(3) && t.has.size() == 4 && t.entry(3).row.flags == CA_UPOD_BLOCKING);
    CHECK(!t.set(3, &r));                         // the same row again changes nothing
    r.grace_s = 30;
    CHECK(t.set(3, &r) && t.entry(3).row.grace_s == 30);
    r.grace_s = 0;
    CHECK(t.set(3, &r));
    t.inherit(9, 3);                              // the planner's copy takes its source's row
    CHECK(t.has_row(9) && t.entry(9).row.req_milli[0] == 5 && t.has.size() == 10);
    t.inherit(11, 4);                             // ... and nothing from a source without one
    CHECK(!t.has_row(11) && t.has.size() == 10);
    CHECK(t.set(3, nullptr) && !t.has_row(3) && t.entry(3).has == 0 && t.entry(3).row.flags == 0);
    CHECK(t.has_row(9));
    t.grow(50);
    CHECK(t.has.size() == 50 && t.rows.size() == 50 && t.has_row(9) && !t.has_row(49));
}

int main() {
    argument_checks();
    full_or_staged();
    row_table();
    for (unsigned seed = 0; seed < 30; seed++) sequences(seed);
    std::puts("podcols host checks ok");
    return 0;
}
