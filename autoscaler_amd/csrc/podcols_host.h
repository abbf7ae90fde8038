// podcols_host.h — the host-only parts of the resident per-pod columns (podcols.hip): the dirty
// set, the choice between a full upload and a staged scatter, the staging builders and the
// argument check of the row calls.  No HIP and no mirror types, so a stand-alone program can
// build them with the host sanitizers (tests/host/podcols_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>
#include "scaledown_host.h"

namespace casim {

// One staged column entry: pod id, its node and its slot in the node's NodeInfo.Pods list.
struct PodColEntry {
    int32_t id, node, slot;
};

// One staged util row: the row, its pod id and the has-row flag it sets (0 clears the row).
struct PodRowEntry {
    ca_util_pod row;
    int32_t id, has;
};
static_assert(sizeof(PodRowEntry) == 56, "PodRowEntry is 56 B");

// More dirty ids than this make a full upload (the rows' max(64, n/4) rule for pods; a design
// choice, not a measurement).
inline size_t podcol_full_limit(size_t n_pods) { return std::max<size_t>(1024, n_pods / 4); }

// Ids whose device entry is stale.  Ids at or above `synced` are the tail: the next sync
// uploads them from the host state as it is then, so they are never marked.  No id is held
// twice (the scatter has no order).
struct PodColDirty {
    size_t synced = 0;            // ids below have a device entry
    bool full = true;             // the next sync uploads every entry
    std::vector<int32_t> ids;
    std::vector<uint8_t> flag;    // [synced]: id is in ids

    void mark(int32_t id) {
        if (full || id < 0 || (size_t)id >= synced) return;
        if (flag.size() < synced) flag.resize(synced, 0);
        if (flag[(size_t)id]) return;
        flag[(size_t)id] = 1;
        ids.push_back(id);
    }
    void mark_full() {
        full = true;
        drop();
    }
    enum { SYNC_NONE = 0, SYNC_STAGED, SYNC_FULL };
    // what the next sync of n_pods ids does for the entries below the tail
    int plan(size_t n_pods) const {
        if (full || ids.size() > podcol_full_limit(n_pods)) return SYNC_FULL;
        return ids.empty() ? SYNC_NONE : SYNC_STAGED;
    }
    // the sync of n_pods ids is queued: nothing is stale
    void done(size_t n_pods) {
        drop();
        synced = n_pods;
        full = false;
    }

  private:
    void drop() {
        for (int32_t id : ids) flag[(size_t)id] = 0;
        ids.clear();
    }
};

// slot of `id` in a node's pod list, -1 when it is not there (searched from the back: pods
// that changed slot are mostly the newest)
template <class Pods> int32_t podcol_slot_of(const Pods& pods, int32_t id) {
    for (size_t i = pods.size(); i-- > 0;)
        if (pods[i] == id) return (int32_t)i;
    return -1;
}

// (node, slot) of ids [lo, hi) into node[0 .. hi - lo) / slot[...]: node_of(id) is PodRow.node,
// pods_of(node) the node's ids in NodeInfo.Pods order.  A pod on no node gets (-1, -1).
template <class NodeOf, class PodsOf>
void podcol_fill_range(size_t lo, size_t hi, NodeOf node_of, PodsOf pods_of, int32_t* node, int32_t* slot) {
    for (size_t id = lo; id < hi; id++) {
        const int32_t x = node_of((int32_t)id);
        node[id - lo] = x;
        slot[id - lo] = x < 0 ? -1 : podcol_slot_of(pods_of(x), (int32_t)id);
    }
}

// Every id's (node, slot) by one walk over the nodes' lists (no search per pod).
template <class PodsOf>
void podcol_fill_full(size_t n_pods, size_t n_nodes, PodsOf pods_of, int32_t* node, int32_t* slot) {
    std::fill(node, node + n_pods, -1);
    std::fill(slot, slot + n_pods, -1);
    for (size_t x = 0; x < n_nodes; x++) {
        const auto& pods = pods_of((int32_t)x);
        for (size_t i = 0; i < pods.size(); i++) {
            const int32_t id = pods[i];
            if (id < 0 || (size_t)id >= n_pods) continue;
            node[id] = (int32_t)x;
            slot[id] = (int32_t)i;
        }
    }
}

// The dirty ids' entries for the scatter, in the order they were marked.
template <class NodeOf, class PodsOf>
void podcol_build_stage(const std::vector<int32_t>& ids, NodeOf node_of, PodsOf pods_of, PodColEntry* out) {
    for (size_t k = 0; k < ids.size(); k++) {
        const int32_t x = node_of(ids[k]);
        out[k] = PodColEntry{ids[k], x, x < 0 ? -1 : podcol_slot_of(pods_of(x), ids[k])};
    }
}

// ca_mirror_set_pod_util_rows / ca_mirror_get_pod_util_rows: CA_OK or CA_EINVAL
inline int check_pod_row_ids(const int32_t* pod_ids, int32_t n, int64_t n_pods) {
    if (n < 0 || (n > 0 && !pod_ids)) return CA_EINVAL;
    return ascending_in_range(pod_ids, n, n_pods) ? CA_OK : CA_EINVAL;
}

// The host copy of the util rows, by pod id; ids past the end have no row.
struct PodRowTable {
    std::vector<ca_util_pod> rows;
    std::vector<uint8_t> has;
    void grow(size_t n_pods) {
        if (has.size() < n_pods) {
            has.resize(n_pods, 0);
            rows.resize(n_pods, ca_util_pod{});
        }
    }
    bool has_row(int32_t id) const { return (size_t)id < has.size() && has[(size_t)id]; }
    // rows == NULL clears; returns whether anything changed (a row equal to the stored one, byte
    // for byte, changes nothing: it is not sent again)
    bool set(int32_t id, const ca_util_pod* row) {
        if (!row) {
            if (!has_row(id)) return false;
            has[(size_t)id] = 0;
            rows[(size_t)id] = ca_util_pod{};
            return true;
        }
        if (has_row(id) && std::memcmp(&rows[(size_t)id], row, sizeof *row) == 0) return false;
        grow((size_t)id + 1);
        has[(size_t)id] = 1;
        rows[(size_t)id] = *row;
        return true;
    }
    // the copy the planner commits is the same pod object: it takes its source's row and flag
    void inherit(int32_t id, int32_t src) {
        if (has_row(src)) {
            const ca_util_pod r = rows[(size_t)src];
            set(id, &r);
        }
    }
    PodRowEntry entry(int32_t id) const {
        PodRowEntry e;
        e.row = has_row(id) ? rows[(size_t)id] : ca_util_pod{};
        e.id = id;
        e.has = has_row(id) ? 1 : 0;
        return e;
    }
};

// A slot is written only inside its node's list: [0, count).
inline bool podcol_slot_ok(int32_t slot, int32_t count) { return slot >= 0 && slot < count; }

}  // namespace casim
