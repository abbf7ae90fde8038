// scaledown_host.h — the host-only parts of scaledown.hip: the override validation of
// ca_mirror_utilization, the candidates' move lists and the subset selection of
// ca_removal_plan_create_candidates.  No HIP and no mirror types, so a stand-alone program can
// build them with the host sanitizers (tests/host/scaledown_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../include/casim.h"

namespace casim {

// strictly ascending ids in [0, bound)
inline bool ascending_in_range(const int32_t* ids, int32_t n, int64_t bound) {
    for (int32_t k = 0; k < n; k++)
        if (ids[k] < 0 || ids[k] >= bound || (k > 0 && ids[k] <= ids[k - 1])) return false;
    return true;
}

// ca_mirror_util_args against a mirror of n_nodes nodes and n_pods pod ids: CA_OK or CA_EINVAL
inline int check_util_args(const ca_mirror_util_args* a, int64_t n_nodes, int64_t n_pods) {
    if (!a || a->n_node_rows < 0 || a->n_pod_rows < 0) return CA_EINVAL;
    if (a->n_node_rows > 0 && (!a->node_pos || !a->node_rows)) return CA_EINVAL;
    if (a->n_pod_rows > 0 && (!a->pod_ids || !a->pod_rows)) return CA_EINVAL;
    if (!ascending_in_range(a->node_pos, a->n_node_rows, n_nodes)) return CA_EINVAL;
    if (!ascending_in_range(a->pod_ids, a->n_pod_rows, n_pods)) return CA_EINVAL;
    return CA_OK;
}

// CA_UPOD_* of pod `id`'s row: its override's, or the default's from the record's CA_POD_* flags
inline uint32_t util_row_flags(const ca_mirror_util_args* a, int32_t id, uint32_t pod_flags) {
    if (a->n_pod_rows > 0) {
        const int32_t* e = a->pod_ids + a->n_pod_rows;
        const int32_t* p = std::lower_bound(a->pod_ids, e, id);
        if (p != e && *p == id) return a->pod_rows[p - a->pod_ids].flags;
    }
    return (pod_flags & CA_POD_DAEMONSET) ? CA_UPOD_DAEMONSET : CA_UPOD_MOVABLE;
}

// The candidates' pods to move in NodeInfo.Pods order: pods_of(node) is the node's pod ids in
// that order, flags_of(id) the record's CA_POD_* flags.  off gets cand.size() + 1 offsets.
template <class PodsOf, class FlagsOf>
void build_move_lists(const ca_mirror_util_args* a, const std::vector<int32_t>& cand, PodsOf pods_of, FlagsOf flags_of,
                      std::vector<int32_t>& off, std::vector<int32_t>& moves) {
    off.assign(1, 0);
    off.reserve(cand.size() + 1);
    moves.clear();
    for (int32_t nd : cand) {
        for (int32_t id : pods_of(nd))
            if (util_row_flags(a, id, flags_of(id)) & CA_UPOD_MOVABLE) moves.push_back(id);
        off.push_back((int32_t)moves.size());
    }
}

// The lists of the n given candidate positions, in the given order: CA_EINVAL (outputs
// unspecified) unless each is a candidate (cand_of[node] >= 0) and none repeats.
inline int select_candidates(const int32_t* nodes, int32_t n, const std::vector<int32_t>& cand_of,
                             const std::vector<int32_t>& status, const std::vector<int32_t>& move_off,
                             const std::vector<int32_t>& move_pods, std::vector<int32_t>& out_status,
                             std::vector<int32_t>& out_off, std::vector<int32_t>& out_moves) {
    std::vector<uint8_t> seen(cand_of.size(), 0);
    out_status.clear();
    out_off.assign(1, 0);
    out_moves.clear();
    for (int32_t k = 0; k < n; k++) {
        const int32_t nd = nodes[k];
        if (nd < 0 || (size_t)nd >= cand_of.size() || cand_of[nd] < 0 || seen[nd]) return CA_EINVAL;
        seen[nd] = 1;
        const int32_t c = cand_of[nd];
        out_status.push_back(status[c]);
        out_moves.insert(out_moves.end(), move_pods.begin() + move_off[c], move_pods.begin() + move_off[c + 1]);
        out_off.push_back((int32_t)out_moves.size());
    }
    return CA_OK;
}

}  // namespace casim
