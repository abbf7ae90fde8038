// Host-only part of the Estimate plan's Go-order sort record (estimate.hip): which settings a
// stored set of Go-order ids was sorted under, whether a run may use them, and how the ids'
// epoch advances.  No HIP: tests/host/sort_reuse_host_check.cpp builds it with the host
// sanitizers and runs it on a CPU.
#pragma once
#include <cstdint>

namespace casim {

// Everything k_class_rank / k_pdq_sort / k_pdq_sort_parts depend on that can differ between two
// runs of one plan.  The plan's lists, templates and the podset's class scores are not here:
// they are written at creation alone (a podset's d_cls_sc only by its upload in mirror.hip, and
// a plan holds its podset const).
struct GoSortKey {
    int32_t fan_parts = 0, fan_min = 0, fan_steps = 0;   // the fan settings the sort was launched with
    int32_t n_sorts = 0;                                 // sort sharing: workgroups of k_pdq_sort
    uint8_t decoupled = 0;                               // the decoupled path ran (ids into d_spod_go)
    uint8_t fold = 0;                                    // class ranks inside the sort kernel (CASIM_NO_RANK_FOLD)
    uint8_t fanned = 0;                                  // k_pdq_sort_parts was launched
    uint8_t go_order = 0;                                // go_sort_order()
};

inline bool go_sort_key_equal(const GoSortKey& a, const GoSortKey& b) {
    return a.fan_parts == b.fan_parts && a.fan_min == b.fan_min && a.fan_steps == b.fan_steps &&
           a.n_sorts == b.n_sorts && a.decoupled == b.decoupled && a.fold == b.fold && a.fanned == b.fanned &&
           a.go_order == b.go_order;
}

// The record of the ids in d_spod_go / d_ids_ready: valid only between a run (or the plan's
// creation) that sorted them and returned CA_OK and the next call that may write those areas.
struct GoSortRecord {
    bool valid = false;
    int32_t epoch = 0;           // the epoch every fan flag of the stored ids holds
    GoSortKey key;
};

// A decoupled run under `want` uses the stored ids instead of sorting.
inline bool go_sort_reusable(const GoSortRecord& r, const GoSortKey& want, bool reuse_on) {
    return reuse_on && r.valid && r.epoch > 0 && want.decoupled && go_sort_key_equal(r.key, want);
}

// The epoch of the next sort.  Epochs are positive; 0 in a fan record means "none".  At
// INT32_MAX the table is cleared first (*wrapped) and the count starts over at 1.
inline int32_t go_sort_next_epoch(int32_t cur, bool* wrapped) {
    *wrapped = cur == INT32_MAX || cur < 0;
    return *wrapped ? 1 : cur + 1;
}

}  // namespace casim
