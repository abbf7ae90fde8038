// util_core.h — utilization.Calculate's arithmetic (CA/simulator/utilization/info.go:48-127),
// shared by the table form (utilization.hip) and the mirror form (scaledown.hip): one pod's
// share of its node's sums, the per-node atomic accumulator, and the node's Info row.
#pragma once
#include "casim_internal.h"

namespace casim {

// per-node sums that pods add into with atomics (k_added_sums, k_mirror_pod_sums); the node
// kernel that consumes a row clears it
struct UtilSum {
    unsigned long long req[3], dsm[3];       // int64 sums (two's complement adds)
    int32_t drain, pad;
    int64_t pad2;
};
static_assert(sizeof(UtilSum) == 64, "UtilSum");

constexpr int64_t kNsPerS = 1000000000LL;
constexpr int64_t kLongTerminatingExtraNs = 30 * kNsPerS;   // drain.go:34 PodLongTerminatingExtraThreshold

// calculateUtilizationOfResource's final ratio (info.go:126): float64 / float64 of the
// MilliValue difference, one correctly rounded IEEE division (built -ffp-contract=off).
__device__ inline double util_ratio(int64_t pods, int64_t alloc, int64_t dsm) {
    return (double)pods / (double)(alloc - dsm);
}

// one pod's share of its node's sums (info.go:100-124)
__device__ inline void pod_share(const ca_util_pod& p, int32_t skip_ds, int32_t skip_mirror, int64_t now_ns,
                                 int64_t (&req)[3], int64_t (&dsm)[3], int& drain) {
    drain |= (int)(p.flags & (CA_UPOD_MOVABLE | CA_UPOD_BLOCKING));
    const bool factored = (skip_ds && (p.flags & CA_UPOD_DAEMONSET)) || (skip_mirror && (p.flags & CA_UPOD_MIRROR));
    // drain.IsPodLongTerminating (utils/drain/drain.go:294-306): deleted, and deletion +
    // grace + 30 s strictly before now
    const bool long_term = !factored && (p.flags & CA_UPOD_DELETED) &&
                           p.deletion_ns + p.grace_s * kNsPerS + kLongTerminatingExtraNs < now_ns;
    for (int r = 0; r < 3; r++) {
        if (factored) dsm[r] += p.req_milli[r];
        else if (!long_term) req[r] += p.req_milli[r];
    }
}

// a pod's share added to its node's accumulator row
__device__ inline void util_sum_add(UtilSum& a, const int64_t (&req)[3], const int64_t (&dsm)[3], int drain) {
    for (int r = 0; r < 3; r++) {
        if (req[r]) atomicAdd(&a.req[r], (unsigned long long)req[r]);
        if (dsm[r]) atomicAdd(&a.dsm[r], (unsigned long long)dsm[r]);
    }
    if (drain) atomicOr(&a.drain, drain);
}

// the node's Info from its sums (info.go:48-94) and the FindEmptyNodesToRemove verdict
// (cluster.go:197-199)
__device__ inline ca_util_info node_info(const ca_util_node& nd, const int64_t (&req)[3], const int64_t (&dsm)[3],
                                         int drain) {
    ca_util_info o;
    o.cpu = o.mem = o.gpu = o.utilization = 0.0;
    o.resource = CA_UTIL_CPU;
    o.status = CA_UTIL_OK;
    o._pad = 0;
    o.empty = drain == 0;                                         // cluster.go:197-199
    if (nd.flags & CA_UNODE_GPU_CONFIG) {                         // info.go:49-58
        o.resource = CA_UTIL_GPU;
        if ((nd.flags & CA_UNODE_HAS_GPU) && nd.alloc_milli[2] != 0) {
            o.gpu = util_ratio(req[2], nd.alloc_milli[2], dsm[2]);
            o.utilization = o.gpu;
        }                                                         // unready GPU: Info{Gpu 0, Util 0}, nil
    } else if (!(nd.flags & CA_UNODE_HAS_CPU)) {                  // info.go:88-94 -> Info{}, err
        o.status = CA_UTIL_NO_CPU;
    } else if (nd.alloc_milli[0] == 0) {
        o.status = CA_UTIL_ZERO_CPU;
    } else if (!(nd.flags & CA_UNODE_HAS_MEM)) {
        o.status = CA_UTIL_NO_MEM;
    } else if (nd.alloc_milli[1] == 0) {
        o.status = CA_UTIL_ZERO_MEM;
    } else {                                                      // info.go:61-80
        o.cpu = util_ratio(req[0], nd.alloc_milli[0], dsm[0]);
        o.mem = util_ratio(req[1], nd.alloc_milli[1], dsm[1]);
        if (o.cpu > o.mem) { o.resource = CA_UTIL_CPU; o.utilization = o.cpu; }
        else               { o.resource = CA_UTIL_MEM; o.utilization = o.mem; }
    }
    return o;
}

}  // namespace casim
