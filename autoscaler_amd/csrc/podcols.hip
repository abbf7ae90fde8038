// podcols.hip — the resident per-pod columns of the mirror: pod -> node, the pod's slot in its
// node's NodeInfo.Pods list, and the util row its caller set (with a has-row flag).
//
// The host rows stay authoritative.  Every mutation that changes a pod's node or slot marks
// the pod (ca_mirror::pcol_mark); ids at or above the synced count are a tail and go up from
// the host state at sync, so appends (add_pods, FilterOutSchedulable's placements, the
// planner's copies) mark nothing.  sync_pod_cols uploads the tail as contiguous ranges, the
// marked ids as (id, node, slot) entries behind a scatter kernel, or everything when more than
// max(1024, P/4) ids are stale.  Util rows go up as (id, row, flag) entries behind their own
// scatter.  The dirty set, the staging builders and the argument checks are podcols_host.h.
#include "mirror.h"

#include <chrono>
#include <cstring>

using namespace casim;

namespace {

constexpr int kThreads = 256;

inline size_t al64(size_t b) { return (b + 63) & ~(size_t)63; }
inline unsigned blocks_of(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// (id, node, slot) entries into the columns; no id occurs twice
__global__ __launch_bounds__(kThreads) void k_podcol_scatter(const PodColEntry* __restrict__ e, int32_t k,
                                                             int32_t* __restrict__ node, int32_t* __restrict__ slot,
                                                             int32_t n_pods) {
    const int32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= k) return;
    const PodColEntry v = e[i];
    if ((uint32_t)v.id >= (uint32_t)n_pods) return;
    node[v.id] = v.node;
    slot[v.id] = v.slot;
}

// (id, row, flag) entries into the util rows and the has-row flags; no id occurs twice
__global__ __launch_bounds__(kThreads) void k_podrow_scatter(const PodRowEntry* __restrict__ e, int32_t k,
                                                             ca_util_pod* __restrict__ rows, uint8_t* __restrict__ has,
                                                             int32_t n_pods) {
    const int32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= k) return;
    const PodRowEntry v = e[i];
    if ((uint32_t)v.id >= (uint32_t)n_pods) return;
    rows[v.id] = v.row;
    has[v.id] = (uint8_t)(v.has != 0);
}

// ca_mirror_reorder_nodes: the node column through the inverse permutation (slots do not change)
__global__ __launch_bounds__(kThreads) void k_podcol_reorder(int32_t* __restrict__ node, int32_t n_pods,
                                                             const int32_t* __restrict__ inv, int32_t n) {
    const int32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_pods) return;
    const int32_t v = node[i];
    if (v >= 0 && v < n) node[i] = inv[v];
}

}  // namespace

int ca_mirror::ensure_pod_cols() {
    if (pcol) return CA_OK;
    CA_HIP_CHECK(hipSetDevice(device));
    std::unique_ptr<PodCols> c(new PodCols());
    CA_HIP_CHECK(hipEventCreate(&c->ev));
    c->rdirty.full = true;
    pcol = std::move(c);
    return CA_OK;
}

int ca_mirror::reorder_pod_cols(const int32_t* d_inv, int32_t n) {
    PodCols& c = *pcol;
    hipLaunchKernelGGL(k_podcol_reorder, dim3(blocks_of(c.dirty.synced)), dim3(kThreads), 0, stream,
                       c.d_node.as<int32_t>(), (int32_t)c.dirty.synced, d_inv, n);
    CA_HIP_CHECK(hipGetLastError());
    c.stat[PodCols::ST_REORDERS]++;
    return CA_OK;
}

int ca_mirror::sync_pod_cols() {
    PodCols& c = *pcol;
    const size_t P = pods.size(), synced = c.dirty.synced;
    const int np = c.dirty.plan(P), rp = c.rdirty.plan(P);
    if (np == PodColDirty::SYNC_NONE && rp == PodColDirty::SYNC_NONE && synced == P) return CA_OK;
    int rc;
    if (c.cap < P) {
        const size_t cap = std::max(P, c.cap * 2);
        if ((rc = c.d_node.reserve_keep(sizeof(int32_t) * cap, stream)) != CA_OK ||
            (rc = c.d_slot.reserve_keep(sizeof(int32_t) * cap, stream)) != CA_OK ||
            (rc = c.d_has.reserve_keep(cap, stream)) != CA_OK ||
            (rc = c.d_row.reserve_keep(sizeof(ca_util_pod) * cap, stream)) != CA_OK)
            return rc;
        c.cap = cap;
    }
    c.rows.grow(P);
    // ranges [lo, P) go up whole; below them the marked ids' entries
    const size_t lo_n = np == PodColDirty::SYNC_FULL ? 0 : synced, lo_r = rp == PodColDirty::SYNC_FULL ? 0 : synced;
    const size_t k_n = np == PodColDirty::SYNC_STAGED ? c.dirty.ids.size() : 0;
    std::vector<int32_t> row_ids;
    if (rp == PodColDirty::SYNC_STAGED) row_ids = c.rdirty.ids;
    for (size_t id = lo_r; id < P; id++)
        if (c.rows.has[id]) row_ids.push_back((int32_t)id);
    const size_t k_r = row_ids.size();
    const size_t o_node = 0, o_slot = o_node + al64(sizeof(int32_t) * (P - lo_n)),
                 o_has = o_slot + al64(sizeof(int32_t) * (P - lo_n)), o_ent = o_has + al64(P - lo_r),
                 o_row = o_ent + al64(sizeof(PodColEntry) * k_n), bytes = o_row + al64(sizeof(PodRowEntry) * k_r);
    // (an earlier sync's copies out of the staging are done)
    CA_HIP_CHECK(hipStreamSynchronize(stream));
    if ((rc = c.h_stage.reserve(bytes + 64)) != CA_OK || (rc = c.d_stage.reserve(bytes - o_ent + 64)) != CA_OK) return rc;
    unsigned char* h = c.h_stage.as<unsigned char>();
    auto node_of = [&](int32_t id) { return pods[(size_t)id].node; };
    auto pods_of = [&](int32_t x) -> const std::vector<int32_t>& { return nodes[(size_t)x].pods; };
    int32_t* hn = reinterpret_cast<int32_t*>(h + o_node);
    int32_t* hs = reinterpret_cast<int32_t*>(h + o_slot);
    if (lo_n == 0) podcol_fill_full(P, nodes.size(), pods_of, hn, hs);
    else podcol_fill_range(lo_n, P, node_of, pods_of, hn, hs);
    if (P > lo_r) std::memcpy(h + o_has, c.rows.has.data() + lo_r, P - lo_r);
    if (k_n > 0) podcol_build_stage(c.dirty.ids, node_of, pods_of, reinterpret_cast<PodColEntry*>(h + o_ent));
    PodRowEntry* hr = reinterpret_cast<PodRowEntry*>(h + o_row);
    for (size_t k = 0; k < k_r; k++) hr[k] = c.rows.entry(row_ids[k]);

    int64_t up = 0;
    if (P > lo_n) {
        CA_HIP_CHECK(hipMemcpyAsync(c.d_node.as<int32_t>() + lo_n, hn, sizeof(int32_t) * (P - lo_n), hipMemcpyHostToDevice, stream));
        CA_HIP_CHECK(hipMemcpyAsync(c.d_slot.as<int32_t>() + lo_n, hs, sizeof(int32_t) * (P - lo_n), hipMemcpyHostToDevice, stream));
        up += (int64_t)(2 * sizeof(int32_t) * (P - lo_n));
    }
    if (P > lo_r) {
        CA_HIP_CHECK(hipMemcpyAsync(c.d_has.as<uint8_t>() + lo_r, h + o_has, P - lo_r, hipMemcpyHostToDevice, stream));
        up += (int64_t)(P - lo_r);
    }
    if (k_n + k_r > 0) {
        unsigned char* d = c.d_stage.as<unsigned char>();
        CA_HIP_CHECK(hipMemcpyAsync(d, h + o_ent, bytes - o_ent, hipMemcpyHostToDevice, stream));
        up += (int64_t)(sizeof(PodColEntry) * k_n + sizeof(PodRowEntry) * k_r);
        if (k_n > 0) {
            hipLaunchKernelGGL(k_podcol_scatter, dim3(blocks_of(k_n)), dim3(kThreads), 0, stream,
                               reinterpret_cast<const PodColEntry*>(d), (int32_t)k_n, c.d_node.as<int32_t>(),
                               c.d_slot.as<int32_t>(), (int32_t)P);
            CA_HIP_CHECK(hipGetLastError());
        }
        if (k_r > 0) {
            hipLaunchKernelGGL(k_podrow_scatter, dim3(blocks_of(k_r)), dim3(kThreads), 0, stream,
                               reinterpret_cast<const PodRowEntry*>(d + (o_row - o_ent)), (int32_t)k_r,
                               c.d_row.as<ca_util_pod>(), c.d_has.as<uint8_t>(), (int32_t)P);
            CA_HIP_CHECK(hipGetLastError());
        }
    }
    if (np == PodColDirty::SYNC_FULL) c.stat[PodCols::ST_FULL]++;
    else c.stat[PodCols::ST_TAIL] += (int64_t)(P - synced);
    if (np == PodColDirty::SYNC_STAGED) { c.stat[PodCols::ST_STAGED]++; c.stat[PodCols::ST_ENTRIES] += (int64_t)k_n; }
    c.stat[PodCols::ST_ROWS] += (int64_t)k_r;
    c.stat[PodCols::ST_BYTES] += up;
    c.dirty.done(P);
    c.rdirty.done(P);
    return CA_OK;
}

extern "C" {

int ca_mirror_set_pod_util_rows(ca_mirror* m, const int32_t* pod_ids, const ca_util_pod* rows, int32_t n) {
    if (!m || check_pod_row_ids(pod_ids, n, (int64_t)m->pods.size()) != CA_OK) return CA_EINVAL;
    int rc = m->ensure_pod_cols();
    if (rc != CA_OK) return rc;
    PodCols& c = *m->pcol;
    for (int32_t k = 0; k < n; k++)
        if (c.rows.set(pod_ids[k], rows ? rows + k : nullptr)) c.rdirty.mark(pod_ids[k]);
    return CA_OK;
}

int ca_mirror_get_pod_util_rows(ca_mirror* m, const int32_t* pod_ids, ca_util_pod* rows, uint8_t* has_row, int32_t n) {
    if (!m || check_pod_row_ids(pod_ids, n, (int64_t)m->pods.size()) != CA_OK) return CA_EINVAL;
    for (int32_t k = 0; k < n; k++) {
        const PodRowEntry e = m->pcol ? m->pcol->rows.entry(pod_ids[k]) : PodRowTable().entry(pod_ids[k]);
        if (rows) rows[k] = e.row;
        if (has_row) has_row[k] = (uint8_t)e.has;
    }
    return CA_OK;
}

int ca_mirror_fetch_pod_columns(ca_mirror* m, int32_t* node, int32_t* slot, int32_t n_pods) {
    if (!m || n_pods < 0 || (size_t)n_pods != m->pods.size() || (n_pods > 0 && (!node || !slot))) return CA_EINVAL;
    int rc = m->ensure_pod_cols();
    if (rc != CA_OK) return rc;
    CA_HIP_CHECK(hipSetDevice(m->device));
    if ((rc = m->sync_pod_cols()) != CA_OK) return rc;
    if (n_pods > 0) {
        CA_HIP_CHECK(hipMemcpyAsync(node, m->pcol->d_node.ptr, sizeof(int32_t) * n_pods, hipMemcpyDeviceToHost, m->stream));
        CA_HIP_CHECK(hipMemcpyAsync(slot, m->pcol->d_slot.ptr, sizeof(int32_t) * n_pods, hipMemcpyDeviceToHost, m->stream));
    }
    CA_HIP_CHECK(hipStreamSynchronize(m->stream));
    return CA_OK;
}

int ca_mirror_pod_count(const ca_mirror* m, int32_t* out) {
    if (!m || !out) return CA_EINVAL;
    *out = (int32_t)m->pods.size();
    return CA_OK;
}

int ca_mirror_pod_column_stats(const ca_mirror* m, int64_t* out, int32_t cap) {
    if (!m || (!out && cap > 0)) return CA_EINVAL;
    for (int32_t i = 0; i < cap && i < PodCols::ST_N; i++) out[i] = m->pcol ? m->pcol->stat[i] : 0;
    return PodCols::ST_N;
}

}  // extern "C"
