// scaledown.hip — scale-down eligibility from the mirror's own state.
//
// ca_mirror_utilization: utilization.Calculate (CA/simulator/utilization/info.go:48-127) for
// every node of the mirror, from the resident pod records (ca_pod_spec.score_*, the
// containers-only sums, and CA_POD_DAEMONSET) and the pod -> node column, with the caller's
// override rows for what the mirror cannot know.  One thread per mirror pod id adds its share
// into its node's UtilSum row with integer atomics (order-free, so bit-exact), one thread per
// node turns the row into its ca_util_info (util_core.h node_info: the same function as the
// table form's) and clears it.
//
// ca_scale_down_candidates: the nodes classified against the thresholds on the device, the
// empty and the non-empty ones compacted in position order by one workgroup's scan, and the
// candidates' pods to move listed on the host in NodeInfo.Pods order (NodeRow.pods), ready for
// ca_removal_plan_create.
//
// The resident forms (ca_mirror_utilization_resident, ca_scale_down_candidates_create_resident)
// read the pod -> node, slot and util-row columns podcols.hip keeps on the device instead of a
// per-call staging fill, and list the pods to move on the device: a slot table over the
// candidates' NodeInfo.Pods positions, compacted in order in tiles of 2048 entries.
#include "mirror.h"
#include "util_core.h"
#include "scaledown_host.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

using namespace casim;

struct ca_scale_down_candidates {
    ca_mirror* m = nullptr;
    int64_t order_epoch = 0;               // the mirror's node order the positions are in
    int32_t n_nodes = 0;
    std::vector<ca_util_info> info;
    std::vector<uint8_t> cls;              // CA_SD_* per node
    std::vector<int32_t> empty, cand, status;
    std::vector<int32_t> cand_of;          // node position -> index in cand, -1 for the others
    std::vector<int32_t> move_off, move_pods;
    float t[7] = {0, 0, 0, 0, 0, 0, 0};    // ca_scale_down_candidates_timings
};

namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;         // the compaction's one workgroup
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kTile = 2048;                // slot-table entries per compaction tile
constexpr int kTilePer = kTile / kThreads; // ... per thread, contiguous
// counts[] of k_classify_compact, continued by the move-list kernels
enum { CN_EMPTY = 0, CN_CAND, CN_TABLE, CN_MOVES, CN_BAD };

inline size_t al64(size_t b) { return (b + 63) & ~(size_t)63; }

// byte offsets of one call's inputs in UtilScratch::in / h_in
struct InLayout {
    size_t pod_node, nodes, ids, rows, bits, eligible, bytes;
    // resident: the pod -> node column is on the device already; its place holds the nodes'
    // pod counts, and the overrides are found by binary search alone (no bitmap)
    InLayout(size_t n_nodes, size_t n_pods, size_t n_over, bool elig, bool resident = false) {
        pod_node = 0;
        nodes = al64(sizeof(int32_t) * (resident ? n_nodes : n_pods));
        ids = nodes + al64(sizeof(ca_util_node) * n_nodes);
        rows = ids + al64(sizeof(int32_t) * n_over);
        bits = rows + al64(sizeof(ca_util_pod) * n_over);
        eligible = bits + (n_over && !resident ? al64(sizeof(uint32_t) * ((n_pods + 31) / 32)) : 0);
        bytes = eligible + (elig ? al64(n_nodes) : 0);
    }
};

// One thread per mirror pod id: the pod's row (its override, or the default from its
// record), its share (pod_share), added to its node's sums.
__global__ __launch_bounds__(kThreads) void k_mirror_pod_sums(
    const int32_t* __restrict__ pod_node, const ca_pod_spec* __restrict__ specs, int32_t n_pods, int32_t n_nodes,
    const uint32_t* __restrict__ over_bits, const int32_t* __restrict__ over_ids,
    const ca_util_pod* __restrict__ over_rows, int32_t n_over, int32_t skip_ds, int32_t skip_mirror, int64_t now_ns,
    UtilSum* __restrict__ acc) {
    const int32_t id = blockIdx.x * kThreads + threadIdx.x;
    if (id >= n_pods) return;
    const int32_t x = pod_node[id];
    if ((uint32_t)x >= (uint32_t)n_nodes) return;                 // on no node
    ca_util_pod p;
    if (over_bits && ((over_bits[id >> 5] >> (id & 31)) & 1u)) {
        int32_t lo = 0, hi = n_over - 1;                          // the marked id is in the sorted list
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (over_ids[mid] < id) lo = mid + 1; else hi = mid;
        }
        p = over_rows[lo];
    } else {
        const ca_pod_spec& s = specs[id];
        p.req_milli[0] = s.score_milli_cpu;
        p.req_milli[1] = (int64_t)((uint64_t)s.score_memory * 1000ull);   // Value() -> MilliValue(), wrapping
        p.req_milli[2] = 0;
        p.deletion_ns = p.grace_s = 0;
        p.flags = (s.flags & CA_POD_DAEMONSET) ? CA_UPOD_DAEMONSET : CA_UPOD_MOVABLE;
        p._pad = 0;
    }
    int64_t req[3] = {0, 0, 0}, dsm[3] = {0, 0, 0};
    int drain = 0;
    pod_share(p, skip_ds, skip_mirror, now_ns, req, dsm, drain);
    util_sum_add(acc[x], req, dsm, drain);
}

// The row of pod `id` for the resident forms: the call's override (binary search, only when the
// call has any), else the resident row, else the default from the record.
__device__ inline ca_util_pod resident_row(int32_t id, const ca_pod_spec* __restrict__ specs,
                                           const int32_t* __restrict__ over_ids,
                                           const ca_util_pod* __restrict__ over_rows, int32_t n_over,
                                           const uint8_t* __restrict__ has_row, const ca_util_pod* __restrict__ rows) {
    if (n_over > 0) {
        int32_t lo = 0, hi = n_over - 1;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (over_ids[mid] < id) lo = mid + 1; else hi = mid;
        }
        if (over_ids[lo] == id) return over_rows[lo];
    }
    if (has_row[id]) return rows[id];
    const ca_pod_spec& s = specs[id];
    ca_util_pod p;
    p.req_milli[0] = s.score_milli_cpu;
    p.req_milli[1] = (int64_t)((uint64_t)s.score_memory * 1000ull);       // Value() -> MilliValue(), wrapping
    p.req_milli[2] = 0;
    p.deletion_ns = p.grace_s = 0;
    p.flags = (s.flags & CA_POD_DAEMONSET) ? CA_UPOD_DAEMONSET : CA_UPOD_MOVABLE;
    p._pad = 0;
    return p;
}

// k_mirror_pod_sums from the resident columns: one thread per mirror pod id.
__global__ __launch_bounds__(kThreads) void k_mirror_pod_sums_resident(
    const int32_t* __restrict__ pod_node, const uint8_t* __restrict__ has_row, const ca_util_pod* __restrict__ rows,
    const ca_pod_spec* __restrict__ specs, int32_t n_pods, int32_t n_nodes, const int32_t* __restrict__ over_ids,
    const ca_util_pod* __restrict__ over_rows, int32_t n_over, int32_t skip_ds, int32_t skip_mirror, int64_t now_ns,
    UtilSum* __restrict__ acc) {
    const int32_t id = blockIdx.x * kThreads + threadIdx.x;
    if (id >= n_pods) return;
    const int32_t x = pod_node[id];
    if ((uint32_t)x >= (uint32_t)n_nodes) return;                 // on no node
    const ca_util_pod p = resident_row(id, specs, over_ids, over_rows, n_over, has_row, rows);
    int64_t req[3] = {0, 0, 0}, dsm[3] = {0, 0, 0};
    int drain = 0;
    pod_share(p, skip_ds, skip_mirror, now_ns, req, dsm, drain);
    util_sum_add(acc[x], req, dsm, drain);
}

// Exclusive scan of one value per thread over a workgroup of W waves (wave shuffles, the
// waves' sums through LDS); `total` is the workgroup's sum in every thread.  Ends in a barrier,
// so `lds` can be used again at once.
template <int W>
__device__ inline int32_t block_excl_scan(int32_t v, int32_t* lds, int32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int32_t before = 0;
    total = 0;
    for (int w = 0; w < W; w++) {
        if (w == wave) before = total;
        total += lds[w];
    }
    __syncthreads();
    return before + inc - v;
}

// Move lists, step 1: node position -> index among the candidates (-1 for the others).
__global__ __launch_bounds__(kThreads) void k_cand_map(const uint8_t* __restrict__ cls, const int32_t* __restrict__ cand,
                                                       const int32_t* __restrict__ counts, int32_t n,
                                                       int32_t* __restrict__ cand_of) {
    const int32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (cls[i] != CA_SD_CANDIDATE) cand_of[i] = -1;
    if (i < counts[CN_CAND]) {
        const int32_t x = cand[i];
        if ((uint32_t)x < (uint32_t)n) cand_of[x] = i;
    }
}

// Step 2: the candidates' offsets in the slot table, an exclusive scan of their nodes' pod
// counts in candidate order (one workgroup, 1024 candidates a step).  off[n_cand] and
// counts[CN_TABLE] get the table's size; the other move-list counters start at 0.
__global__ __launch_bounds__(kScanThreads) void k_cand_offsets(const int32_t* __restrict__ cand,
                                                               const int32_t* __restrict__ node_pods, int32_t n,
                                                               int32_t table_cap, int32_t* __restrict__ off,
                                                               int32_t* __restrict__ counts) {
    __shared__ int32_t lds[kScanWaves];
    const int32_t nc = min(counts[CN_CAND], n);
    int32_t base = 0;                                             // the same in every thread
    for (int32_t c0 = 0; c0 < nc; c0 += kScanThreads) {
        const int32_t c = c0 + (int32_t)threadIdx.x;
        int32_t v = 0;
        if (c < nc) {
            const int32_t x = cand[c];
            if ((uint32_t)x < (uint32_t)n) v = max(node_pods[x], 0);
        }
        int32_t total;
        const int32_t ex = block_excl_scan<kScanWaves>(v, lds, total);
        if (c < nc) off[c] = base + ex;
        base += total;
    }
    if (threadIdx.x == 0) {
        off[nc] = base;
        counts[CN_TABLE] = base > table_cap ? 0 : base;
        counts[CN_MOVES] = 0;
        counts[CN_BAD] = base > table_cap ? 1 : 0;                // the counts do not add up to the pods on nodes
    }
}

// Step 3: every pod on a candidate writes its id at its NodeInfo.Pods position when its row is
// movable.  A slot outside its node's list is not written and raises counts[CN_BAD].
__global__ __launch_bounds__(kThreads) void k_slot_table(
    const int32_t* __restrict__ pod_node, const int32_t* __restrict__ pod_slot, const uint8_t* __restrict__ has_row,
    const ca_util_pod* __restrict__ rows, const ca_pod_spec* __restrict__ specs, int32_t n_pods, int32_t n_nodes,
    const int32_t* __restrict__ over_ids, const ca_util_pod* __restrict__ over_rows, int32_t n_over,
    const int32_t* __restrict__ cand_of, const int32_t* __restrict__ off, const int32_t* __restrict__ node_pods,
    int32_t table_cap, int32_t* __restrict__ table, int32_t* __restrict__ counts) {
    const int32_t id = blockIdx.x * kThreads + threadIdx.x;
    if (id >= n_pods) return;
    const int32_t x = pod_node[id];
    if ((uint32_t)x >= (uint32_t)n_nodes) return;
    const int32_t c = cand_of[x];
    if (c < 0) return;
    const int32_t s = pod_slot[id];
    const int64_t at = (int64_t)off[c] + s;
    if (s < 0 || s >= node_pods[x] || at >= (int64_t)table_cap || counts[CN_BAD]) {
        counts[CN_BAD] = 1;                                       // pod columns out of sync
        return;
    }
    uint32_t flags;
    if (n_over == 0 && !has_row[id]) flags = (specs[id].flags & CA_POD_DAEMONSET) ? CA_UPOD_DAEMONSET : CA_UPOD_MOVABLE;
    else flags = resident_row(id, specs, over_ids, over_rows, n_over, has_row, rows).flags;
    if (flags & CA_UPOD_MOVABLE) table[at] = id;
}

// Step 4a: the filled entries of each tile of 2048.
__global__ __launch_bounds__(kThreads) void k_tile_count(const int32_t* __restrict__ table,
                                                         const int32_t* __restrict__ counts,
                                                         int32_t* __restrict__ tile_cnt) {
    __shared__ int32_t lds[kThreads / 64];
    const int32_t p0 = (int32_t)blockIdx.x * kTile + (int32_t)threadIdx.x * kTilePer;
    int32_t v = 0;
    if (p0 < counts[CN_TABLE])                                    // (the table is padded to whole tiles with -1)
        for (int j = 0; j < kTilePer; j++) v += table[p0 + j] >= 0;
    int32_t total;
    (void)block_excl_scan<kThreads / 64>(v, lds, total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// Step 4b: the tiles' bases (one workgroup) and the number of pods to move.
__global__ __launch_bounds__(kScanThreads) void k_tile_scan(const int32_t* __restrict__ tile_cnt, int32_t n_tiles,
                                                            int32_t* __restrict__ tile_base,
                                                            int32_t* __restrict__ counts) {
    __shared__ int32_t lds[kScanWaves];
    int32_t base = 0;
    for (int32_t t0 = 0; t0 < n_tiles; t0 += kScanThreads) {
        const int32_t t = t0 + (int32_t)threadIdx.x;
        int32_t total;
        const int32_t ex = block_excl_scan<kScanWaves>(t < n_tiles ? tile_cnt[t] : 0, lds, total);
        if (t < n_tiles) tile_base[t] = base + ex;
        base += total;
    }
    if (threadIdx.x == 0) counts[CN_MOVES] = base;
}

// Step 4c: the filled entries in table order into lists[n_cand + 1 ...], and every table
// position's rank among them (the candidates' offsets into the list, k_move_off).
__global__ __launch_bounds__(kThreads) void k_tile_write(const int32_t* __restrict__ table,
                                                         const int32_t* __restrict__ counts,
                                                         const int32_t* __restrict__ tile_base,
                                                         int32_t* __restrict__ rank, int32_t* __restrict__ lists) {
    __shared__ int32_t lds[kThreads / 64];
    const int32_t p0 = (int32_t)blockIdx.x * kTile + (int32_t)threadIdx.x * kTilePer;
    if ((int32_t)blockIdx.x * kTile >= counts[CN_TABLE]) return;  // (the whole workgroup)
    int32_t e[kTilePer], v = 0;
    for (int j = 0; j < kTilePer; j++) { e[j] = table[p0 + j]; v += e[j] >= 0; }
    int32_t total;
    int32_t r = tile_base[blockIdx.x] + block_excl_scan<kThreads / 64>(v, lds, total);
    int32_t* moves = lists + counts[CN_CAND] + 1;
    for (int j = 0; j < kTilePer; j++) {
        rank[p0 + j] = r;
        if (e[j] >= 0) moves[r++] = e[j];
    }
}

// Step 4d: move_off[c] = the rank of candidate c's first table position.
__global__ __launch_bounds__(kThreads) void k_move_off(const int32_t* __restrict__ off, const int32_t* __restrict__ counts,
                                                       const int32_t* __restrict__ rank, int32_t n,
                                                       int32_t* __restrict__ lists) {
    const int32_t c = blockIdx.x * kThreads + threadIdx.x;
    if (c > min(counts[CN_CAND], n)) return;
    const int32_t p = off[c];
    lists[c] = p < counts[CN_TABLE] ? rank[p] : counts[CN_MOVES];
}

// One thread per node: its sums (read and cleared) and its row -> ca_util_info and drain bits.
__global__ __launch_bounds__(kThreads) void k_mirror_node_util(const ca_util_node* __restrict__ nodes, int32_t n_nodes,
                                                               UtilSum* __restrict__ acc, ca_util_info* __restrict__ out,
                                                               int32_t* __restrict__ out_drain,
                                                               ca_util_info* __restrict__ out_host) {
    const int32_t node = blockIdx.x * kThreads + threadIdx.x;
    if (node >= n_nodes) return;
    const UtilSum a = acc[node];
    if (a.drain | a.req[0] | a.req[1] | a.req[2] | a.dsm[0] | a.dsm[1] | a.dsm[2]) acc[node] = UtilSum{};
    int64_t req[3], dsm[3];
    for (int r = 0; r < 3; r++) { req[r] = (int64_t)a.req[r]; dsm[r] = (int64_t)a.dsm[r]; }
    const ca_util_info o = node_info(nodes[node], req, dsm, a.drain);
    out[node] = o;
    out_drain[node] = a.drain;
    if (out_host) out_host[node] = o;                             // page-locked caller rows (zero-copy)
}

// The nodes' classes and the ordered compaction of the empty ones and the candidates: one
// workgroup walks the nodes 1024 at a time (ballots per wave, the waves' counts through LDS,
// a running base), so both lists come out in ascending position.  15 000 nodes are 15 steps.
__global__ __launch_bounds__(kScanThreads) void k_classify_compact(
    const ca_util_info* __restrict__ info, const int32_t* __restrict__ drain, const uint8_t* __restrict__ eligible,
    int32_t n, double thr, double gpu_thr, uint8_t* __restrict__ cls, int32_t* __restrict__ empty,
    int32_t* __restrict__ cand, int32_t* __restrict__ cand_status, int32_t* __restrict__ counts) {
    __shared__ int32_t w_e[kScanWaves], w_c[kScanWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t base_e = 0, base_c = 0;                               // the same in every thread
    for (int32_t t0 = 0; t0 < n; t0 += kScanThreads) {
        const int32_t i = t0 + (int32_t)threadIdx.x;
        int c = -1, dr = 0;
        if (i < n) {
            const ca_util_info o = info[i];
            dr = drain[i];
            if (eligible && !eligible[i]) c = CA_SD_INELIGIBLE;
            else if (o.status != CA_UTIL_OK) c = CA_SD_UTIL_ERROR;
            else if (o.utilization >= (o.resource == CA_UTIL_GPU ? gpu_thr : thr)) c = CA_SD_NOT_BELOW;   // eligibility.go:158-178
            else c = dr == 0 ? CA_SD_EMPTY : CA_SD_CANDIDATE;
            cls[i] = (uint8_t)c;
        }
        const bool is_e = c == CA_SD_EMPTY, is_c = c == CA_SD_CANDIDATE;
        const unsigned long long be = __ballot(is_e), bc = __ballot(is_c);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (lane == 0) { w_e[wave] = __popcll(be); w_c[wave] = __popcll(bc); }
        __syncthreads();
        int32_t oe = base_e, oc = base_c, te = 0, tc = 0;
        for (int w = 0; w < kScanWaves; w++) {
            if (w == wave) { oe += te; oc += tc; }
            te += w_e[w];
            tc += w_c[w];
        }
        if (is_e) empty[oe + __popcll(be & below)] = i;
        if (is_c) {
            const int32_t k = oc + __popcll(bc & below);
            cand[k] = i;
            cand_status[k] = (dr & CA_UPOD_BLOCKING) ? CA_UNREMOVABLE_BLOCKED_BY_POD : 0;
        }
        base_e += te;
        base_c += tc;
        __syncthreads();                                          // w_e / w_c are rewritten by the next step
    }
    if (threadIdx.x == 0) { counts[0] = base_e; counts[1] = base_c; }
}

int check_args(const ca_mirror* m, const ca_mirror_util_args* a) {
    if (!m) return CA_EINVAL;
    return check_util_args(a, (int64_t)m->nodes.size(), (int64_t)m->pods.size());
}

// acc back to all zero after a call that may have left sums in it
void clear_acc(ca_mirror* m) {
    UtilScratch& u = m->ut;
    (void)hipStreamSynchronize(m->stream);
    if (u.acc_rows == 0 ||
        (hipMemsetAsync(u.acc.ptr, 0, sizeof(UtilSum) * u.acc_rows, m->stream) == hipSuccess &&
         hipStreamSynchronize(m->stream) == hipSuccess))
        u.acc_dirty = false;
    (void)hipGetLastError();
}

#define UT_CHECK(expr)                                                             \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) {                                                    \
            casim::set_last_error(std::string(#expr) + ": " + hipGetErrorString(_e)); \
            clear_acc(m);                                                          \
            return CA_EDEVICE;                                                     \
        }                                                                          \
    } while (0)

// The body of ca_mirror_utilization.  `eligible` ([n_nodes] or NULL) rides along in the input
// copy for ca_scale_down_candidates_create, which passes finish = false: the kernels are left
// queued on the mirror's stream (events ev0 / ev1 around them), the caller queues its own work
// behind them, syncs, and clears acc_dirty.  resident: the pod kernel reads the resident
// columns (brought up to date here) and the staging carries the nodes' pod counts instead of
// the pod -> node column.
int util_run(ca_mirror* m, const ca_mirror_util_args* a, ca_util_info* out, int32_t* out_drain, float* kernel_ms,
             const uint8_t* eligible, bool finish, bool resident = false) {
    int st = check_args(m, a);
    if (st != CA_OK) return st;
    if (resident && (st = m->ensure_pod_cols()) != CA_OK) return st;
    UtilScratch& u = m->ut;
    const size_t n_nodes = m->nodes.size(), n_pods = m->pods.size(), n_over = (size_t)a->n_pod_rows;
    if (kernel_ms) *kernel_ms = 0.0f;
    u.stage_ms = 0;
    u.h2d_bytes = u.d2h_bytes = 0;
    u.n_nodes = (int32_t)n_nodes;
    if (n_nodes == 0) return CA_OK;
    CA_HIP_CHECK(hipSetDevice(m->device));
    const InLayout L(n_nodes, n_pods, n_over, eligible != nullptr, resident);
    if ((st = u.h_in.reserve(L.bytes + 64)) != CA_OK) return st;
    unsigned char* h = u.h_in.as<unsigned char>();

    // node rows: the default from the node's allocatable, or the caller's
    ca_util_node* hn = reinterpret_cast<ca_util_node*>(h + L.nodes);
    for (size_t i = 0, k = 0; i < n_nodes; i++) {
        if (k < (size_t)a->n_node_rows && (size_t)a->node_pos[k] == i) { hn[i] = a->node_rows[k++]; continue; }
        const ca_node_spec& s = m->nodes[i].spec;
        ca_util_node r;
        r.alloc_milli[0] = s.alloc_milli_cpu;
        if (__builtin_mul_overflow(s.alloc_memory, (int64_t)1000, &r.alloc_milli[1])) return CA_EUNSUPPORTED;
        r.alloc_milli[2] = 0;
        r.flags = CA_UNODE_HAS_CPU | CA_UNODE_HAS_MEM;
        r._pad = 0;
        hn[i] = r;
    }
    // the pod -> node column (PodRow.node lives in the chunked host records); the resident
    // forms send each node's pod count in its place
    const auto t0 = std::chrono::steady_clock::now();
    int32_t* hp = reinterpret_cast<int32_t*>(h + L.pod_node);
    const int32_t T = (int32_t)std::min<size_t>(8, n_pods >> 16);
    if (resident) {
        u.table_pods = 0;
        for (size_t i = 0; i < n_nodes; i++) {
            hp[i] = (int32_t)m->nodes[i].pods.size();
            u.table_pods += m->nodes[i].pods.size();
        }
    } else if (T > 1) {
        parallel_run(T, [&](int32_t w) {
            const size_t b = n_pods * (size_t)w / (size_t)T, e = n_pods * ((size_t)w + 1) / (size_t)T;
            for (size_t i = b; i < e; i++) hp[i] = m->pods[i].node;
        });
    } else {
        for (size_t i = 0; i < n_pods; i++) hp[i] = m->pods[i].node;
    }
    u.stage_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (n_over) {
        std::memcpy(h + L.ids, a->pod_ids, sizeof(int32_t) * n_over);
        std::memcpy(h + L.rows, a->pod_rows, sizeof(ca_util_pod) * n_over);
    }
    if (n_over && !resident) {
        uint32_t* bits = reinterpret_cast<uint32_t*>(h + L.bits);
        std::memset(bits, 0, sizeof(uint32_t) * ((n_pods + 31) / 32));
        for (size_t k = 0; k < n_over; k++) bits[a->pod_ids[k] >> 5] |= 1u << (a->pod_ids[k] & 31);
    }
    if (eligible) std::memcpy(h + L.eligible, eligible, n_nodes);

    if ((st = m->sync_pods()) != CA_OK) return st;
    if (resident) {
        const auto t1 = std::chrono::steady_clock::now();
        if ((st = m->sync_pod_cols()) != CA_OK) return st;
        u.stage_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
    }
    if ((st = u.in.reserve(L.bytes + 64)) != CA_OK || (st = u.info.reserve(sizeof(ca_util_info) * n_nodes)) != CA_OK ||
        (st = u.drain.reserve(sizeof(int32_t) * n_nodes)) != CA_OK)
        return st;
    if (u.acc_rows < n_nodes) {                                   // new rows start zero, like the old ones
        const size_t rows = std::max(n_nodes, u.acc_rows * 2);
        u.acc_rows = 0;
        if ((st = u.acc.reserve(sizeof(UtilSum) * rows)) != CA_OK) return st;
        u.acc_rows = rows;
        u.acc_dirty = true;
    }
    if (u.acc_dirty) {
        clear_acc(m);
        if (u.acc_dirty) { set_last_error("ca_mirror_utilization: clearing the sums failed"); return CA_EDEVICE; }
    }

    // a page-locked `out` (ca_host_alloc) takes the rows straight from the kernel
    ca_util_info* dst = nullptr;
    if (out) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeHost &&
            attr.devicePointer != nullptr)
            dst = static_cast<ca_util_info*>(attr.devicePointer);
        else
            (void)hipGetLastError();
    }
    unsigned char* d = u.in.as<unsigned char>();
    CA_HIP_CHECK(hipMemcpyAsync(d, h, L.bytes, hipMemcpyHostToDevice, m->stream));
    u.h2d_bytes = (int64_t)L.bytes;
    CA_HIP_CHECK(hipEventRecord(m->ev0, m->stream));
    u.acc_dirty = true;
    if (n_pods > 0 && resident) {
        const casim::PodCols& c = *m->pcol;
        hipLaunchKernelGGL(k_mirror_pod_sums_resident, dim3((unsigned)((n_pods + kThreads - 1) / kThreads)), dim3(kThreads),
                           0, m->stream, c.d_node.as<const int32_t>(), c.d_has.as<const uint8_t>(),
                           c.d_row.as<const ca_util_pod>(), m->d_pods.spec.as<const ca_pod_spec>(), (int32_t)n_pods,
                           (int32_t)n_nodes, reinterpret_cast<const int32_t*>(d + L.ids),
                           reinterpret_cast<const ca_util_pod*>(d + L.rows), (int32_t)n_over,
                           a->skip_daemonset_pods ? 1 : 0, a->skip_mirror_pods ? 1 : 0, a->now_ns, u.acc.as<UtilSum>());
        UT_CHECK(hipGetLastError());
    } else if (n_pods > 0) {
        hipLaunchKernelGGL(k_mirror_pod_sums, dim3((unsigned)((n_pods + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                           m->stream, reinterpret_cast<const int32_t*>(d + L.pod_node),
                           m->d_pods.spec.as<const ca_pod_spec>(), (int32_t)n_pods, (int32_t)n_nodes,
                           n_over ? reinterpret_cast<const uint32_t*>(d + L.bits) : nullptr,
                           reinterpret_cast<const int32_t*>(d + L.ids), reinterpret_cast<const ca_util_pod*>(d + L.rows),
                           (int32_t)n_over, a->skip_daemonset_pods ? 1 : 0, a->skip_mirror_pods ? 1 : 0, a->now_ns,
                           u.acc.as<UtilSum>());
        UT_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_mirror_node_util, dim3((unsigned)((n_nodes + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       m->stream, reinterpret_cast<const ca_util_node*>(d + L.nodes), (int32_t)n_nodes,
                       u.acc.as<UtilSum>(), u.info.as<ca_util_info>(), u.drain.as<int32_t>(), dst);
    UT_CHECK(hipGetLastError());
    UT_CHECK(hipEventRecord(m->ev1, m->stream));
    if (out && !dst) {
        UT_CHECK(hipMemcpyAsync(out, u.info.ptr, sizeof(ca_util_info) * n_nodes, hipMemcpyDeviceToHost, m->stream));
    }
    if (out) u.d2h_bytes += (int64_t)(sizeof(ca_util_info) * n_nodes);
    if (out_drain) {
        UT_CHECK(hipMemcpyAsync(out_drain, u.drain.ptr, sizeof(int32_t) * n_nodes, hipMemcpyDeviceToHost, m->stream));
        u.d2h_bytes += (int64_t)(sizeof(int32_t) * n_nodes);
    }
    if (!finish) return CA_OK;
    UT_CHECK(hipStreamSynchronize(m->stream));
    u.acc_dirty = false;                                          // the node kernel cleared what the pods added
    if (kernel_ms) CA_HIP_CHECK(hipEventElapsedTime(kernel_ms, m->ev0, m->ev1));
    return CA_OK;
}

// byte offsets of the move-list kernels' buffers in PodCols::d_mv
struct MoveLayout {
    size_t n_tiles, cand_of, off, tile_cnt, tile_base, rank, table, lists, bytes;
    MoveLayout(size_t n_nodes, size_t table_pods) {
        n_tiles = std::max<size_t>(1, (table_pods + kTile - 1) / kTile);
        cand_of = 0;
        off = cand_of + al64(sizeof(int32_t) * n_nodes);
        tile_cnt = off + al64(sizeof(int32_t) * (n_nodes + 1));
        tile_base = tile_cnt + al64(sizeof(int32_t) * n_tiles);
        rank = tile_base + al64(sizeof(int32_t) * n_tiles);
        table = rank + al64(sizeof(int32_t) * n_tiles * kTile);
        lists = table + al64(sizeof(int32_t) * n_tiles * kTile);
        bytes = lists + al64(sizeof(int32_t) * (n_nodes + 1 + table_pods));
    }
};

// The move lists on the device, queued behind k_classify_compact: d_counts / d_cand / d_cls are
// its outputs, `in` the call's staged inputs (InLayout L, resident).
int queue_move_lists(ca_mirror* m, const ca_mirror_util_args* a, const InLayout& L, int32_t* d_counts,
                     const int32_t* d_cand, const uint8_t* d_cls) {
    UtilScratch& u = m->ut;
    casim::PodCols& c = *m->pcol;
    const size_t n = m->nodes.size(), n_pods = m->pods.size();
    const MoveLayout M(n, u.table_pods);
    int st = c.d_mv.reserve(M.bytes + 64);
    if (st != CA_OK) return st;
    unsigned char* d = c.d_mv.as<unsigned char>();
    const unsigned char* in = u.in.as<const unsigned char>();
    int32_t* cand_of = reinterpret_cast<int32_t*>(d + M.cand_of);
    int32_t* off = reinterpret_cast<int32_t*>(d + M.off);
    int32_t* tile_cnt = reinterpret_cast<int32_t*>(d + M.tile_cnt);
    int32_t* tile_base = reinterpret_cast<int32_t*>(d + M.tile_base);
    int32_t* rank = reinterpret_cast<int32_t*>(d + M.rank);
    int32_t* table = reinterpret_cast<int32_t*>(d + M.table);
    int32_t* lists = reinterpret_cast<int32_t*>(d + M.lists);
    const int32_t* node_pods = reinterpret_cast<const int32_t*>(in + L.pod_node);
    const unsigned nb = (unsigned)((n + kThreads - 1) / kThreads);
    CA_HIP_CHECK(hipMemsetAsync(table, 0xFF, sizeof(int32_t) * M.n_tiles * kTile, m->stream));
    hipLaunchKernelGGL(k_cand_map, dim3(nb), dim3(kThreads), 0, m->stream, d_cls, d_cand, d_counts, (int32_t)n, cand_of);
    hipLaunchKernelGGL(k_cand_offsets, dim3(1), dim3(kScanThreads), 0, m->stream, d_cand, node_pods, (int32_t)n,
                       (int32_t)u.table_pods, off, d_counts);
    if (n_pods > 0)
        hipLaunchKernelGGL(k_slot_table, dim3((unsigned)((n_pods + kThreads - 1) / kThreads)), dim3(kThreads), 0, m->stream,
                           c.d_node.as<const int32_t>(), c.d_slot.as<const int32_t>(), c.d_has.as<const uint8_t>(),
                           c.d_row.as<const ca_util_pod>(), m->d_pods.spec.as<const ca_pod_spec>(), (int32_t)n_pods,
                           (int32_t)n, reinterpret_cast<const int32_t*>(in + L.ids),
                           reinterpret_cast<const ca_util_pod*>(in + L.rows), a->n_pod_rows, cand_of, off, node_pods,
                           (int32_t)u.table_pods, table, d_counts);
    hipLaunchKernelGGL(k_tile_count, dim3((unsigned)M.n_tiles), dim3(kThreads), 0, m->stream, table, d_counts, tile_cnt);
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kScanThreads), 0, m->stream, tile_cnt, (int32_t)M.n_tiles, tile_base,
                       d_counts);
    hipLaunchKernelGGL(k_tile_write, dim3((unsigned)M.n_tiles), dim3(kThreads), 0, m->stream, table, d_counts, tile_base,
                       rank, lists);
    hipLaunchKernelGGL(k_move_off, dim3((unsigned)((n + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, m->stream, off,
                       d_counts, rank, (int32_t)n, lists);
    CA_HIP_CHECK(hipGetLastError());
    CA_HIP_CHECK(hipEventRecord(c.ev, m->stream));
    return CA_OK;
}

// The candidates' pods to move, in NodeInfo.Pods order, listed on the host from NodeRow.pods.
void host_move_lists(ca_mirror* m, const ca_mirror_util_args* a, ca_scale_down_candidates* h) {
    const auto t1 = std::chrono::steady_clock::now();
    const int32_t n_cand = (int32_t)h->cand.size();
    auto pods_of = [&](int32_t nd) -> const std::vector<int32_t>& { return m->nodes[nd].pods; };
    auto flags_of = [&](int32_t id) { return m->pods[(size_t)id].spec.flags; };
    // (a record read per pod misses the cache: large candidate sets go over the worker pool,
    // contiguous ranges of candidates, joined in order)
    const int32_t T = std::min<int32_t>(8, n_cand / 64);
    if (T > 1) {
        std::vector<std::vector<int32_t>> sub((size_t)T), off((size_t)T), mv((size_t)T);
        parallel_run(T, [&](int32_t w) {
            const size_t b = (size_t)n_cand * (size_t)w / (size_t)T, e = (size_t)n_cand * ((size_t)w + 1) / (size_t)T;
            sub[w].assign(h->cand.begin() + b, h->cand.begin() + e);
            build_move_lists(a, sub[w], pods_of, flags_of, off[w], mv[w]);
        });
        h->move_off.assign(1, 0);
        for (int32_t w = 0; w < T; w++) {
            const int32_t base = (int32_t)h->move_pods.size();
            for (size_t k = 1; k < off[w].size(); k++) h->move_off.push_back(base + off[w][k]);
            h->move_pods.insert(h->move_pods.end(), mv[w].begin(), mv[w].end());
        }
    } else {
        build_move_lists(a, h->cand, pods_of, flags_of, h->move_off, h->move_pods);
    }
    h->t[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count();
}

// The lists queue_move_lists' kernels built, [move_off (n_cand + 1) | move_pods], in one copy.
int fetch_move_lists(ca_mirror* m, ca_scale_down_candidates* h, int32_t n_moves) {
    UtilScratch& u = m->ut;
    casim::PodCols& pc = *m->pcol;
    const size_t n_cand = h->cand.size(), ints = n_cand + 1 + (size_t)n_moves;
    const MoveLayout M(m->nodes.size(), u.table_pods);
    int st = pc.h_mv.reserve(sizeof(int32_t) * ints);
    if (st != CA_OK) return st;
    if (hipMemcpyAsync(pc.h_mv.ptr, pc.d_mv.as<unsigned char>() + M.lists, sizeof(int32_t) * ints, hipMemcpyDeviceToHost,
                       m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess) {
        set_last_error("ca_scale_down_candidates_create_resident: fetching the move lists failed");
        return CA_EDEVICE;
    }
    u.d2h_bytes += (int64_t)(sizeof(int32_t) * ints);
    const int32_t* mv = pc.h_mv.as<const int32_t>();
    h->move_off.assign(mv, mv + n_cand + 1);
    h->move_pods.assign(mv + n_cand + 1, mv + ints);
    (void)hipEventElapsedTime(&h->t[3], m->ev2, pc.ev);          // device time of the move-list kernels
    return CA_OK;
}

int candidates_create(ca_mirror* m, const ca_mirror_util_args* a, double threshold, double gpu_threshold,
                      const uint8_t* eligible, ca_scale_down_candidates** out, bool resident) {
    if (!out) return CA_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    int st = util_run(m, a, nullptr, nullptr, nullptr, eligible, false, resident);
    if (st != CA_OK) return st;
    UtilScratch& u = m->ut;
    const size_t n = m->nodes.size();
    auto* h = new ca_scale_down_candidates();
    h->m = m;
    h->order_epoch = m->order_epoch;
    h->n_nodes = (int32_t)n;
    h->cand_of.assign(n, -1);
    h->move_off.assign(1, 0);
    if (n > 0) {
        auto fail = [&](int rc) { clear_acc(m); delete h; return rc; };
        // [counts (16 ints) | empty n | cand n | status n | class n bytes], then the info rows on the host side
        const size_t ints = 16 + 3 * n, cls_bytes = al64(sizeof(int32_t) * ints + n);
        if ((st = u.cls.reserve(cls_bytes)) != CA_OK ||
            (st = u.h_cls.reserve(cls_bytes + sizeof(ca_util_info) * n)) != CA_OK)
            return fail(st);
        int32_t* d = u.cls.as<int32_t>();
        const InLayout L(n, m->pods.size(), (size_t)a->n_pod_rows, eligible != nullptr, resident);
        hipLaunchKernelGGL(k_classify_compact, dim3(1), dim3(kScanThreads), 0, m->stream, u.info.as<const ca_util_info>(),
                           u.drain.as<const int32_t>(),
                           eligible ? u.in.as<const uint8_t>() + L.eligible : nullptr, (int32_t)n, threshold,
                           gpu_threshold, reinterpret_cast<uint8_t*>(d + ints), d + 16, d + 16 + n, d + 16 + 2 * n, d);
        unsigned char* hc = u.h_cls.as<unsigned char>();
        if (hipGetLastError() != hipSuccess || hipEventRecord(m->ev2, m->stream) != hipSuccess) {
            set_last_error("ca_scale_down_candidates_create: classification failed");
            return fail(CA_EDEVICE);
        }
        // (its own status: a failed reserve is not a device failure; its HIP errors name themselves)
        if (resident && (st = queue_move_lists(m, a, L, d, d + 16 + n, reinterpret_cast<const uint8_t*>(d + ints))) != CA_OK)
            return fail(st);
        if (hipMemcpyAsync(hc, d, cls_bytes, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
            hipMemcpyAsync(hc + cls_bytes, u.info.ptr, sizeof(ca_util_info) * n, hipMemcpyDeviceToHost, m->stream) !=
                hipSuccess ||
            hipStreamSynchronize(m->stream) != hipSuccess) {
            set_last_error(resident ? "ca_scale_down_candidates_create_resident: fetching the classes failed"
                                    : "ca_scale_down_candidates_create: classification failed");
            return fail(CA_EDEVICE);
        }
        u.acc_dirty = false;
        u.d2h_bytes += (int64_t)(cls_bytes + sizeof(ca_util_info) * n);
        (void)hipEventElapsedTime(&h->t[0], m->ev0, m->ev1);
        (void)hipEventElapsedTime(&h->t[1], m->ev1, m->ev2);
        const int32_t* hi = reinterpret_cast<const int32_t*>(hc);
        const int32_t n_empty = hi[CN_EMPTY], n_cand = hi[CN_CAND];
        if (resident && hi[CN_BAD]) {
            // a slot outside its node's list, or counts that do not add up: nothing was written there
            set_last_error("ca_scale_down_candidates_create_resident: pod columns out of sync");
            delete h;
            return CA_EDEVICE;
        }
        h->empty.assign(hi + 16, hi + 16 + n_empty);
        h->cand.assign(hi + 16 + n, hi + 16 + n + n_cand);
        h->status.assign(hi + 16 + 2 * n, hi + 16 + 2 * n + n_cand);
        h->cls.assign(hc + sizeof(int32_t) * ints, hc + sizeof(int32_t) * ints + n);
        h->info.resize(n);
        std::memcpy(h->info.data(), hc + cls_bytes, sizeof(ca_util_info) * n);
        for (int32_t c = 0; c < n_cand; c++) h->cand_of[h->cand[c]] = c;
        if (resident) {
            if ((st = fetch_move_lists(m, h, hi[CN_MOVES])) != CA_OK) { delete h; return st; }
        } else {
            host_move_lists(m, a, h);
        }
    }
    h->t[2] = u.stage_ms;
    h->t[5] = (float)u.h2d_bytes;
    h->t[6] = (float)u.d2h_bytes;
    h->t[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = h;
    return CA_OK;
}

}  // namespace

extern "C" {

int ca_mirror_utilization(ca_mirror* m, const ca_mirror_util_args* a, ca_util_info* out, int32_t* out_drain,
                          float* kernel_ms) {
    return util_run(m, a, out, out_drain, kernel_ms, nullptr, true);
}

int ca_mirror_utilization_resident(ca_mirror* m, const ca_mirror_util_args* a, ca_util_info* out, int32_t* out_drain,
                                   float* kernel_ms) {
    return util_run(m, a, out, out_drain, kernel_ms, nullptr, true, true);
}

int ca_scale_down_candidates_create(ca_mirror* m, const ca_mirror_util_args* a, double threshold,
                                    double gpu_threshold, const uint8_t* eligible, ca_scale_down_candidates** out) {
    return candidates_create(m, a, threshold, gpu_threshold, eligible, out, false);
}

int ca_scale_down_candidates_create_resident(ca_mirror* m, const ca_mirror_util_args* a, double threshold,
                                             double gpu_threshold, const uint8_t* eligible,
                                             ca_scale_down_candidates** out) {
    return candidates_create(m, a, threshold, gpu_threshold, eligible, out, true);
}

int ca_scale_down_candidates_info(const ca_scale_down_candidates* h, int32_t* n_nodes, int32_t* n_empty,
                                  int32_t* n_cand, int32_t* n_moves) {
    if (!h) return CA_EINVAL;
    if (n_nodes) *n_nodes = h->n_nodes;
    if (n_empty) *n_empty = (int32_t)h->empty.size();
    if (n_cand) *n_cand = (int32_t)h->cand.size();
    if (n_moves) *n_moves = (int32_t)h->move_pods.size();
    return CA_OK;
}

int ca_scale_down_candidates_fetch(const ca_scale_down_candidates* h, ca_util_info* info, uint8_t* node_class,
                                   int32_t* empty, int32_t* cand, int32_t* cand_status, int32_t* move_off,
                                   int32_t* move_pods) {
    if (!h) return CA_EINVAL;
    auto put = [](auto* dst, const auto& v) {
        if (dst && !v.empty()) std::memcpy(dst, v.data(), sizeof(v[0]) * v.size());
    };
    put(info, h->info);
    put(node_class, h->cls);
    put(empty, h->empty);
    put(cand, h->cand);
    put(cand_status, h->status);
    put(move_off, h->move_off);
    put(move_pods, h->move_pods);
    return CA_OK;
}

int ca_scale_down_candidates_timings(const ca_scale_down_candidates* h, float* out, int32_t cap) {
    if (!h || !out || cap < 0) return CA_EINVAL;
    const int32_t n = std::min<int32_t>(cap, 7);
    for (int32_t i = 0; i < n; i++) out[i] = h->t[i];
    return 7;
}

int ca_scale_down_candidates_destroy(ca_scale_down_candidates* h) {
    if (!h) return CA_EINVAL;
    delete h;
    return CA_OK;
}

int ca_removal_plan_create_candidates(const ca_scale_down_candidates* h, const int32_t* nodes, int32_t n,
                                      const uint8_t* dest_mask, ca_removal_plan** out) {
    if (!h || !out || (nodes && n < 0)) return CA_EINVAL;
    if (h->order_epoch != h->m->order_epoch) return CA_ESTATE;   // created before a ca_mirror_reorder_nodes
    if (!nodes)                                                  // every candidate, in position order
        return ca_removal_plan_create(h->m, h->cand.data(), (int32_t)h->cand.size(), dest_mask, h->status.data(),
                                      h->move_off.data(), h->move_pods.data(), out);
    std::vector<int32_t> status, off, moves;
    if (select_candidates(nodes, n, h->cand_of, h->status, h->move_off, h->move_pods, status, off, moves) != CA_OK)
        return CA_EINVAL;
    return ca_removal_plan_create(h->m, nodes, n, dest_mask, status.data(), off.data(), moves.data(), out);
}

}  // extern "C"
