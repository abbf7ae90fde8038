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

inline size_t al64(size_t b) { return (b + 63) & ~(size_t)63; }

// byte offsets of one call's inputs in UtilScratch::in / h_in
struct InLayout {
    size_t pod_node, nodes, ids, rows, bits, eligible, bytes;
    InLayout(size_t n_nodes, size_t n_pods, size_t n_over, bool elig) {
        pod_node = 0;
        nodes = al64(sizeof(int32_t) * n_pods);
        ids = nodes + al64(sizeof(ca_util_node) * n_nodes);
        rows = ids + al64(sizeof(int32_t) * n_over);
        bits = rows + al64(sizeof(ca_util_pod) * n_over);
        eligible = bits + (n_over ? al64(sizeof(uint32_t) * ((n_pods + 31) / 32)) : 0);
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
// behind them, syncs, and clears acc_dirty.
int util_run(ca_mirror* m, const ca_mirror_util_args* a, ca_util_info* out, int32_t* out_drain, float* kernel_ms,
             const uint8_t* eligible, bool finish) {
    int st = check_args(m, a);
    if (st != CA_OK) return st;
    UtilScratch& u = m->ut;
    const size_t n_nodes = m->nodes.size(), n_pods = m->pods.size(), n_over = (size_t)a->n_pod_rows;
    if (kernel_ms) *kernel_ms = 0.0f;
    u.stage_ms = 0;
    u.h2d_bytes = u.d2h_bytes = 0;
    u.n_nodes = (int32_t)n_nodes;
    if (n_nodes == 0) return CA_OK;
    CA_HIP_CHECK(hipSetDevice(m->device));
    const InLayout L(n_nodes, n_pods, n_over, eligible != nullptr);
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
    // the pod -> node column (PodRow.node lives in the chunked host records)
    const auto t0 = std::chrono::steady_clock::now();
    int32_t* hp = reinterpret_cast<int32_t*>(h + L.pod_node);
    const int32_t T = (int32_t)std::min<size_t>(8, n_pods >> 16);
    if (T > 1) {
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
        uint32_t* bits = reinterpret_cast<uint32_t*>(h + L.bits);
        std::memset(bits, 0, sizeof(uint32_t) * ((n_pods + 31) / 32));
        for (size_t k = 0; k < n_over; k++) bits[a->pod_ids[k] >> 5] |= 1u << (a->pod_ids[k] & 31);
    }
    if (eligible) std::memcpy(h + L.eligible, eligible, n_nodes);

    if ((st = m->sync_pods()) != CA_OK) return st;
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
    if (n_pods > 0) {
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

}  // namespace

extern "C" {

int ca_mirror_utilization(ca_mirror* m, const ca_mirror_util_args* a, ca_util_info* out, int32_t* out_drain,
                          float* kernel_ms) {
    return util_run(m, a, out, out_drain, kernel_ms, nullptr, true);
}

int ca_scale_down_candidates_create(ca_mirror* m, const ca_mirror_util_args* a, double threshold,
                                    double gpu_threshold, const uint8_t* eligible, ca_scale_down_candidates** out) {
    if (!out) return CA_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    int st = util_run(m, a, nullptr, nullptr, nullptr, eligible, false);
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
        const InLayout L(n, m->pods.size(), (size_t)a->n_pod_rows, eligible != nullptr);
        hipLaunchKernelGGL(k_classify_compact, dim3(1), dim3(kScanThreads), 0, m->stream, u.info.as<const ca_util_info>(),
                           u.drain.as<const int32_t>(),
                           eligible ? u.in.as<const uint8_t>() + L.eligible : nullptr, (int32_t)n, threshold,
                           gpu_threshold, reinterpret_cast<uint8_t*>(d + ints), d + 16, d + 16 + n, d + 16 + 2 * n, d);
        unsigned char* hc = u.h_cls.as<unsigned char>();
        if (hipGetLastError() != hipSuccess || hipEventRecord(m->ev2, m->stream) != hipSuccess ||
            hipMemcpyAsync(hc, d, cls_bytes, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
            hipMemcpyAsync(hc + cls_bytes, u.info.ptr, sizeof(ca_util_info) * n, hipMemcpyDeviceToHost, m->stream) !=
                hipSuccess ||
            hipStreamSynchronize(m->stream) != hipSuccess) {
            set_last_error("ca_scale_down_candidates_create: classification failed");
            return fail(CA_EDEVICE);
        }
        u.acc_dirty = false;
        u.d2h_bytes += (int64_t)(cls_bytes + sizeof(ca_util_info) * n);
        (void)hipEventElapsedTime(&h->t[0], m->ev0, m->ev1);
        (void)hipEventElapsedTime(&h->t[1], m->ev1, m->ev2);
        const int32_t* hi = reinterpret_cast<const int32_t*>(hc);
        const int32_t n_empty = hi[0], n_cand = hi[1];
        h->empty.assign(hi + 16, hi + 16 + n_empty);
        h->cand.assign(hi + 16 + n, hi + 16 + n + n_cand);
        h->status.assign(hi + 16 + 2 * n, hi + 16 + 2 * n + n_cand);
        h->cls.assign(hc + sizeof(int32_t) * ints, hc + sizeof(int32_t) * ints + n);
        h->info.resize(n);
        std::memcpy(h->info.data(), hc + cls_bytes, sizeof(ca_util_info) * n);
        // the candidates' pods to move, in NodeInfo.Pods order
        const auto t1 = std::chrono::steady_clock::now();
        for (int32_t c = 0; c < n_cand; c++) h->cand_of[h->cand[c]] = c;
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
    h->t[2] = u.stage_ms;
    h->t[5] = (float)u.h2d_bytes;
    h->t[6] = (float)u.d2h_bytes;
    h->t[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = h;
    return CA_OK;
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
