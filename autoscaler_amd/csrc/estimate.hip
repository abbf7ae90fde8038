// estimate.hip — BinpackingNodeEstimator.Estimate for a batch of node groups.
//
// Reference: CA/estimator/binpacking_estimator.go:65-193,
//            CA/estimator/threshold_based_limiter.go:27-64,
//            CA/utils/scheduler/scheduler.go:73-91 (template copies),
//            CA/simulator/predicatechecker/schedulerbased.go:90-136 (rotating scan).
//
// Pipeline of one headline step (C2: uniform score classes, no cross-class float64 ties —
// the decoupled Go order):
//   st3 (high priority)  k_pdq_sort      Go 1.19 sort.Slice's exact permutation (class ranks
//                                        folded in), one 1024-thread workgroup per sort
//                                        class — the groups with equal pod lists and equal
//                                        class ranks on their templates (sort_classes) —
//                                        run for the class's first group; writes the
//                                        Go-order pod ids and that group's epoch-stamped
//                                        ready flag, which the other members' consumers read.
//   (plan creation)      k_cls_hist      per-class counts of each group's list, once: the
//                                        lists never change after creation.
//   st  (heavy groups)   k_run_table     class ranks, the plan's counts by rank, each rank's
//                                        first stream position, the class's stream record
//                                        against the template, its requests and their
//                                        reciprocals in float64.
//                        k_ffd_chain     one 4-wave workgroup per group: the sequential
//                                        First-Fit-Decreasing loop (per pod, or per run of
//                                        identical pods in closed form) with the new-node
//                                        rows in LDS, walking the group's run table (copied
//                                        to LDS in its prologue); pushes 16384-output tickets.
//                                        (CASIM_TABLE_CHAIN=0, or a table too large for LDS:
//                                        k_emit_runs writes run heads and stream windows
//                                        first and the chain reads those.)  Rows in LDS, no
//                                        ports / extended resources / node ordinals, groups
//                                        <= 2^20 pods, quantities < 2^53: the lean
//                                        instantiation (CASIM_LEAN_CHAIN=0: the generic one).
//   st2 (light groups)   the same kernels for the groups outside the heavy set.
//   pub_stream           k_publish       claims tickets in completion order and writes the
//                                        scheduled pods (Go-order ids) into the caller's
//                                        page-locked buffer while the chains run; a ticket
//                                        waits for the sort parts its positions lie in.
//   host                 lastIndex fix-up: groups whose result depends on their lastIndex
//                        input are re-run until every input equals its predecessor's
//                        output (exact); the host joins the streams.
// Other paths: non-uniform podsets (C4) sort in Go order first (k_class_rank, k_pdq_sort,
// radix passes, k_emit_bucket) and then chain; > 4096 score classes use k_score_tiles +
// k_merge_runs + k_emit_stream; device-resident results expand the chains' segments with
// k_copy_segments; a publisher that gives up falls back to the same copy + D2H.
#include "mirror.h"
#include "device_filters.h"
#include "pdqsort.h"
#include "sort_reuse_host.h"
#include "chain_owner_host.h"

#include <cstring>
#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <tuple>
#include <chrono>
#include <mutex>
#include <thread>
#include <cstdlib>

namespace casim {

// per (group, pod) static bits computed against the template (k_score_tiles)
enum : uint32_t {
    SF_EVAL    = 0x1u,   // FitsAnyNode visits new nodes with filters (counts evals)
    SF_FA_OK   = 0x2u,   // static filters pass on the template (FitsAnyNode path)
    SF_CP_EVAL = 0x4u,   // CheckPredicates runs filters (PreFilter ok)
    SF_CP_OK   = 0x8u,   // static filters incl. NodeUnschedulable pass (CheckPredicates path)
    SF_ZERO    = 0x10u,  // PF_ALL_ZERO
    SF_SCALAR  = 0x20u,  // PF_SCALAR_REQ
    SF_PORTS   = 0x40u,  // PF_PORTS
    SF_UNSUP   = 0x80u,  // PF_HOSTNAME_DEP / PF_OUT_OF_SCOPE: group unsupported (casim.h scope)
};

struct alignas(16) SortItem {
    uint64_t key;     // ~ordered(score): ascending key == descending score
    uint32_t pos;     // position in the group's pod list (tie-break, stable)
    uint32_t flags;   // SF_*
};
static_assert(sizeof(SortItem) == 16, "SortItem");

struct alignas(16) StreamPod {
    int64_t cpu, mem, eph;
    int32_t pod;      // pod set index
    uint32_t flags;   // SF_* | SF_HEAD | SF_BATCH
};
static_assert(sizeof(StreamPod) == 32, "StreamPod");

// stream-only bits (k_emit_stream)
enum : uint32_t {
    SF_HEAD  = 0x100u,   // first pod of a run of identical consecutive pods
    SF_BATCH = 0x200u,   // run-batchable: resource-only (no ports / scalars), requests >= 0
};

struct alignas(16) GroupMeta {
    int64_t tcpu, tmem, teph;      // template free (alloc - template pods)
    int32_t tpods;                 // template free pod slots
    int32_t off;                   // offset into the pod lists / streams
    int32_t count;                 // pods in the group
    int32_t tmpl;                  // template index
    uint32_t tflags;               // NF_* of the template
    int32_t moff;                  // offset of the group's 64-pod head masks
    int32_t ids_off;               // decoupled Go order: offset of the group's ids in d_spod_go — its own `off`,
                                   // or that of the group whose sort it shares (sort_classes)
    int32_t hoff;                  // offset of the group's radix histograms [256][rtiles]
    int32_t rtiles;                // radix tiles of the group (bucket sort)
    int32_t ids_grp;               // ... and the group whose ready flag covers those ids (itself, or that group)
};
static_assert(sizeof(GroupMeta) == 64, "GroupMeta");
// Group handled by a block: the launch's group map (a subset of the batch, e.g. the
// heavy groups launched first) or the block index itself.
#define GSEL(b) (gmap ? gmap[(b)] : (int)(b))

struct alignas(16) ChainOut {
    int32_t node_count, n_sched, nodes_added, lin;
    int32_t lout, status, sensitive, had_success;
    uint64_t evals;
    uint64_t pad;        // diagnostics (ca_estimate_plan_group_ticks)
    int32_t nseg;        // run-placement segments written to the group's segment list
    int32_t pad2[3];
};
static_assert(sizeof(ChainOut) == 64, "ChainOut");

// A run placement: stream positions [src, src+len) were scheduled as outputs
// [dst, dst+len) of the group (k_copy_segments fills sched_pod from them).
struct alignas(16) Seg {
    int32_t dst, src, len, pad;
};

constexpr int TILE = 1024;

__device__ inline uint64_t ordered_bits(double d) {
    if (d == 0.0) d = 0.0;   // -0 == +0 for the comparator (binpacking_estimator.go:74)
    uint64_t u = (uint64_t)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ inline bool item_less(const SortItem& a, const SortItem& b) {
    return a.key < b.key || (a.key == b.key && a.pos < b.pos);
}

// SF_* bits of a pod against a group's template: the template-only part of the
// filter chain (schedulerbased.go:107-129 PreFilter / Unschedulable skip, framework.go
// order via dev_static_filters), evaluated once per (group, pod).  The full pod record
// is read only when a static filter can matter.
__device__ inline uint32_t static_sf(const PodHot& p, const ca_template& tp, bool tunsched,
                                     const ca_pod_spec* __restrict__ specs, const ca_selector_term* __restrict__ terms,
                                     const ca_selector_req* __restrict__ reqs) {
    uint32_t sf = 0;
    const bool pre_fail = (p.flags & PF_PREFILTER_FAIL) != 0;
    bool static_ok = true;
    if ((p.flags & (PF_NODE_NAME | PF_AFFINITY)) || (tp.node.taints && !(p.flags & PF_TAINT_MASK_ALL))) {
        const ca_pod_spec& s = specs[p.spec];
        if ((p.flags & (PF_NODE_NAME | PF_AFFINITY)) || (tp.node.taints & ~s.tolerated_taints)) {
            NodeStatic ns;
            ns.taints = tp.node.taints;
            for (int w = 0; w < CA_LABEL_WORDS; w++) ns.labels[w] = tp.node.label_pairs[w];
            ns.keys = tp.node.label_keys;
            for (int k = 0; k < CA_MAX_INT_KEYS; k++) ns.ints[k] = tp.node.int_label[k];
            ns.int_valid = tp.node.int_label_valid;
            ns.name_id = tp.node.name_id;
            static_ok = dev_static_filters(s, p.flags, terms, reqs, ns, false) == CA_PLUGIN_NONE;
        }
    }
    if (!pre_fail && !tunsched) sf |= SF_EVAL;                           // schedulerbased.go:125
    if ((sf & SF_EVAL) && static_ok) sf |= SF_FA_OK;
    if (!pre_fail) sf |= SF_CP_EVAL;
    if (!pre_fail && (!tunsched || (p.flags & PF_TOL_UNSCHED)) && static_ok) sf |= SF_CP_OK;
    if (p.flags & PF_ALL_ZERO) sf |= SF_ZERO;
    if (p.flags & PF_SCALAR_REQ) sf |= SF_SCALAR;
    if (p.flags & PF_PORTS) sf |= SF_PORTS;
    if (p.flags & (PF_HOSTNAME_DEP | PF_OUT_OF_SCOPE)) sf |= SF_UNSUP;
    return sf;
}

// the score class of every (group, pod) item, gathered from the podset's class column
__global__ void __launch_bounds__(256) k_item_cls(const int32_t* __restrict__ pod_idx, const int32_t* __restrict__ cls,
                                                 int32_t* __restrict__ out, int32_t n) {
    for (int32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = cls[pod_idx[i]];
}

// The lists from the option matrix (ca_estimate_plan_create_options; DESIGN.md §4 "lists
// from the option matrix").  Group g's list is the concatenation, for e ascending with
// ok[g][e] != 0, of equivalence group e's pods eg_pod[eg_off[e] .. eg_off[e+1])
// (ComputeExpansionOption's append, orchestrator.go:468-482).  No [G][n_eg] table of list
// offsets is kept (with one pod per equivalence group it would be as large as the lists):
// k_option_chunks leaves, per row, the list offset at which every chunk of OPT_CHUNK
// equivalence groups starts, and k_option_lists redoes the scan inside a chunk in LDS.
constexpr int OPT_TILE = 2048;     // output positions of one group per workgroup (abi.OPTION_LIST_TILE)
constexpr int OPT_CHUNK = 256;     // equivalence groups per partial sum (abi.OPTION_LIST_CHUNK)

// inclusive scan of one value per thread over a 256-thread block (wsum: 4 words of LDS; the
// caller's next barrier separates two scans)
__device__ inline int32_t block_scan_256(int32_t v, int32_t* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    for (int q = 0; q < w; q++) x += wsum[q];
    return x;
}

// one workgroup per row: chunk_pre[g][k] = list offset of the first pod of chunk k
__global__ void __launch_bounds__(256) k_option_chunks(const int32_t* __restrict__ eg_off, const uint8_t* __restrict__ ok,
                                                      int32_t n_eg, int32_t nch, int32_t* __restrict__ chunk_pre) {
    __shared__ int32_t wsum[4];
    const uint8_t* row = ok + (size_t)blockIdx.x * (size_t)n_eg;
    int32_t* pre = chunk_pre + (size_t)blockIdx.x * (size_t)nch;
    int32_t running = 0;
    for (int32_t k = 0; k < nch; k++) {
        const int32_t e = k * OPT_CHUNK + (int32_t)threadIdx.x;
        const int32_t len = (e < n_eg && row[e]) ? eg_off[e + 1] - eg_off[e] : 0;
        (void)block_scan_256(len, wsum);
        if (threadIdx.x == 0) pre[k] = running;
        running += wsum[0] + wsum[1] + wsum[2] + wsum[3];      // the chunk's total
        __syncthreads();
    }
}

// One workgroup per OPT_TILE output positions of one group (as k_copy_segments): a binary
// search of the row's chunk offsets for the chunk holding the first position, then chunk
// after chunk: the passing groups' lengths are scanned in LDS, and every output position
// finds its equivalence group there (8 LDS probes) — consecutive threads write consecutive
// positions, and read consecutive eg_pod entries inside a segment.  The score class is
// gathered beside the pod id (item_cls != NULL: the bucket path).
__global__ void __launch_bounds__(256) k_option_lists(const GroupMeta* __restrict__ groups,
                                                     const int32_t* __restrict__ eg_off, const int32_t* __restrict__ eg_pod,
                                                     const uint8_t* __restrict__ ok, int32_t n_eg, int32_t nch,
                                                     const int32_t* __restrict__ chunk_pre, const int32_t* __restrict__ cls,
                                                     int32_t* __restrict__ pod_idx, int32_t* __restrict__ item_cls) {
    __shared__ int32_t s_end[OPT_CHUNK], s_delta[OPT_CHUNK], wsum[4];
    const GroupMeta gm = groups[blockIdx.y];
    const int32_t base = (int32_t)blockIdx.x * OPT_TILE;
    if (base >= gm.count) return;
    const int32_t end = min(base + OPT_TILE, gm.count);
    const uint8_t* row = ok + (size_t)blockIdx.y * (size_t)n_eg;
    const int32_t* pre = chunk_pre + (size_t)blockIdx.y * (size_t)nch;
    int32_t k0 = 0, hi = nch;                      // last chunk starting at or before base
    while (hi - k0 > 1) {
        const int32_t mid = (k0 + hi) >> 1;
        if (pre[mid] <= base) k0 = mid; else hi = mid;
    }
    int32_t* dst = pod_idx + gm.off;
    int32_t* dcl = item_cls ? item_cls + gm.off : nullptr;
    for (int32_t k = k0; k < nch; k++) {
        const int32_t cstart = pre[k];
        if (cstart >= end) break;
        const int32_t e = k * OPT_CHUNK + (int32_t)threadIdx.x;
        int32_t src = 0, len = 0;
        if (e < n_eg && row[e]) { src = eg_off[e]; len = eg_off[e + 1] - src; }
        const int32_t x = block_scan_256(len, wsum);
        s_end[threadIdx.x] = cstart + x;                       // list offset after group e
        s_delta[threadIdx.x] = src - (cstart + x - len);       // eg_pod index of list position i: delta + i
        __syncthreads();
        const int32_t a = max(base, cstart), b = min(end, s_end[OPT_CHUNK - 1]);
        for (int32_t i = a + (int32_t)threadIdx.x; i < b; i += 256) {
            int32_t lo = 0, up = OPT_CHUNK - 1;                // first group ending after i (i < s_end[last])
            while (lo < up) {
                const int32_t mid = (lo + up) >> 1;
                if (s_end[mid] > i) up = mid; else lo = mid + 1;
            }
            const int32_t pod = eg_pod[s_delta[lo] + i];
            dst[i] = pod;
            if (dcl) dcl[i] = cls[pod];
        }
        __syncthreads();
    }
}

// 1. score + static predicates + tile sort ----------------------------------
__global__ void __launch_bounds__(256) k_score_tiles(
    const GroupMeta* __restrict__ groups, const int32_t* __restrict__ pod_idx, const ca_template* __restrict__ tmpls,
    const PodHot* __restrict__ ph, const ca_pod_spec* __restrict__ specs, const ca_selector_term* __restrict__ terms,
    const ca_selector_req* __restrict__ reqs, SortItem* __restrict__ out, uint32_t* __restrict__ group_unsup) {
    __shared__ SortItem tile[TILE];
    const GroupMeta gm = groups[blockIdx.y];
    const int32_t base = (int32_t)blockIdx.x * TILE;
    if (base >= gm.count) return;
    const int32_t n = min(TILE, gm.count - base);
    const ca_template& tp = tmpls[gm.tmpl];
    const int64_t acpu = tp.node.alloc_milli_cpu, amem = tp.node.alloc_memory;
    const bool tunsched = (tp.node.flags & CA_NODE_UNSCHEDULABLE) != 0;
    uint32_t unsup = 0;
    for (int t = threadIdx.x; t < TILE; t += blockDim.x) {
        SortItem it;
        if (t < n) {
            const int32_t pos = base + t;
            const int32_t pidx = pod_idx[gm.off + pos];
            const PodHot p = ph[pidx];
            const ca_pod_spec& s = specs[p.spec];
            // calculatePodScore (binpacking_estimator.go:164-193): containers-only sums
            double score = 0.0;
            if (acpu > 0) score += (double)s.score_milli_cpu / (double)acpu;
            if (amem > 0) score += (double)s.score_memory / (double)amem;
            const uint32_t sf = static_sf(p, tp, tunsched, specs, terms, reqs);
            if (sf & SF_UNSUP) unsup = 1;
            it.key = ~ordered_bits(score);
            it.pos = (uint32_t)pos;
            it.flags = sf;
        } else {
            it.key = ~0ull;
            it.pos = 0xFFFFFFFFu;
            it.flags = 0;
        }
        tile[t] = it;
    }
    if (unsup) atomicOr(&group_unsup[blockIdx.y], 1u);
    __syncthreads();
    // bitonic sort of TILE items, ascending (key, pos)
    for (int k = 2; k <= TILE; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < TILE; t += blockDim.x) {
                const int ixj = t ^ j;
                if (ixj > t) {
                    const SortItem a = tile[t], b = tile[ixj];
                    const bool up = (t & k) == 0;
                    if (up ? item_less(b, a) : item_less(a, b)) { tile[t] = b; tile[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < n; t += blockDim.x) out[gm.off + base + t] = tile[t];
}

// 2. merge pass: runs of `width` -> runs of 2*width --------------------------
__global__ void __launch_bounds__(256) k_merge_runs(const GroupMeta* __restrict__ groups, const SortItem* __restrict__ src,
                                                   SortItem* __restrict__ dst, int32_t width) {
    const GroupMeta gm = groups[blockIdx.y];
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= gm.count) return;
    const SortItem* g = src + gm.off;
    const SortItem me = g[i];
    const int32_t run = i / width;
    const int32_t pair = run ^ 1;
    const int32_t pstart = pair * width;
    int32_t rank = 0;
    if (pstart < gm.count) {
        const int32_t pend = min(pstart + width, gm.count);
        int32_t lo = pstart, hi = pend;             // count partner items < me
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (item_less(g[mid], me)) lo = mid + 1; else hi = mid;
        }
        rank = lo - pstart;
    }
    const int32_t start = min(run, pair) * width;
    dst[gm.off + start + (i - run * width) + rank] = me;
}

// 3. gather the stream + run heads -------------------------------------------
// A run is a maximal sequence of consecutive sorted pods that behave identically on
// every new node: equal requests and equal SF_* bits, resource-only.  heads[] holds
// one 64-bit mask per 64 stream positions (bit set = a run starts there; positions
// past the group end are heads).
__device__ inline bool batchable(const PodHot& p, uint32_t sf) {
    return !(sf & (SF_PORTS | SF_SCALAR | SF_UNSUP)) && p.cpu >= 0 && p.mem >= 0 && p.eph >= 0;
}

__global__ void __launch_bounds__(256) k_emit_stream(const GroupMeta* __restrict__ groups, const SortItem* __restrict__ src,
                                                    const int32_t* __restrict__ pod_idx, const PodHot* __restrict__ ph,
                                                    StreamPod* __restrict__ out, int32_t* __restrict__ spod,
                                                    uint64_t* __restrict__ heads) {
    const GroupMeta gm = groups[blockIdx.y];
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    bool head = true;
    if (i < gm.count) {
        const SortItem it = src[gm.off + i];
        const int32_t pidx = pod_idx[gm.off + (int32_t)it.pos];
        const PodHot p = ph[pidx];
        const bool bat = batchable(p, it.flags);
        if (i > 0 && bat) {
            const SortItem pv = src[gm.off + i - 1];
            const PodHot q = ph[pod_idx[gm.off + (int32_t)pv.pos]];
            head = !(pv.flags == it.flags && q.cpu == p.cpu && q.mem == p.mem && q.eph == p.eph);
        }
        StreamPod sp;
        sp.cpu = p.cpu; sp.mem = p.mem; sp.eph = p.eph;
        sp.pod = pidx;
        sp.flags = it.flags | (head ? SF_HEAD : 0u) | (bat ? SF_BATCH : 0u);
        out[gm.off + i] = sp;
        spod[gm.off + i] = pidx;
    }
    const uint64_t hb = __ballot(head);
    if ((threadIdx.x & 63) == 0 && i < gm.count) heads[gm.moff + (i >> 6)] = hb;
}

// 1'-3'. bucket sort over score classes ----------------------------------------
// The sort key (score desc, list position asc) depends on a pod only through its
// score class (ca_podset: equal score_milli_cpu and score_memory) and its position.  So
// when the pod set has at most CLS_MAX classes, each group ranks its classes by score
// (k_class_rank: dense rank, equal scores share a rank = the tie-by-position rule H2),
// and its pod list — already in position order — is stably sorted by that rank with
// 8-bit LSD counting passes (k_radix_hist / k_radix_scan / k_radix_scatter; ranks of
// equal digits inside a wave by ballot multisplit).  k_emit_bucket then builds the
// stream exactly as k_emit_stream does from the comparison sort.  Same output as
// k_score_tiles + k_merge_runs + k_emit_stream, ~8 B of HBM per item and pass instead
// of ~300.
constexpr int CLS_MAX = 4096;
constexpr int RT = 2048;               // items per radix tile
constexpr int RTHREADS = 256;
constexpr int RPT = RT / RTHREADS;     // items per thread
constexpr int RCH = RT / 64 / (RTHREADS / 64);   // 64-item chunks per wave

// Dense ranks of the U score classes against a group's template, by one 1024-thread
// workgroup: float64 score of every class, bitonic sort of the classes in LDS, dense rank
// (equal scores share a rank).  On return sc[i] is the rank of class idx[i], i < U.
// block_class_rank for NP <= 64 by one wavefront, the class score sums already loaded
// (lane i: class i's cpu / memory sums; any value past U): lane i holds class i's key; its
// place in the (key, class) order and its dense rank are counts over the other lanes
// (readlane broadcasts, no barrier per bitonic stage).  Every thread of the block calls it.
__device__ inline void wave_class_rank(const ca_template& tp, int64_t s_cpu, int64_t s_mem, int32_t U, int32_t NP,
                                       uint64_t* key, uint32_t* idx, int32_t* sc) {
    const int64_t acpu = tp.node.alloc_milli_cpu, amem = tp.node.alloc_memory;
    if (threadIdx.x < 64) {
        const int lane = (int)threadIdx.x;
        uint64_t k = ~0ull;
        if (lane < U) {
            double score = 0.0;               // calculatePodScore, same float64 operations
            if (acpu > 0) score += (double)s_cpu / (double)acpu;
            if (amem > 0) score += (double)s_mem / (double)amem;
            k = ~ordered_bits(score);
        }
        const uint32_t klo = (uint32_t)k, khi = (uint32_t)(k >> 32);
        int pos = 0, eq_before = 0;
        for (int j = 0; j < NP; j++) {
            const uint64_t kj = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(khi, j) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane(klo, j);
            pos += (kj < k || (kj == k && j < lane)) ? 1 : 0;
            eq_before += (kj == k && j < lane) ? 1 : 0;
        }
        const int first = eq_before == 0 ? 1 : 0;           // the lowest class holding its key
        int dense = 0;
        for (int j = 0; j < NP; j++) {
            const uint64_t kj = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(khi, j) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane(klo, j);
            dense += (__builtin_amdgcn_readlane(first, j) && kj < k) ? 1 : 0;
        }
        if (lane < NP) { key[pos] = k; idx[pos] = (uint32_t)lane; sc[pos] = dense; }
    }
    __syncthreads();
}

__device__ inline void block_class_rank(const ca_template& tp, const int64_t* __restrict__ cls_sc, int32_t U,
                                        int32_t NP, uint64_t* key, uint32_t* idx, int32_t* sc) {
    const int64_t acpu = tp.node.alloc_milli_cpu, amem = tp.node.alloc_memory;
    if (NP <= 64) {
        const int l = (int)threadIdx.x;
        const int64_t c0 = l < U ? cls_sc[2 * l] : 0, c1 = l < U ? cls_sc[2 * l + 1] : 0;
        wave_class_rank(tp, c0, c1, U, NP, key, idx, sc);
        return;
    }
    for (int i = threadIdx.x; i < NP; i += blockDim.x) {
        uint64_t k = ~0ull;
        if (i < U) {
            // calculatePodScore (binpacking_estimator.go:164-193), same float64 operations
            double score = 0.0;
            if (acpu > 0) score += (double)cls_sc[2 * i] / (double)acpu;
            if (amem > 0) score += (double)cls_sc[2 * i + 1] / (double)amem;
            k = ~ordered_bits(score);            // ascending key == descending score
        }
        key[i] = k;
        idx[i] = (uint32_t)i;
    }
    __syncthreads();
    for (int k = 2; k <= NP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < NP; t += blockDim.x) {
                const int ixj = t ^ j;
                if (ixj > t) {
                    const uint64_t a = key[t], b = key[ixj];
                    const uint32_t ia = idx[t], ib = idx[ixj];
                    const bool up = (t & k) == 0;
                    const bool less_ba = b < a || (b == a && ib < ia);
                    const bool less_ab = a < b || (a == b && ia < ib);
                    if (up ? less_ba : less_ab) { key[t] = b; key[ixj] = a; idx[t] = ib; idx[ixj] = ia; }
                }
            }
            __syncthreads();
        }
    }
    // dense rank: number of distinct keys before
    for (int i = threadIdx.x; i < NP; i += blockDim.x) sc[i] = (i > 0 && key[i] != key[i - 1]) ? 1 : 0;
    __syncthreads();
    for (int o = 1; o < NP; o <<= 1) {
        int32_t v[CLS_MAX / 1024];
        int n = 0;
        for (int i = threadIdx.x; i < NP; i += blockDim.x) v[n++] = (i >= o ? sc[i - o] : 0);
        __syncthreads();
        n = 0;
        for (int i = threadIdx.x; i < NP; i += blockDim.x) sc[i] += v[n++];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(1024) k_class_rank(const GroupMeta* __restrict__ groups,
                                                    const ca_template* __restrict__ tmpls,
                                                    const int64_t* __restrict__ cls_sc, int32_t U, int32_t NP,
                                                    int32_t* __restrict__ crank,
    const int32_t* __restrict__ gmap) {
    __shared__ uint64_t key[CLS_MAX];
    __shared__ uint32_t idx[CLS_MAX];
    __shared__ int32_t sc[CLS_MAX];
    const int gi = GSEL(blockIdx.x);
    const GroupMeta gm = groups[gi];
    block_class_rank(tmpls[gm.tmpl], cls_sc, U, NP, key, idx, sc);
    for (int i = threadIdx.x; i < U; i += blockDim.x) crank[(size_t)gi * U + idx[i]] = sc[i];
}

__device__ inline uint32_t item_digit(const GroupMeta& gm, const uint32_t* __restrict__ src, int32_t i,
                                      const int32_t* __restrict__ pod_idx, const int32_t* __restrict__ pcls,
                                      const int32_t* __restrict__ crank_g, int shift, uint32_t* pos_out) {
    const uint32_t pos = src ? src[gm.off + i] : (uint32_t)i;
    *pos_out = pos;
    const int32_t pidx = pod_idx[gm.off + (int32_t)pos];
    return ((uint32_t)crank_g[pcls[pidx]] >> shift) & 255u;
}

__global__ void __launch_bounds__(RTHREADS) k_radix_hist(const GroupMeta* __restrict__ groups,
                                                        const uint32_t* __restrict__ src,
                                                        const int32_t* __restrict__ pod_idx,
                                                        const int32_t* __restrict__ pcls,
                                                        const int32_t* __restrict__ crank, int32_t U, int shift,
                                                        int32_t* __restrict__ hist, const int32_t* __restrict__ gmap) {
    __shared__ int32_t h[256];
    const int gi = GSEL(blockIdx.y);
    const GroupMeta gm = groups[gi];
    const int32_t t = (int32_t)blockIdx.x;
    if (t >= gm.rtiles) return;
    h[threadIdx.x] = 0;
    __syncthreads();
    const int32_t* cr = crank + (size_t)gi * U;
    const int32_t base = t * RT;
    for (int r = 0; r < RPT; r++) {
        const int32_t i = base + r * RTHREADS + (int32_t)threadIdx.x;
        if (i < gm.count) {
            uint32_t pos;
            atomicAdd(&h[item_digit(gm, src, i, pod_idx, pcls, cr, shift, &pos)], 1);
        }
    }
    __syncthreads();
    hist[gm.hoff + (int32_t)threadIdx.x * gm.rtiles + t] = h[threadIdx.x];
}

// exclusive scan of the group's [256][rtiles] histogram, digit-major: thread d owns
// digit d's row (its tiles, contiguous), so the scan is one row sum per thread, one
// block scan of the 256 row totals and one pass writing the row's prefixes — two
// barriers instead of two per 256 entries.
__global__ void __launch_bounds__(256) k_radix_scan(const GroupMeta* __restrict__ groups, int32_t* __restrict__ hist,
                                                   const int32_t* __restrict__ gmap) {
    __shared__ int32_t wsum[4];
    const GroupMeta gm = groups[GSEL(blockIdx.x)];
    const int32_t nt = gm.rtiles;
    int32_t* row = hist + gm.hoff + (int32_t)threadIdx.x * nt;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int32_t tot = 0;
    for (int32_t j = 0; j < nt; j++) tot += row[j];
    int32_t x = tot;                                     // inclusive wave scan of row totals
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int32_t pre = x - tot;
    for (int q = 0; q < w; q++) pre += wsum[q];
    for (int32_t j = 0; j < nt; j++) {
        const int32_t v = row[j];
        row[j] = pre;
        pre += v;
    }
}

__global__ void __launch_bounds__(RTHREADS) k_radix_scatter(const GroupMeta* __restrict__ groups,
                                                           const uint32_t* __restrict__ src,
                                                           const int32_t* __restrict__ pod_idx,
                                                           const int32_t* __restrict__ pcls,
                                                           const int32_t* __restrict__ crank, int32_t U, int shift,
                                                           const int32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ dst, const int32_t* __restrict__ gmap) {
    __shared__ int32_t wcnt[RTHREADS / 64][256];
    const int gi = GSEL(blockIdx.y);
    const GroupMeta gm = groups[gi];
    const int32_t t = (int32_t)blockIdx.x;
    if (t >= gm.rtiles) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int d = lane; d < 256; d += 64) wcnt[w][d] = 0;
    __builtin_amdgcn_wave_barrier();
    const int32_t* cr = crank + (size_t)gi * U;
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t dg[RCH], pv[RCH];
    int32_t rk[RCH];
    const int32_t wbase = t * RT + w * (RCH * 64);       // wave w owns RCH consecutive chunks
    for (int c = 0; c < RCH; c++) {
        const int32_t i = wbase + c * 64 + lane;
        const bool valid = i < gm.count;
        uint32_t pos = 0, d = 0;
        if (valid) d = item_digit(gm, src, i, pod_idx, pcls, cr, shift, &pos);
        uint64_t peers = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const int32_t before = wcnt[w][valid ? d : 0];
        const int32_t r = before + __builtin_popcountll(peers & lt);
        __builtin_amdgcn_wave_barrier();
        if (valid && (peers & lt) == 0) wcnt[w][d] = before + __builtin_popcountll(peers);
        __builtin_amdgcn_wave_barrier();
        dg[c] = valid ? d : 0xFFFFFFFFu;
        pv[c] = pos;
        rk[c] = r;
    }
    __syncthreads();
    // offset of wave w inside each digit of the tile: the counts of waves before it
    int32_t pre[RTHREADS / 64];
    if (threadIdx.x < 256) {
        int32_t acc = 0;
        for (int q = 0; q < RTHREADS / 64; q++) { pre[q] = acc; acc += wcnt[q][threadIdx.x]; }
    }
    __syncthreads();
    if (threadIdx.x < 256)
        for (int q = 0; q < RTHREADS / 64; q++) wcnt[q][threadIdx.x] = pre[q] + hist[gm.hoff + (int32_t)threadIdx.x * gm.rtiles + t];
    __syncthreads();
    for (int c = 0; c < RCH; c++) {
        if (dg[c] == 0xFFFFFFFFu) continue;
        dst[gm.off + wcnt[w][dg[c]] + rk[c]] = pv[c];
    }
}

// 1*-3*. decoupled Go order: the stable class order of a group is its
// classes in rank order, each class's pods together, and every pod of a class is the same
// record but for its controller — so the chain stream follows from per-class counts alone,
// with no sort of the pod list.  k_run_table (one workgroup per group; the class ranks
// computed in its prologue): the class counts of the group's list, each rank's first
// stream position rstart[g][r] (r in [0, U]), and the stream record of the rank's class
// rsp[g][r] (its representative pod's requests and static bits against the template);
// round 1 without k_round_init it also sets the group's lastIndex input / need /
// unsupported flags.  k_emit_runs: the stream itself.  The pod id of a stream entry is not
// needed: decoupled chains emit stream positions and the consumers map them through the
// Go-order ids.
#ifdef CASIM_PROF
// k_run_table phase cycles per group slot (< 1024): ranking, counts by rank + scan, records
__device__ unsigned long long g_rt_prof[1024][3];
#endif
// Class counts of every group's list, cls_cnt[g][c] (indexed by class, not by rank), once
// per plan: the lists are written at plan creation and never change, so the pass over them
// does not belong in front of every run's heaviest chain.  One workgroup per tile of
// CLS_HIST_TILE positions of one group; each wave counts a contiguous quarter of the tile,
// 64 positions per step, adding a run of equal classes up in a register (classes come in
// runs) and touching the workgroup's LDS histogram once per run; one global atomicAdd per
// class present in the tile.  The table is zeroed on the same stream ahead of the launch.
constexpr int CLS_HIST_TILE = 4096;    // (abi.CLS_HIST_TILE)
__global__ void __launch_bounds__(256) k_cls_hist(const GroupMeta* __restrict__ groups,
                                                 const int32_t* __restrict__ item_cls, int32_t U,
                                                 int32_t* __restrict__ cls_cnt) {
    __shared__ int32_t h[CLS_MAX];
    const GroupMeta gm = groups[blockIdx.y];
    const int32_t base = (int32_t)blockIdx.x * CLS_HIST_TILE;
    if (base >= gm.count) return;                                   // (uniform per block)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int c = tid; c < U; c += 256) h[c] = 0;
    __syncthreads();
    constexpr int PER_W = CLS_HIST_TILE / 4, STEPS = PER_W / 64;
    const int32_t end = min(gm.count, base + CLS_HIST_TILE);
    const int32_t wb0 = min(end, base + w * PER_W), wb1 = min(end, wb0 + PER_W);
    int32_t cv[STEPS];
#pragma unroll
    for (int u = 0; u < STEPS; u++) {
        const int32_t i = wb0 + u * 64 + lane;
        cv[u] = i < wb1 ? item_cls[gm.off + i] : -1;
    }
    int32_t cur = -1, acc = 0;                // (wave-uniform) the run being added up
#pragma unroll
    for (int u = 0; u < STEPS; u++) {
        const bool valid = cv[u] >= 0 && cv[u] < U;
        const int32_t c = cv[u];
        const uint64_t vm = __ballot(valid);
        if (!vm) continue;
        const int32_t c0 = __builtin_amdgcn_readlane(c, __builtin_ctzll(vm));
        if (__ballot(valid && c != c0) == 0) {          // one class in this step
            if (c0 == cur) {
                acc += __builtin_popcountll(vm);
            } else {
                if (acc > 0 && lane == 0) atomicAdd(&h[cur], acc);
                cur = c0;
                acc = __builtin_popcountll(vm);
            }
            continue;
        }
        uint64_t act = vm;                                // a class boundary in the step
        while (act) {
            const int l = __builtin_ctzll(act);
            const int32_t cl = __builtin_amdgcn_readlane(c, l);
            const uint64_t m = __ballot(valid && c == cl) & act;
            if (lane == l) atomicAdd(&h[cl], __builtin_popcountll(m));
            act &= ~m;
        }
    }
    if (acc > 0 && lane == 0) atomicAdd(&h[cur], acc);
    __syncthreads();
    int32_t* out = cls_cnt + (size_t)blockIdx.y * U;
    for (int c = tid; c < U; c += 256)
        if (h[c] > 0) atomicAdd(&out[c], h[c]);
}

// A request and its reciprocal in float64, for the copy counts of a run (run_div below;
// k_run_table writes the same two per rank).  req == 0: rcp = +inf, the quotient inf (NaN
// for free == 0) and fmin(., cap) gives cap — a zero request passes whenever free >= 0.
__device__ inline double run_req(int64_t req) { return (double)req; }
__device__ inline double run_rcp(int64_t req) { return req > 0 ? 1.0 / (double)req : __builtin_inf(); }
constexpr int RDIV_N = 7;      // doubles per rank in k_run_table's rdiv: 3 requests, 3 reciprocals, fresh-copy count

__device__ inline int32_t run_rank(const int32_t* __restrict__ st, int32_t U, int32_t i) {
    int32_t lo = 0, hi = U;                  // the last r with st[r] <= i (st[U] is never read)
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (st[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(1024) k_run_table(const GroupMeta* __restrict__ groups,
                                                   const int32_t* __restrict__ cls_cnt,
                                                   const int64_t* __restrict__ cls_sc, int32_t NP,
                                                   const int32_t* __restrict__ cls_rep,
                                                   int32_t U, const ca_template* __restrict__ tmpls,
                                                   const PodHot* __restrict__ ph, const ca_pod_spec* __restrict__ specs,
                                                   const ca_selector_term* __restrict__ terms,
                                                   const ca_selector_req* __restrict__ reqs, int32_t* __restrict__ rstart,
                                                   StreamPod* __restrict__ rsp, uint32_t* __restrict__ group_unsup,
                                                   const int32_t* __restrict__ gmap,
                                                   int32_t* __restrict__ lin, uint8_t* __restrict__ need, int32_t lin0,
                                                   double* __restrict__ rdiv) {
    // lin != null: round 1 without k_round_init — the group's lastIndex input, need flag and
    // unsupported flag are set here (stored, not or-ed)
    // rdiv != null: rdiv[g][r][0..6) the rank's requests and their reciprocals in float64
    // (run_div's values, one thread per class here instead of once per run on the chain), and
    // rdiv[g][r][6] the copies of the class's pod on a fresh template copy, capped at the
    // group's pod count (the lean chain's closed-form opening takes min(., pods left in the run))
    __shared__ int32_t cnt[CLS_MAX];
    __shared__ uint32_t s_unsup;
    __shared__ int32_t rc[CLS_MAX];
    __shared__ int32_t cr[CLS_MAX];           // rank of each class
    __shared__ uint64_t key[CLS_MAX];
    __shared__ uint32_t idx[CLS_MAX];
    __shared__ int32_t wsum[16];
    const int gi = GSEL(blockIdx.x);
    const GroupMeta gm = groups[gi];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_unsup = 0;
#ifdef CASIM_PROF
    const uint64_t t_r0 = clock64();
#endif
    // The class counts of the group's list come from the plan (k_cls_hist, once at creation:
    // the list pass took ~40k of this kernel's ~65k cycles in front of the heaviest chain,
    // DESIGN §8).  They are requested first, with the class scores (ranking, up to 64
    // classes), so the ranking waits only for the scores.
    const bool small = NP <= 64;
    int64_t s_cpu = 0, s_mem = 0;
    if (small && tid < U) { s_cpu = cls_sc[2 * tid]; s_mem = cls_sc[2 * tid + 1]; }
    const int32_t* gcnt = cls_cnt + (size_t)gi * U;
    int32_t my[CLS_MAX / 1024];               // classes tid, tid + 1024, ...
#pragma unroll
    for (int q = 0; q < CLS_MAX / 1024; q++) {
        const int c = tid + q * 1024;
        my[q] = c < U ? gcnt[c] : 0;
    }
    if (small) wave_class_rank(tmpls[gm.tmpl], s_cpu, s_mem, U, NP, key, idx, rc);   // (rc: scratch)
    else block_class_rank(tmpls[gm.tmpl], cls_sc, U, NP, key, idx, rc);
    for (int i = tid; i < U; i += 1024) cr[idx[i]] = rc[i];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CLS_MAX / 1024; q++) {
        const int c = tid + q * 1024;
        if (c < U) { cnt[c] = my[q]; rc[c] = 0; }
    }
    __syncthreads();
#ifdef CASIM_PROF
    const uint64_t t_r1 = clock64();
#endif
    for (int c = tid; c < U; c += 1024)
        if (cnt[c] > 0) atomicAdd(&rc[cr[c]], cnt[c]);
    __syncthreads();
    // exclusive scan of the counts by rank: thread t owns ranks [4t, 4t + 4)
    int32_t v[4], loc = 0;
    for (int q = 0; q < 4; q++) { const int r = 4 * tid + q; v[q] = r < U ? rc[r] : 0; loc += v[q]; }
    int32_t x = loc;
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int32_t pre = x - loc;
    for (int q = 0; q < w; q++) pre += wsum[q];
    int32_t* rs = rstart + (size_t)gi * (U + 1);
    for (int q = 0; q < 4; q++) {
        const int r = 4 * tid + q;
        if (r < U) rs[r] = pre;
        pre += v[q];
    }
    if (tid == 0) rs[U] = gm.count;
#ifdef CASIM_PROF
    const uint64_t t_r3 = clock64();
#endif
    // the record of each present class, at its rank
    const ca_template& tp = tmpls[gm.tmpl];
    const bool tunsched = (tp.node.flags & CA_NODE_UNSCHEDULABLE) != 0;
    uint32_t unsup = 0;
    for (int c = tid; c < U; c += 1024) {
        if (cnt[c] == 0) continue;
        const PodHot p = ph[cls_rep[c]];
        const uint32_t sf = static_sf(p, tp, tunsched, specs, terms, reqs);
        StreamPod sp;
        sp.cpu = p.cpu; sp.mem = p.mem; sp.eph = p.eph;
        sp.pod = cls_rep[c];
        sp.flags = sf | (batchable(p, sf) ? SF_BATCH : 0u);
        rsp[(size_t)gi * U + cr[c]] = sp;
        if (rdiv) {
            double* d = rdiv + ((size_t)gi * U + cr[c]) * RDIV_N;
            const int64_t req[3] = {p.cpu, p.mem, p.eph};
            for (int i = 0; i < 3; i++) {
                d[i] = run_req(req[i]);
                d[3 + i] = run_rcp(req[i]);
            }
            d[6] = (double)co_fresh_copies(gm.tcpu, gm.tmem, gm.teph, gm.tpods, d, d + 3, (sf & SF_ZERO) != 0, gm.count);
        }
        unsup |= sf & SF_UNSUP;
    }
    if (unsup) atomicOr(&s_unsup, 1u);
    __syncthreads();                              // s_unsup
    if (tid == 0) {
        if (lin) { lin[gi] = lin0; need[gi] = 1; group_unsup[gi] = s_unsup ? 1u : 0u; }
        else if (s_unsup) atomicOr(&group_unsup[gi], 1u);
#ifdef CASIM_PROF
        if (gi < 1024) {
            const uint64_t t_r4 = clock64();
            g_rt_prof[gi][0] = t_r1 - t_r0; g_rt_prof[gi][1] = t_r3 - t_r1; g_rt_prof[gi][2] = t_r4 - t_r3;
        }
#endif
    }
}

// The stream from the run table: one thread per position — position -> rank by binary
// search of the rank starts in LDS, the record, run heads exactly as k_emit_bucket marks
// them.  (Measured against a variant inside k_run_table, one thread per 64-position
// window: 0.49 against 0.50 ms per headline step — the wide grid wins.)
__global__ void __launch_bounds__(256) k_emit_runs(const GroupMeta* __restrict__ groups,
                                                  const int32_t* __restrict__ rstart, const StreamPod* __restrict__ rsp,
                                                  int32_t U, StreamPod* __restrict__ out, uint64_t* __restrict__ heads,
                                                  const int32_t* __restrict__ gmap, int32_t all_windows) {
    __shared__ int32_t st[CLS_MAX + 1];
    const int gi = GSEL(blockIdx.y);
    const GroupMeta gm = groups[gi];
    const int32_t base = (int32_t)(blockIdx.x * blockDim.x);
    if (base >= gm.count) return;                                   // (uniform per block)
    const int32_t* rs = rstart + (size_t)gi * (U + 1);
    for (int r = threadIdx.x; r <= U; r += blockDim.x) st[r] = rs[r];
    __syncthreads();
    const int32_t i = base + (int32_t)threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (base + (int32_t)(threadIdx.x & ~63u) >= gm.count) return;   // whole wave past the end
    bool head = true;
    StreamPod sp = {};
    if (i < gm.count) {
        const int32_t r = run_rank(st, U, i);
        sp = rsp[(size_t)gi * U + r];
        const bool bat = (sp.flags & SF_BATCH) != 0;
        if (i > 0 && bat) {
            head = false;
            if (i == st[r]) {                                       // first pod of its class
                const StreamPod q = rsp[(size_t)gi * U + run_rank(st, U, i - 1)];
                head = !((q.flags & ~SF_BATCH) == (sp.flags & ~SF_BATCH) && q.cpu == sp.cpu && q.mem == sp.mem &&
                         q.eph == sp.eph);
            }
        }
        sp.flags |= head ? SF_HEAD : 0u;
    }
    const uint64_t hb = __ballot(head);
    if (lane == 0) heads[gm.moff + (i >> 6)] = hb;
    // With run batching the chain reads a stream entry only at a run head or inside a
    // non-batchable run (whose every pod is a head), and only from the 64-entry window
    // holding it: windows without a head are never read, so they are not written (C2: ~1
    // window in 10 has a head).  The per-pod chain (CASIM_RUN_BATCH=0) reads every window.
    if ((hb != 0 || all_windows) && i < gm.count) out[gm.off + i] = sp;
}

// 1''-2''. Go 1.19 sort.Slice order (binpacking_estimator.go:74; pdqsort.h) ----------
// One 1024-thread workgroup per group: the rank of every position of the group's list
// (its class's dense rank, k_class_rank, or an explicit per-position rank from
// k_item_rank), then pdqsort_func's exact permutation.  Groups of at most lds_n pods with
// at most 256 ranks sort in LDS (16-bit positions + 8-bit ranks); the others in global
// memory (rank above position in 32 or 64 bits).  Output: sorted[off + k] = position of
// the k-th pod, the same layout as the radix sort's.  force (tests): 1 LDS, 2 / 3 global.
// Scratch per group: gE [off, off+n) (8 B), scr [off, off+n), stack from off/2 + 2g.
constexpr int PDQ_LDS_N = 50368;       // ~3.16 B per pod + the static control block (~4.6 KB) <= 160 KB
// dynamic LDS of k_pdq_sort for groups of up to lds_n pods: positions (2 B), ranks (1 B),
// the partition's right-zone bitmap (1 bit) and its per-word prefix counts (2 B / 64)
__host__ __device__ inline size_t pdq_lds_bytes(int32_t lds_n) {
    const size_t np = ((size_t)std::max(lds_n, 0) + 63) & ~(size_t)63;
    return (3 * np + np / 8 + 2 * (np / 64 + 1) + 15) & ~(size_t)15;
}

// Two-launch sort of the decoupled path: lists longer than FAN_MIN positions stop after the
// workgroup step that leaves FAN_PARTS long frames pending (FAN_TOP_STEPS steps at most)
// and finish in up to FAN_PARTS part workgroups.  Knobs (diagnostics): CASIM_SORT_FAN=0
// turns it off, CASIM_SORT_FAN_MIN / _PARTS / _STEPS replace the defaults.
constexpr int32_t FAN_MIN = 8192, FAN_PARTS = 8, FAN_TOP_STEPS = 4;
inline void fan_knobs(int32_t* parts, int32_t* fmin, int32_t* steps) {
    *parts = FAN_PARTS;
    *fmin = FAN_MIN;
    *steps = FAN_TOP_STEPS;
    if (const char* e = knob_env("CASIM_SORT_FAN_PARTS")) *parts = atoi(e);
    if (const char* e = knob_env("CASIM_SORT_FAN_MIN")) *fmin = std::max(0, atoi(e));
    if (const char* e = knob_env("CASIM_SORT_FAN_STEPS")) *steps = atoi(e);
    *parts = std::min(std::max(*parts, 1), (int32_t)pdq::FAN_PARTS_MAX);
    *steps = std::min(std::max(*steps, 1), (int32_t)pdq::FAN_STEPS_MAX);
    if (const char* e = knob_env("CASIM_SORT_FAN")) if (atoi(e) == 0) *parts = 0;
}

#ifndef CASIM_PDQ_UB
#define CASIM_PDQ_UB 8
#endif
constexpr int PDQ_UB = CASIM_PDQ_UB;   // list positions per thread whose gathers are in flight together
__global__ void __launch_bounds__(pdq::NT) k_pdq_sort(const GroupMeta* __restrict__ groups,
                                                     const int32_t* __restrict__ pod_idx,
                                                     const int32_t* __restrict__ pcls,
                                                     const int32_t* __restrict__ crank, int32_t U,
                                                     const uint32_t* __restrict__ item_rank,
                                                     uint32_t* __restrict__ sorted, uint64_t* __restrict__ gE,
                                                     uint64_t* __restrict__ xs_all, pdq::Frame* __restrict__ stack_all,
                                                     int32_t lds_n, int32_t force, int32_t limit0, const int32_t* __restrict__ gmap,
                                                     int32_t* __restrict__ ids_out, int32_t* __restrict__ fan,
                                                     int32_t ids_epoch, const int32_t* __restrict__ item_cls,
                                                     const ca_template* __restrict__ tmpls,
                                                     const int64_t* __restrict__ cls_sc, int32_t NP,
                                                     int32_t fan_parts, int32_t fan_min, int32_t fan_steps) {
    // fan != null: the group's record of the fan table (pdqsort.h FAN_*) is written — the
    // part bounds and ready flags the publisher waits on.  fan_parts > 0: an LDS-store sort
    // of more than fan_min positions runs only its top phase here and hands its pending
    // frames to k_pdq_sort_parts (below); every other sort ends here as one part.
    extern __shared__ __align__(16) unsigned char pdq_dyn[];
    __shared__ pdq::Ctl ctl;
#ifdef CASIM_PROF
    const uint64_t t_k0 = clock64();
#endif
    const int gi = GSEL(blockIdx.x);
    const GroupMeta gm = groups[gi];
    const int32_t n = gm.count, off = gm.off;
    const int tid = threadIdx.x;
    uint32_t* scr = reinterpret_cast<uint32_t*>(xs_all + off);    // ranks, then the exchange scratch
    pdq::Frame* stack = stack_all + off / 2 + 2 * gi;
    if (tid == 0) ctl.rmax = 0;
    __syncthreads();
    const bool fit = n <= lds_n;
    const size_t npad = ((size_t)lds_n + 63) & ~(size_t)63;
    uint16_t* e16 = reinterpret_cast<uint16_t*>(pdq_dyn);
    uint8_t* rk = pdq_dyn + 2 * npad;
    uint64_t* rmb = reinterpret_cast<uint64_t*>(pdq_dyn + 3 * npad);
    uint16_t* rmp = reinterpret_cast<uint16_t*>(rmb + npad / 64);
    // cls_sc != null: the class ranks are computed here (k_class_rank's work, one launch
    // less on the sort's critical path): the bitonic scratch lives in the element store
    // (free until the ranks are loaded), the rank of each class in the partition bitmap
    // area (free until the first partition); the host checks both fit
    const uint16_t* crk = nullptr;
    // the first slice of the list's classes is requested before the class ranking, so its
    // latency hides behind the ranking's barriers
    int32_t pre[PDQ_UB];
    const bool preload = item_cls && !item_rank;
    if (preload) {
#pragma unroll
        for (int u = 0; u < PDQ_UB; u++) { const int32_t i = tid + u * pdq::NT; pre[u] = i < n ? item_cls[off + i] : 0; }
    }
    if (cls_sc) {
        uint64_t* key = reinterpret_cast<uint64_t*>(pdq_dyn);
        uint32_t* idx = reinterpret_cast<uint32_t*>(pdq_dyn + 8 * (size_t)NP);
        int32_t* scv = reinterpret_cast<int32_t*>(pdq_dyn + 12 * (size_t)NP);
        block_class_rank(tmpls[gm.tmpl], cls_sc, U, NP, key, idx, scv);
        uint16_t* w = reinterpret_cast<uint16_t*>(rmb);
        for (int i = tid; i < U; i += pdq::NT) w[idx[i]] = (uint16_t)scv[i];
        __syncthreads();
        crk = w;
    }
    uint32_t rmax = 0;
    // the ranks of the list: a chain of three dependent gathers per position (list -> pod ->
    // class -> rank), issued PDQ_UB positions at a time so their latencies overlap
    for (int32_t i0 = tid; i0 < n; i0 += pdq::NT * PDQ_UB) {
        uint32_t r[PDQ_UB];
        if (item_rank) {
#pragma unroll
            for (int u = 0; u < PDQ_UB; u++) { const int32_t i = i0 + u * pdq::NT; r[u] = i < n ? item_rank[off + i] : 0u; }
        } else {
            int32_t pi[PDQ_UB], cl[PDQ_UB];
            if (item_cls && preload && i0 == tid) {
#pragma unroll
                for (int u = 0; u < PDQ_UB; u++) cl[u] = pre[u];
            } else if (item_cls) {
#pragma unroll
                for (int u = 0; u < PDQ_UB; u++) { const int32_t i = i0 + u * pdq::NT; cl[u] = i < n ? item_cls[off + i] : 0; }
            } else {
#pragma unroll
                for (int u = 0; u < PDQ_UB; u++) { const int32_t i = i0 + u * pdq::NT; pi[u] = i < n ? pod_idx[off + i] : 0; }
#pragma unroll
                for (int u = 0; u < PDQ_UB; u++) { const int32_t i = i0 + u * pdq::NT; cl[u] = i < n ? pcls[pi[u]] : 0; }
            }
#pragma unroll
            for (int u = 0; u < PDQ_UB; u++) {
                const int32_t i = i0 + u * pdq::NT;
                r[u] = i < n ? (crk ? (uint32_t)crk[cl[u]] : (uint32_t)crank[(size_t)gi * U + cl[u]]) : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < PDQ_UB; u++) {
            const int32_t i = i0 + u * pdq::NT;
            if (i >= n) break;
            rmax = max(rmax, r[u]);
            if (fit) { e16[i] = (uint16_t)i; rk[i] = (uint8_t)r[u]; }
            else scr[i] = r[u];                        // (the LDS store keeps its ranks in LDS)
        }
    }
    for (int d = 32; d >= 1; d >>= 1) rmax = max(rmax, (uint32_t)__shfl_xor((int)rmax, d, 64));
    if ((tid & 63) == 0) atomicMax(&ctl.rmax, rmax);
    __syncthreads();
    const uint32_t R = ctl.rmax;
    int mode = (fit && R < 256) ? 1 : (n <= (1 << 20) && R < 4096) ? 2 : 3;
    if (force == 1 && fit && R < 256) mode = 1;
    else if (force == 2 && n <= (1 << 20) && R < 4096) mode = 2;
    else if (force == 3) mode = 3;
    if (mode != 1 && fit) {
        // the ranks went to LDS only (8 bits): gather them again for a global store (a group
        // that fits LDS but has >= 256 ranks, or a forced store in tests)
        for (int32_t i = tid; i < n; i += pdq::NT) {
            uint32_t r;
            if (item_rank) r = item_rank[off + i];
            else {
                const int32_t cl = item_cls ? item_cls[off + i] : pcls[pod_idx[off + i]];
                r = crk ? (uint32_t)crk[cl] : (uint32_t)crank[(size_t)gi * U + cl];
            }
            scr[i] = r;
        }
        __syncthreads();
    }
    if (mode == 1) {
        const pdq::LdsStore st{e16, rk, rmb, rmp};
#ifdef CASIM_PROF
        const uint64_t t_k1 = clock64();
#endif
        // (one call of the step loop for both forms: its code is the kernel's largest part)
        const bool fanned = fan && fan_parts > 0 && n > fan_min;
        const int cap = n / 2 + 2;
        pdq::wg_sort_root<pdq::LdsStore>(n, stack, cap, ctl, limit0);
        pdq::wg_steps(st, n, stack, cap, scr, ctl, fanned ? fan_parts : 0, fan_steps);
#ifdef CASIM_PROF
        const uint64_t t_k2f = clock64();
#endif
        if (fanned) {
            // top phase: the steps stopped with enough long frames pending; the store (position
            // and rank per element; gE is otherwise unused by this store), the frame counts
            // and the split go to global memory.  The frames are in `stack` already.
            uint32_t* spill = reinterpret_cast<uint32_t*>(gE + off);
            for (int32_t i = tid; i < n; i += pdq::NT) spill[i] = st.ld(i);
            int32_t* fr = fan + (size_t)gi * pdq::FAN_STRIDE;
            const int np = pdq::wg_fan_split(stack, cap, ctl, n, fan_parts, fr + pdq::FAN_LO);
            if (tid == 0) {
                fr[pdq::FAN_NPARTS] = np;
                fr[pdq::FAN_FANNED] = 1;
                fr[pdq::FAN_TOP] = ctl.top;
                fr[pdq::FAN_NSMALL] = ctl.nsmall;
                __threadfence();
                __hip_atomic_store(&fr[pdq::FAN_BOUNDS], ids_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
#ifdef CASIM_PROF
                if (gi < 128) {
                    const uint64_t t_k3 = clock64();
                    pdq::g_pdq_wg[3 * gi] = t_k3 - t_k0;
                    pdq::g_pdq_wg[3 * gi + 1] = t_k1 - t_k0;
                    pdq::g_pdq_wg[3 * gi + 2] = t_k3 - t_k2f;         // (fanned: spill + split)
                }
#endif
            }
            return;
        }
        pdq::wg_short(st, stack, cap, ctl);
#ifdef CASIM_PROF
        const uint64_t t_k2 = clock64();
#endif
        if (ids_out) {
            // decoupled Go order: the pod ids in sorted order, gathered straight from the
            // group's list (pod_idx[off + e16[k]], PDQ_UB positions per thread in flight).
            // With the stream chains this gather was ~40 % of the slowest workgroup's time on
            // C2 and the list went through LDS in coalesced slices instead; with the run-table
            // chains (no stream traffic beside the sort) the gather is the faster of the two,
            // with one workgroup per group as with shared sorts (profiles/sort_share_ab.txt).
            for (int32_t k0 = tid; k0 < n; k0 += pdq::NT * PDQ_UB) {
                int32_t v[PDQ_UB];
#pragma unroll
                for (int u = 0; u < PDQ_UB; u++) { const int32_t k = k0 + u * pdq::NT; v[u] = k < n ? pod_idx[off + (int32_t)e16[k]] : 0; }
#pragma unroll
                for (int u = 0; u < PDQ_UB; u++) { const int32_t k = k0 + u * pdq::NT; if (k < n) ids_out[off + k] = v[u]; }
            }
        } else
            for (int32_t k = tid; k < n; k += pdq::NT) sorted[off + k] = e16[k];
#ifdef CASIM_PROF
        __syncthreads();
        if (tid == 0 && gi < 128) {
            const uint64_t t_k3 = clock64();
            pdq::g_pdq_wg[3 * gi] = t_k3 - t_k0;
            pdq::g_pdq_wg[3 * gi + 1] = t_k1 - t_k0;
            pdq::g_pdq_wg[3 * gi + 2] = t_k3 - t_k2;
        }
#endif
    } else if (mode == 2) {
        uint32_t* e = reinterpret_cast<uint32_t*>(gE + off);
        for (int32_t i = tid; i < n; i += pdq::NT) e[i] = (scr[i] << 20) | (uint32_t)i;
        __syncthreads();
        const pdq::G32Store st{e};
        pdq::wg_sort(st, n, stack, n / 2 + 2, scr, ctl, limit0);
        if (ids_out)
            for (int32_t k = tid; k < n; k += pdq::NT) ids_out[off + k] = pod_idx[off + (int32_t)(e[k] & 0xFFFFFu)];
        else
            for (int32_t k = tid; k < n; k += pdq::NT) sorted[off + k] = e[k] & 0xFFFFFu;
    } else {
        uint64_t* e = gE + off;
        for (int32_t i = tid; i < n; i += pdq::NT) e[i] = ((uint64_t)scr[i] << 32) | (uint32_t)i;
        __syncthreads();
        const pdq::G64Store st{e};
        pdq::wg_sort(st, n, stack, n / 2 + 2, xs_all + off, ctl, limit0);
        if (ids_out)
            for (int32_t k = tid; k < n; k += pdq::NT) ids_out[off + k] = pod_idx[off + (int32_t)(uint32_t)e[k]];
        else
            for (int32_t k = tid; k < n; k += pdq::NT) sorted[off + k] = (uint32_t)e[k];
    }
    if (fan) {                                         // this group's ids are final: one part
        __syncthreads();
        if (tid == 0) {
            int32_t* fr = fan + (size_t)gi * pdq::FAN_STRIDE;
            fr[pdq::FAN_NPARTS] = 1;
            fr[pdq::FAN_FANNED] = 0;
            fr[pdq::FAN_LO] = 0;
            fr[pdq::FAN_LO + 1] = n;
            __threadfence();
            __hip_atomic_store(&fr[pdq::FAN_BOUNDS], ids_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&fr[pdq::FAN_FLAG], ids_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The second launch of the two-launch sort, queued behind k_pdq_sort on its stream (the
// kernel boundary is the hand-off: no sort workgroup waits on another).  Workgroup (j, c)
// finishes part j of fanned sort fmap[c]: positions [lo - 1, hi) of the spilled store back
// into LDS at their own indices (the same dynamic LDS layout; lo - 1 is the final element
// the partitionEqual test of a frame starting at lo reads), the pending frames inside
// [lo, hi) into a frame area of its own, the step loop and the short frames on them, then
// the part's ids (or positions: `sorted`, tests) and its ready flag.
__global__ void __launch_bounds__(pdq::NT) k_pdq_sort_parts(const GroupMeta* __restrict__ groups,
                                                           const int32_t* __restrict__ pod_idx,
                                                           uint32_t* __restrict__ sorted, const uint64_t* __restrict__ gE,
                                                           const pdq::Frame* __restrict__ stack_all,
                                                           pdq::Frame* __restrict__ pstack_all, int32_t lds_n,
                                                           const int32_t* __restrict__ fmap,
                                                           int32_t* __restrict__ ids_out, int32_t* fan, int32_t ids_epoch) {
    extern __shared__ __align__(16) unsigned char pdq_dyn[];
    __shared__ pdq::Ctl ctl;
#ifdef CASIM_PROF
    const uint64_t t_p0 = clock64();
#endif
    const int gi = fmap ? fmap[blockIdx.y] : (int)blockIdx.y;
    const int j = blockIdx.x;
    int32_t* fr = fan + (size_t)gi * pdq::FAN_STRIDE;
    if (!fr[pdq::FAN_FANNED] || j >= fr[pdq::FAN_NPARTS]) return;
    const GroupMeta gm = groups[gi];
    const int32_t n = gm.count, off = gm.off;
    const int32_t lo = fr[pdq::FAN_LO + j], hi = fr[pdq::FAN_LO + j + 1];
    const int tid = threadIdx.x;
    const size_t npad = ((size_t)lds_n + 63) & ~(size_t)63;
    uint16_t* e16 = reinterpret_cast<uint16_t*>(pdq_dyn);
    uint8_t* rk = pdq_dyn + 2 * npad;
    uint64_t* rmb = reinterpret_cast<uint64_t*>(pdq_dyn + 3 * npad);
    uint16_t* rmp = reinterpret_cast<uint16_t*>(rmb + npad / 64);
    const pdq::LdsStore st{e16, rk, rmb, rmp};
    const uint32_t* spill = reinterpret_cast<const uint32_t*>(gE + off);
    for (int32_t i = max(lo - 1, 0) + tid; i < hi; i += pdq::NT) st.st(i, spill[i]);
    __syncthreads();
#ifdef CASIM_PROF
    const uint64_t t_p1 = clock64();
#endif
    pdq::Frame* stack = pstack_all + (off + lo) / 2 + 2 * (gi * pdq::FAN_PARTS_MAX + j);
    const int cap = (hi - lo) / 2 + 2;
    pdq::wg_fan_collect(stack_all + off / 2 + 2 * gi, n / 2 + 2, fr[pdq::FAN_TOP], fr[pdq::FAN_NSMALL], lo, hi, stack,
                        cap, ctl);
    pdq::wg_steps(st, n, stack, cap, (uint32_t*)nullptr, ctl, 0, 0);
#ifdef CASIM_PROF
    const uint64_t t_p2 = clock64();
#endif
    pdq::wg_short(st, stack, cap, ctl);
#ifdef CASIM_PROF
    const uint64_t t_p3 = clock64();
#endif
    if (ids_out) {
        for (int32_t k0 = lo + tid; k0 < hi; k0 += pdq::NT * PDQ_UB) {
            int32_t v[PDQ_UB];
#pragma unroll
            for (int u = 0; u < PDQ_UB; u++) { const int32_t k = k0 + u * pdq::NT; v[u] = k < hi ? pod_idx[off + (int32_t)e16[k]] : 0; }
#pragma unroll
            for (int u = 0; u < PDQ_UB; u++) { const int32_t k = k0 + u * pdq::NT; if (k < hi) ids_out[off + k] = v[u]; }
        }
    } else {
        for (int32_t k = lo + tid; k < hi; k += pdq::NT) sorted[off + k] = e16[k];
    }
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        __hip_atomic_store(&fr[pdq::FAN_FLAG + j], ids_epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
#ifdef CASIM_PROF
        const int slot = gi * pdq::FAN_PARTS_MAX + j;
        if (slot < 128 * pdq::FAN_PARTS_MAX) {
            const uint64_t t_p4 = clock64();
            unsigned long long* w = pdq::g_pdq_part + 4 * slot;
            w[0] = t_p1 - t_p0; w[1] = t_p2 - t_p1; w[2] = t_p3 - t_p2; w[3] = t_p4 - t_p3;
        }
#endif
    }
}

// Dense rank of every position of a group's list from the comparison-sorted items
// (k_score_tiles + k_merge_runs: ascending key == descending float64 score): equal scores
// share a rank.  The Go-order path for pod sets with more than CLS_MAX score classes.
__global__ void __launch_bounds__(1024) k_item_rank(const GroupMeta* __restrict__ groups,
                                                   const SortItem* __restrict__ items, uint32_t* __restrict__ item_rank) {
    __shared__ uint32_t wtot[16];
    const GroupMeta gm = groups[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t carry = 0;
    for (int32_t base = 0; base < gm.count; base += 1024) {
        const int32_t i = base + tid;
        const bool valid = i < gm.count;
        SortItem it = {};
        uint32_t f = 0;
        if (valid) {
            it = items[gm.off + i];
            f = (i > 0 && items[gm.off + i - 1].key != it.key) ? 1u : 0u;
        }
        uint32_t incl = f;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wtot[w] = incl;
        __syncthreads();
        uint32_t pre = carry, tot = carry;
        for (int q = 0; q < 16; q++) { if (q < w) pre += wtot[q]; tot += wtot[q]; }
        if (valid) item_rank[gm.off + (int32_t)it.pos] = pre + incl;
        carry = tot;
        __syncthreads();
    }
}

// stream of one group from the bucket-sorted positions (same output as k_emit_stream)
__global__ void __launch_bounds__(256) k_emit_bucket(const GroupMeta* __restrict__ groups,
                                                    const uint32_t* __restrict__ sorted,
                                                    const int32_t* __restrict__ pod_idx, const ca_template* __restrict__ tmpls,
                                                    const PodHot* __restrict__ ph, const ca_pod_spec* __restrict__ specs,
                                                    const ca_selector_term* __restrict__ terms,
                                                    const ca_selector_req* __restrict__ reqs,
                                                    StreamPod* __restrict__ out, int32_t* __restrict__ spod,
                                                    uint64_t* __restrict__ heads, uint32_t* __restrict__ group_unsup,
                                                    const int32_t* __restrict__ gmap) {
    const int gi = GSEL(blockIdx.y);
    const GroupMeta gm = groups[gi];
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    const int lane = threadIdx.x & 63;
    if ((int32_t)(blockIdx.x * blockDim.x + (threadIdx.x & ~63u)) >= gm.count) return;   // whole wave past the end
    const ca_template& tp = tmpls[gm.tmpl];
    const bool tunsched = (tp.node.flags & CA_NODE_UNSCHEDULABLE) != 0;
    const bool valid = i < gm.count;
    PodHot p = {};
    uint32_t sf = 0;
    int32_t pidx = 0;
    if (valid) {
        pidx = pod_idx[gm.off + (int32_t)sorted[gm.off + i]];
        p = ph[pidx];
        sf = static_sf(p, tp, tunsched, specs, terms, reqs);
    }
    // the previous stream entry: lane - 1, or recomputed by lane 0
    int64_t qc = __shfl_up(p.cpu, 1, 64), qm = __shfl_up(p.mem, 1, 64), qe = __shfl_up(p.eph, 1, 64);
    uint32_t qf = __shfl_up(sf, 1, 64);
    if (lane == 0 && valid && i > 0) {
        const PodHot q = ph[pod_idx[gm.off + (int32_t)sorted[gm.off + i - 1]]];
        qc = q.cpu; qm = q.mem; qe = q.eph;
        qf = static_sf(q, tp, tunsched, specs, terms, reqs);
    }
    bool head = true;
    if (valid) {
        const bool bat = batchable(p, sf);
        if (i > 0 && bat) head = !(qf == sf && qc == p.cpu && qm == p.mem && qe == p.eph);
        StreamPod sp;
        sp.cpu = p.cpu; sp.mem = p.mem; sp.eph = p.eph;
        sp.pod = pidx;
        sp.flags = sf | (head ? SF_HEAD : 0u) | (bat ? SF_BATCH : 0u);
        out[gm.off + i] = sp;
        spod[gm.off + i] = pidx;
        if (sf & SF_UNSUP) atomicOr(&group_unsup[gi], 1u);
    }
    const uint64_t hb = __ballot(head);
    if (lane == 0) heads[gm.moff + (i >> 6)] = hb;
}

// 4. the First-Fit-Decreasing chain -------------------------------------------
#ifdef CASIM_PROF   // section cycle counters of k_ffd_chain (profiling build only)
constexpr int NPROF = 24;   // + [12] loop top (window moves, head reads), [13] epilogue, [14] before the loop
// [15..16] blocks over all row passes, of the wave that sent most to the quotients: rows read,
// admitted to the float64 quotients ([17] that wave); [18..19] the row pass split: rows (with
// the wave reductions the compiler schedules ahead of the clock), cross-wave exchange;
// [20..22] an opening: the template's copy count, row writes (the generic chain: and their
// barrier), evals and segment; [23] workgroup barriers executed in the loop
__device__ unsigned long long g_chain_prof[1024][NPROF];
#define PROF_T(v) const uint64_t v = clock64()
#define PROF_ADD(i, t) prof[i] += clock64() - (t)
#define PROF_INC(i) prof[i]++
#define PROF_ADDN(i, n) prof[i] += (n)
#else
#define PROF_T(v) (void)0
#define PROF_ADD(i, t) (void)0
#define PROF_INC(i) (void)0
#define PROF_ADDN(i, n) (void)0
#endif
__device__ inline int64_t rl64(int64_t v, int lane) {
    const uint64_t u = (uint64_t)v;
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, lane);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), lane);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ inline int32_t rl32(int32_t v, int lane) { return (int32_t)__builtin_amdgcn_readlane((uint32_t)v, lane); }

// wavefront reductions (device-library DPP reductions; all 64 lanes active at every call site)
extern "C" __device__ long long __ockl_wfred_add_i64(long long);
extern "C" __device__ long long __ockl_wfred_max_i64(long long);
__device__ inline int64_t wave_max64(int64_t v) { return __ockl_wfred_max_i64(v); }
__device__ inline int32_t wave_max32(int32_t v) { return __ockl_wfred_max_i32(v); }
__device__ inline int32_t wave_min32(int32_t v) { return __ockl_wfred_min_i32(v); }
__device__ inline int64_t wave_sum64(int64_t v) { return __ockl_wfred_add_i64(v); }
__device__ inline int32_t mbcnt(uint64_t m) {
    return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The chain workgroup: CW wavefronts, one per SIMD of the CU.  Every wave runs the same
// sequential control flow on the same (uniform) state; the per-row loops over the
// group's new nodes are split across the waves in 64-row blocks (row j -> lane j mod 64
// of one wave: the generic chain deals the blocks out in contiguous ranges from the
// current row count, wave_rows; the lean chain gives block b to wave b mod CW for the
// whole kernel, chain_owner_host.h), so the row work of a run — copy counts, level
// counts, row updates, opened rows — runs on all four SIMDs; the placement list of a
// call that wants node ordinals is dealt thread by thread (rotated rank rr -> thread
// rr mod CT).  Cross-wave reductions go through LDS, double-buffered by a parity
// bit so that one barrier per reduction suffices (a wave cannot reach the next use of
// a buffer before every wave has read it: that needs the barrier in between).
// Barrier that orders LDS only.  __syncthreads() is also a workgroup fence for global
// memory, i.e. an s_waitcnt vmcnt(0) before s_barrier: every barrier would wait for the
// chain's result stores and the stream prefetch.  The waves of a chain workgroup share
// state through LDS only (their global stores are write-only results, released once at
// the end with __threadfence), so an LDS-scoped fence is all the barriers need.
__device__ inline void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// The chain's barrier: LDS-only while the rows are in LDS; a workgroup fence over every
// address space when the rows live in an HBM slab (GM), so row stores of one wave are
// visible to the others (all waves of the workgroup share the CU's L1).
template <bool GM> __device__ inline void cbar() {
    if (GM) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    } else {
        lds_barrier();
    }
}
#ifndef CASIM_CW
#define CASIM_CW 4
#endif
constexpr int CW = CASIM_CW;
constexpr int CT = 64 * CW;
constexpr int RED_N = 5;
struct ChainRed {
    int64_t v[2][CW][RED_N];
    int32_t cnt[2][CW];
    int32_t pick;          // a value one wave found, for every wave (barrier-ordered)
};
enum { R_SUM = 0, R_MAX = 1, R_MIN = 2 };
extern "C" __device__ long long __ockl_wfred_min_i64(long long);
template <int OP> __device__ inline int64_t wred(int64_t v) {
    return OP == R_SUM ? __ockl_wfred_add_i64(v) : OP == R_MAX ? __ockl_wfred_max_i64(v) : __ockl_wfred_min_i64(v);
}
template <int OP> __device__ inline int64_t wcomb(int64_t a, int64_t b) {
    return OP == R_SUM ? a + b : OP == R_MAX ? (a > b ? a : b) : (a < b ? a : b);
}
template <int OA, int OB, int OC, bool GM = false>
__device__ inline void blk_red3(ChainRed& cr, int& par, int wv, int lane, int64_t& a, int64_t& b, int64_t& c) {
    a = wred<OA>(a); b = wred<OB>(b); c = wred<OC>(c);
    if (lane == 0) { cr.v[par][wv][0] = a; cr.v[par][wv][1] = b; cr.v[par][wv][2] = c; }
    cbar<GM>();
    a = cr.v[par][0][0]; b = cr.v[par][0][1]; c = cr.v[par][0][2];
    for (int w = 1; w < CW; w++) {
        a = wcomb<OA>(a, cr.v[par][w][0]); b = wcomb<OB>(b, cr.v[par][w][1]); c = wcomb<OC>(c, cr.v[par][w][2]);
    }
    par ^= 1;
}
// Five reductions with one barrier; the waves' partial values stay readable in
// cr.v[par ^ 1] (the buffer just used) until the reduction after next.
__device__ inline int64_t wred_rt(int op, int64_t v) {
    return op == R_SUM ? wred<R_SUM>(v) : op == R_MAX ? wred<R_MAX>(v) : wred<R_MIN>(v);
}
__device__ inline int64_t wcomb_rt(int op, int64_t a, int64_t b) {
    return op == R_SUM ? a + b : op == R_MAX ? (a > b ? a : b) : (a < b ? a : b);
}
template <bool GM = false>
__device__ inline void blk_red5(ChainRed& cr, int& par, int wv, int lane, int64_t (&x)[RED_N], const int (&op)[RED_N]) {
    for (int i = 0; i < RED_N; i++) x[i] = wred_rt(op[i], x[i]);
    if (lane == 0)
        for (int i = 0; i < RED_N; i++) cr.v[par][wv][i] = x[i];
    cbar<GM>();
    for (int i = 0; i < RED_N; i++) {
        int64_t a = cr.v[par][0][i];
        for (int w = 1; w < CW; w++) a = wcomb_rt(op[i], a, cr.v[par][w][i]);
        x[i] = a;
    }
    par ^= 1;
}
// Cross-wave step only: x[] already reduced within each wave (wave-uniform).
template <bool GM = false>
__device__ inline void blk_xchg5(ChainRed& cr, int& par, int wv, int lane, int64_t (&x)[RED_N], const int (&op)[RED_N]) {
    if (lane == 0)
        for (int i = 0; i < RED_N; i++) cr.v[par][wv][i] = x[i];
    cbar<GM>();
    for (int i = 0; i < RED_N; i++) {
        int64_t a = cr.v[par][0][i];
        for (int w = 1; w < CW; w++) a = wcomb_rt(op[i], a, cr.v[par][w][i]);
        x[i] = a;
    }
    par ^= 1;
}
__device__ inline int32_t hibit(uint64_t m) { return 63 - __builtin_clzll(m); }
// lanes below `n` (n in [0, 64])
__device__ inline uint64_t lanes_below(int32_t n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : ((1ull << n) - 1); }

// Rows of the group split in contiguous 64-row-aligned ranges, one per wave, so that
// per-wave counts in wave order are counts in row order.
__device__ inline void wave_rows(int32_t k, int wv, int32_t& lo, int32_t& hi) {
    const int32_t cpw = (((k + 63) >> 6) + CW - 1) / CW;      // 64-row chunks per wave
    lo = min(k, wv * cpw * 64);
    hi = min(k, lo + cpw * 64);
}
// The lean chain's cross-wave exchange (32-bit: a run's copy sum is only used as min(S, rem)
// with rem <= 2^20, so each wave's part saturates at rem) and its per-block counts of
// qualifying rows (block b in bc[.][b]; at most 64 blocks), double-buffered like ChainRed.
struct LeanX {
    int32_t v[2][CW][RED_N + 3];      // (32 B per wave)
    int32_t bc[2][64];
};
// inclusive prefix sum across the 64 lanes (DPP row shifts, then row broadcasts 15 / 31);
// every lane active
__device__ inline int32_t lane_incl_scan(int32_t v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);     // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);     // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);     // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);     // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);     // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);     // row_bcast:31 -> rows 2, 3
    return v;
}
// LDS written by one lane of a wave and read by another lane of the same wave: the hardware
// runs a wave's LDS operations in order; this keeps the compiler from moving them across.
__device__ inline void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}
// Evals of opening n_open template copies for the rest of a run (closed form of the
// per-node sum: node i's opening pod fails FitsAnyNode over the k0+i rows before it
// (i > 0), passes CheckPredicates, and its next pi-2 pods scan k0+i+1 rows each, the
// first of them from j00 on node 0).
__device__ inline uint64_t open_evals(int32_t n_open, int32_t ct, int32_t placed2, int32_t k0, int32_t j00,
                                      uint64_t kev, bool cp_eval) {
    const uint64_t no = (uint64_t)n_open;
    uint64_t ev = kev * ((no - 1) * (uint64_t)k0 + (no - 1) * no / 2);
    if (cp_eval) ev += no;
    const uint64_t m = no - 1;                   // full nodes, ct pods each
    if (m > 0 && ct >= 2) ev += (uint64_t)(ct - 1) * (m * (uint64_t)(k0 + 1) + m * (m - 1) / 2) - (uint64_t)j00;
    const int32_t i = n_open - 1;                // the last node
    const int32_t pi = placed2 - i * ct;
    if (pi >= 2) {
        const int32_t j0i = i == 0 ? j00 : 0;
        ev += (uint64_t)(k0 + i - j0i + 1) + (uint64_t)(pi - 2) * (uint64_t)(k0 + i + 1);
    }
    return ev;
}

// Ordered compaction step over the workgroup: thread t contributes `keep` for index
// base + t; returns the thread's slot (exclusive prefix over the workgroup) and the total.
template <bool GM = false>
__device__ inline int32_t blk_compact(ChainRed& cr, int& par, int wv, bool keep, int32_t& total) {
    const uint64_t bm = __ballot(keep);
    if ((threadIdx.x & 63) == 0) cr.cnt[par][wv] = __builtin_popcountll(bm);
    cbar<GM>();
    int32_t before = 0;
    total = 0;
    for (int w = 0; w < CW; w++) {
        const int32_t c = cr.cnt[par][w];
        before += w < wv ? c : 0;
        total += c;
    }
    par ^= 1;
    return before + mbcnt(bm);
}

// New-node row in LDS: free resources of one template copy (32 B, two ds_read_b128).
struct alignas(16) NodeRec {
    int64_t cpu, mem, eph;
    int32_t pods;      // free pod slots
    int32_t used;      // newNodesWithPods membership
};
static_assert(sizeof(NodeRec) == 32, "NodeRec");

// NodeResourcesFit on a row (fit.go:256-300), branch-free so all loads issue together.
__device__ inline bool rec_fits(const NodeRec& r, int64_t pcpu, int64_t pmem, int64_t peph, bool zero) {
    const bool res = (pcpu <= r.cpu) & (pmem <= r.mem) & (peph <= r.eph);
    return (r.pods >= 1) & (zero | res);
}

// How many copies of a resource-only pod (requests >= 0) fit a row one after another:
// copy m+1 fits iff pods >= m+1 and (all-zero or every req <= free - m*req), so the
// count is min(pods, floor(free/req)) over the requested dimensions (fit.go:256-300;
// a zero request passes iff free >= 0).  Capped at `cap`.
__device__ inline int32_t dim_copies(int64_t free_, int64_t req, int32_t cap) {
    if (free_ < 0) return 0;
    if (req == 0) return cap;
    if (free_ < req) return 0;
    // floor(free/req) capped at cap, without a 64-bit integer division: the float64
    // quotient is within one of the exact one once capped, and one step each way fixes it.
    const double qd = (double)free_ / (double)req;
    uint64_t q = qd >= (double)cap ? (uint64_t)cap : (uint64_t)qd;
    const uint64_t f = (uint64_t)free_, r = (uint64_t)req;     // both < 2^63: no wrap below
    if (q * r > f) q--;
    else if (q < (uint64_t)cap && (q + 1) * r <= f) q++;
    return (int32_t)q;
}
__device__ inline int32_t rec_copies(const NodeRec& r, int64_t pcpu, int64_t pmem, int64_t peph, bool zero, int32_t cap) {
    int32_t c = r.pods < cap ? r.pods : cap;
    if (c <= 0) return 0;
    if (!zero) {
        c = min(c, dim_copies(r.cpu, pcpu, c));
        c = min(c, dim_copies(r.mem, pmem, c));
        c = min(c, dim_copies(r.eph, peph, c));
    }
    return c;
}

// rec_copies for the rows of one run: the pod's requests and reciprocals in float64,
// computed once per run.  Exact while every free value and request is below 2^53 (a
// template copy's free values bound every row of its group; checked once per run);
// otherwise the exact integer rec_copies.
struct RunDiv {
    double reqd[3], rcpd[3];
    bool f64;
};
__device__ inline RunDiv run_div(int64_t pcpu, int64_t pmem, int64_t peph, int64_t bound) {
    RunDiv d;
    constexpr int64_t E53 = 1ll << 53;
    d.f64 = bound < E53 && pcpu < E53 && pmem < E53 && peph < E53;
    const int64_t req[3] = {pcpu, pmem, peph};
    for (int i = 0; i < 3; i++) {
        d.reqd[i] = run_req(req[i]);
        d.rcpd[i] = run_rcp(req[i]);
    }
    return d;
}
// floor(free/req) capped at cap with full-rate float64 ops only: below 2^53 the
// conversions are exact, the quotient is within one of the exact floor, and
// fma(-q, req, free) = free - q*req is an integer below 2^53 in magnitude, so it is
// computed exactly and one step each way makes q exact (no 64-bit integer multiply).
__device__ inline int32_t dim_copies_f64(int64_t free_, double rd, double rcpd, int32_t cap) {
    return co_dim_copies_f64(free_, rd, rcpd, cap);     // (chain_owner_host.h: checked on the host)
}
// SREQ: the zero-request tests read the scalar integer requests (the lean chain's float64
// values come from LDS in vector registers; the test is the same one)
template <bool SREQ = false>
__device__ inline int32_t rec_copies_run(const NodeRec& r, const RunDiv& d, bool zero, int32_t cap,
                                         int64_t pcpu, int64_t pmem, int64_t peph) {
    if (!d.f64) return rec_copies(r, pcpu, pmem, peph, zero, cap);     // uniform
    int32_t c = max(0, min(r.pods, cap));
    if (!zero) {     // uniform
        // independent per-dimension quotients (capped at the same c, min taken after);
        // a zero request only needs free >= 0 (uniform skip of the division)
        const int32_t cp = max(c, 1);
        const bool n0 = SREQ ? pcpu != 0 : d.reqd[0] != 0.0, n1 = SREQ ? pmem != 0 : d.reqd[1] != 0.0,
                   n2 = SREQ ? peph != 0 : d.reqd[2] != 0.0;
        const int32_t q0 = n0 ? dim_copies_f64(r.cpu, d.reqd[0], d.rcpd[0], cp) : (r.cpu < 0 ? 0 : cp);
        const int32_t q1 = n1 ? dim_copies_f64(r.mem, d.reqd[1], d.rcpd[1], cp) : (r.mem < 0 ? 0 : cp);
        const int32_t q2 = n2 ? dim_copies_f64(r.eph, d.reqd[2], d.rcpd[2], cp) : (r.eph < 0 ? 0 : cp);
        c = min(c, min(q0, min(q1, q2)));
    }
    return c;
}

// first run head strictly after `pos` (positions >= P count as heads)
__device__ inline int32_t run_end(const uint64_t* __restrict__ hm, int32_t pos, int32_t P, int lane) {
    int32_t c = pos >> 6;
    const int32_t nc = (P + 63) >> 6;
    const int sh = (pos & 63) + 1;
    uint64_t m = hm[c];
    m = sh >= 64 ? 0ull : (m >> sh) << sh;
    if (m) return min(P, (c << 6) + __builtin_ctzll(m));
    for (c = c + 1; c < nc; c += 64) {
        const int32_t cc = c + lane;
        const uint64_t v = cc < nc ? hm[cc] : 0ull;
        const uint64_t b = __ballot(v != 0);
        if (b) {
            const int l = __builtin_ctzll(b);
            return min(P, ((c + l) << 6) + __builtin_ctzll((uint64_t)rl64((int64_t)v, l)));
        }
    }
    return P;
}
// run_end with the head words [pf_c, pf_c + 64) already in registers (lane l holds word
// pf_c + l, 0 past the end; loaded when the previous run started), so finding a run's
// end costs no global round trip unless the run is longer than the 4096 positions held.
__device__ inline int32_t run_end_pf(const uint64_t* __restrict__ hm, int32_t pos, int32_t P, int lane,
                                     int32_t pf_c, uint64_t pf_w) {
    const int32_t c = pos >> 6;
    if (c != pf_c) return run_end(hm, pos, P, lane);
    const int sh = (pos & 63) + 1;
    uint64_t m = (uint64_t)rl64((int64_t)pf_w, 0);
    m = sh >= 64 ? 0ull : (m >> sh) << sh;
    if (m) return min(P, (c << 6) + __builtin_ctzll(m));
    const uint64_t b = __ballot((lane > 0) & (pf_w != 0ull));
    if (b) {
        const int l = __builtin_ctzll(b);
        return min(P, ((c + l) << 6) + __builtin_ctzll((uint64_t)rl64((int64_t)pf_w, l)));
    }
    const int32_t nc = (P + 63) >> 6;
    for (int32_t c2 = c + 64; c2 < nc; c2 += 64) {
        const int32_t cc = c2 + lane;
        const uint64_t v = cc < nc ? hm[cc] : 0ull;
        const uint64_t b2 = __ballot(v != 0);
        if (b2) {
            const int l = __builtin_ctzll(b2);
            return min(P, ((c2 + l) << 6) + __builtin_ctzll((uint64_t)rl64((int64_t)v, l)));
        }
    }
    return P;
}

// Zero-copy results (page-locked sched_pod, no node ordinals): a group hands its output
// range to k_publish in pch-sized chunks ("tickets") as soon as each chunk is final —
// every output of [c*pch, (c+1)*pch) is scheduled — and the rest when it ends, so the
// results cross PCIe while the chains still run, the long ones included.  Each ticket
// carries the group's progress (segments written, pods scheduled) at its push.
// Release at agent scope: the L2s of the 8 XCDs are not coherent, the publisher may run
// on another XCD.  Called by one whole wavefront (the one that stores the results).
//
// A ticket is 64-bit: the chunk (g * nsub + c) in the low word and, for a **pure** chunk —
// every output of it comes from run segments with one stream offset `off` (output i is
// stream position i + off) — off + 1 in the high word.  The publisher copies a pure chunk
// from the stream's pod ids (written before the chains started) and reads nothing the
// chain wrote, so its push needs no release: an agent-scope release writes the XCD's L2
// back (gfx950: its L2 is not coherent with the other XCDs'), microseconds per push on the
// chain's critical path.  Other chunks (single placements, a segment boundary with another
// offset, the group's tail) go with the release and the progress record.
constexpr int PCH = 4096;      // default chunk (CASIM_PUB_CHUNK overrides, for tests)
#ifndef CASIM_PCH_DECOUPLED
#define CASIM_PCH_DECOUPLED 16384
#endif
constexpr int PCH_DECOUPLED = CASIM_PCH_DECOUPLED;   // ... with the decoupled Go order (scripts/gpu_pubsweep2.sh)
__device__ inline void push_chunks(int32_t g, int32_t c0, int32_t c1, int32_t nsub, int64_t* tickets, int32_t* qctl,
                                   int2* prog, int32_t nseg, int32_t nsched, int lane, int32_t pch = 0,
                                   int32_t pure_from = INT32_MAX, int32_t pure_off = 0) {
    if (c1 <= c0) return;
    const bool pure = pch > 0 && (int64_t)c0 * pch >= pure_from;
    if (!pure) __threadfence();
    if (lane == 0) {
        if (!pure)
            for (int32_t c = c0; c < c1; c++) prog[g * nsub + c] = make_int2(nseg, nsched);
        const int32_t base = atomicAdd(&qctl[1], c1 - c0);
        const int64_t hi = pure ? ((int64_t)pure_off + 1) << 32 : 0;
        for (int32_t i = 0; i < c1 - c0; i++) {
            const int64_t v = hi | (int64_t)(uint32_t)(g * nsub + c0 + i);
            if (pure) __hip_atomic_store(&tickets[base + i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else __hip_atomic_store(&tickets[base + i], v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Data the chains write while the publisher runs (progress records, segments) is read
// with device-coherent loads: a uniform plain load may be served from the scalar cache,
// which the acquire does not invalidate, so a line cached for an earlier chunk (or a
// neighbouring group) could hand back entries written after it was filled.
__device__ inline int32_t ld_coh(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline Seg ld_seg(const Seg* p) {
    const int32_t* q = reinterpret_cast<const int32_t*>(p);
    Seg sg;
    sg.dst = ld_coh(q); sg.src = ld_coh(q + 1); sg.len = ld_coh(q + 2); sg.pad = 0;
    return sg;
}

// Publisher (second stream, concurrent with k_ffd_chain): block b claims the next ticket
// in completion order, waits for it, and writes outputs [sub*pch, +pch) of its group
// into the caller's page-locked buffer: single placements from the chain's sched_pod,
// run placements from the stream via the group's segments, -1 past n_scheduled.
// Every block exits once all `total` tickets are claimed.  HIP does not promise that the
// two kernels overlap, so the publisher never waits on a chain that has not started:
// the chains raise qctl[4] when they begin, and a publisher that sees no chain within
// `start_ticks` (100 MHz wall clock; the kernels were serialised) sets qctl[2] and ends,
// as does one whose ticket is not pushed within 200 ms of a started chain (a chain that
// died).  qctl[2] sends the host to the stream-ordered copy (k_copy_segments + D2H).
// T = int32_t: pod ids; T = uint16_t: pod ids of a podset of at most 65535 pods, 0xFFFF for
// "not scheduled" (ca_estimate_plan_run_u16: half the bytes over PCIe).

// first segment of gs[0, nseg) that ends after `key` (from_dst false) or starts at or after
// it (true); segments are in output order.  One wavefront probes 64 evenly spaced segments
// per step with coherent loads in flight together, so a search is one or two round trips
// to L2 instead of one per bisection step.
__device__ inline int32_t seg_lower(const Seg* gs, int32_t nseg, int32_t key, bool from_dst, int lane) {
    int32_t lo = 0, hi = nseg;                     // answer in [lo, hi]
    while (hi - lo > 0) {
        const int32_t span = hi - lo;
        const int32_t step = (span + 63) / 64;
        const int32_t i = lo + lane * step;
        bool past = false;
        if (i < hi) {
            const int32_t* q3 = reinterpret_cast<const int32_t*>(gs + i);
            past = from_dst ? ld_coh(q3) >= key : ld_coh(q3) + ld_coh(q3 + 2) > key;
        }
        const uint64_t m = __ballot(past);
        const int32_t f = m ? (int32_t)__builtin_ctzll(m) : -1;    // first probe past the key
        if (step == 1) { lo = f >= 0 ? lo + f : hi; break; }
        const int32_t nlo = f > 0 ? lo + (f - 1) * step + 1 : (f == 0 ? lo : lo + ((span - 1) / step) * step + 1);
        hi = f >= 0 ? lo + f * step : hi;
        lo = nlo;
    }
    return lo;
}
__device__ inline int32_t bc32(int32_t v) { return (int32_t)__builtin_amdgcn_readfirstlane((uint32_t)v); }
__device__ inline int64_t bc64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// (the helpers below read a whole fan record with one load per wavefront and index it by lane)
static_assert(pdq::FAN_STRIDE <= 64 && pdq::FAN_FLAG == 0 && pdq::FAN_PARTS_MAX <= 32, "fan record: one word per lane, flags first");
static_assert(pdq::FAN_LO + pdq::FAN_PARTS_MAX < pdq::FAN_STRIDE && pdq::FAN_BOUNDS < pdq::FAN_STRIDE &&
              pdq::FAN_NPARTS < pdq::FAN_STRIDE, "fan record: bounds inside the loaded words");
// a sort's fan record (pdq::FAN_STRIDE words), word `lane` in each lane
__device__ inline int32_t fan_load(const int32_t* fr, int lane) {
    return lane < pdq::FAN_STRIDE ? ld_coh(fr + lane) : 0;
}
// the parts of a sort that overlap Go-order positions [s0, s1), from a record whose bounds are final
__device__ inline uint32_t fan_need(int32_t v, int lane, int32_t s0, int32_t s1) {
    const int32_t np = min(rl32(v, pdq::FAN_NPARTS), (int32_t)pdq::FAN_PARTS_MAX);
    const int32_t lo0 = __shfl(v, min(pdq::FAN_LO + lane, 63)), lo1 = __shfl(v, min(pdq::FAN_LO + lane + 1, 63));
    return (uint32_t)__ballot(lane < np && lo0 < s1 && lo1 > s0);
}
__device__ inline uint32_t fan_up(int32_t v, int lane, int32_t epoch) {
    return (uint32_t)__ballot(lane < pdq::FAN_PARTS_MAX && v == epoch);
}

template <typename T>
__global__ void __launch_bounds__(256) k_publish(const GroupMeta* __restrict__ groups, const ChainOut* __restrict__ outs,
                                                const Seg* __restrict__ segs, const int32_t* __restrict__ spod,
                                                const int32_t* sched_dev, int64_t* __restrict__ tickets,
                                                int32_t* __restrict__ qctl, int32_t total, int32_t nsub,
                                                const int2* __restrict__ prog, int32_t pch,
                                                T* pub,              // pub may alias sched_dev (device results)
                                                uint64_t start_ticks, const int32_t* ids_ready, int32_t ids_epoch,
                                                int32_t* __restrict__ hflags, int32_t ids_final) {
    // ids_ready != null (decoupled Go order): the stream's pod ids in spod
    // come from a sort that runs beside the chains — the fan record of the group whose sort
    // wrote them (the group's own, or the representative of its sort class) flags each part
    // of the Go order with this run's epoch once its ids are final — and the chains' single
    // placements are stream positions.  A ticket reads Go-order positions [s0, s1) of that
    // sort and waits for the parts that overlap them:
    //   a pure chunk          its own slice;
    //   a segment ticket      from the first to the last position its segments read — the
    //                         chain walks the stream forwards, so the first and the last
    //                         segment that overlap the chunk bound them;
    //   a group with single   every part: a single placement indexes any position (the
    //   steps so far          chain sets the sign bit of the progress record's nseg).
    // The bounds are final once FAN_BOUNDS holds this run's epoch; a flag seen up stays up.
    // Wave 0 is the block's controller (the other waves sleep at the barrier): it claims the
    // ticket, waits for its push, finds its positions and polls the sort's fan record — 40
    // words, one load — until the parts it needs are up.
    // ids_final: the ids were sorted by an earlier run of the plan (or at its creation) and the
    // host has seen that sort finished — no ticket looks up its positions or loads a fan record.
    const bool wait_ids = ids_ready && !ids_final;
    __shared__ int32_t s_seg0;
    __shared__ int64_t s_tk;
    __shared__ Seg s_segs[64];
    const int lane = (int)threadIdx.x & 63;
    bool gave_up = false;                      // (wave 0)
    for (;;) {
        if (threadIdx.x < 64) {
            int64_t tk = -1;
            int32_t seg0 = 0, t = 0;
            if (lane == 0) t = atomicAdd(&qctl[0], 1);
            t = bc32(t);
            if (t < total) {
                const uint64_t t0 = wall_clock64();
                bool started = false;
                for (;;) {
                    // relaxed polls (an acquire per poll invalidates caches other kernels on
                    // the XCD are using); the acquire comes once, when the ticket is there
                    tk = bc64(__hip_atomic_load(&tickets[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                    if (tk >= 0) {      // consumed: the slot is -1 again for the next run
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        if (lane == 0) __hip_atomic_store(&tickets[t], -1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                    if (bc32(__hip_atomic_load(&qctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) { gave_up = true; break; }
                    if (!started) started = bc32(__hip_atomic_load(&qctl[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0;
                    const uint64_t dt = wall_clock64() - t0;
                    if ((!started && dt > start_ticks) || dt > 20000000ull) {               // 200 ms
                        if (lane == 0) __hip_atomic_store(&qctl[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        gave_up = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                if (tk >= 0) {
                    const int32_t tkid = (int32_t)(uint32_t)(tk & 0xFFFFFFFFll);
                    const int32_t g0 = tkid / nsub;
                    const int32_t a = (tkid - g0 * nsub) * pch, b = min(groups[g0].count, a + pch);
                    const int32_t po = (int32_t)(tk >> 32) - 1;
                    int32_t s0 = 0, s1 = INT32_MAX;
                    if (po >= 0) {
                        s0 = po + a;
                        s1 = po + b;
                    } else {
                        const int32_t* pr = reinterpret_cast<const int32_t*>(prog + tkid);   // progress at the push
                        const int32_t nsw = bc32(ld_coh(pr));
                        const int32_t end = min(b, bc32(ld_coh(pr + 1)));
                        const int32_t nseg = nsw & INT32_MAX;
                        const Seg* gs = segs + groups[g0].off;
                        seg0 = seg_lower(gs, nseg, a, false, lane);
                        if (wait_ids && nsw >= 0) {
                            if (end <= a) {
                                s0 = s1 = 0;                         // the -1 tail alone: no ids
                            } else {
                                const int32_t q1 = seg_lower(gs, nseg, end, true, lane);
                                if (seg0 < q1) {
                                    const Seg f = ld_seg(gs + seg0), l = ld_seg(gs + q1 - 1);
                                    s0 = bc32(f.src - f.dst + max(a, f.dst));
                                    s1 = bc32(l.src - l.dst + min(end, l.dst + l.len));
                                }
                            }
                        }
                    }
                    if (wait_ids && s0 < s1) {
                        const int32_t* fr = ids_ready + (size_t)groups[g0].ids_grp * pdq::FAN_STRIDE;
                        bool bounds = false;
                        uint32_t need = 0;
                        for (;;) {
                            int32_t v = fan_load(fr, lane);
                            if (!bounds && rl32(v, pdq::FAN_BOUNDS) == ids_epoch) {
                                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                                v = fan_load(fr, lane);                  // (the bounds, read behind the acquire)
                                need = fan_need(v, lane, s0, s1);
                                bounds = true;
                            }
                            if (bounds && (need & ~fan_up(v, lane, ids_epoch)) == 0) {
                                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                                break;
                            }
                            if (bc32(__hip_atomic_load(&qctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                                gave_up = true;
                                tk = -1;
                                break;
                            }
                            if (wall_clock64() - t0 > 20000000ull) {                            // 200 ms
                                if (lane == 0) __hip_atomic_store(&qctl[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                gave_up = true;
                                tk = -1;
                                break;
                            }
                            __builtin_amdgcn_s_sleep(2);
                        }
                    }
                }
            }
            if (lane == 0) { s_tk = tk; s_seg0 = seg0; }
        }
        lds_barrier();
        const int64_t tk64 = s_tk;
        if (tk64 < 0) {
            if (threadIdx.x == 0) {
                // gave up (qctl[2]): tell the host, which reads hflags after the round (no copy)
                if (gave_up) hflags[2] = 1;
                // the last block out clears the control words for the next run (every ticket
                // was consumed, so no chain pushes any more; after a give-up the host
                // re-initialises them)
                if (atomicAdd(&qctl[5], 1) == (int32_t)gridDim.x - 1)
                    for (int k = 0; k < 6; k++) __hip_atomic_store(&qctl[k], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
        __threadfence();                                   // acquire for every thread of the block
        const int32_t tk = (int32_t)(uint32_t)(tk64 & 0xFFFFFFFFll);
        const int32_t pure_off = (int32_t)(tk64 >> 32) - 1;   // >= 0: a pure chunk (push_chunks)
        const int32_t g = tk / nsub, sub = tk - g * nsub;
        const GroupMeta gm = groups[g];
        const Seg* gs = segs + gm.off;
        const int32_t soff = ids_ready ? gm.ids_off : gm.off;       // the group's pod ids in spod
        const int32_t a = sub * pch, b = min(gm.count, a + pch);
        if (pure_off >= 0) {
            // one contiguous copy: 16-byte stores into the page-locked buffer (fewer, fuller
            // PCIe writes), scalar stores for the unaligned head and tail
            constexpr int V = 16 / (int)sizeof(T);
            T* const dst = pub + gm.off;
            const int32_t* const src = spod + soff + pure_off;
            int32_t h = a;
            while (h < b && ((uintptr_t)(dst + h) & 15u)) h++;                 // aligned from h on
            const int32_t nv = (b - h) / V;
            for (int32_t i = a + (int32_t)threadIdx.x; i < h; i += blockDim.x) dst[i] = (T)src[i];
            for (int32_t v = (int32_t)threadIdx.x; v < nv; v += blockDim.x) {
                const int32_t i0 = h + v * V;
                T w[V];
#pragma unroll
                for (int u = 0; u < V; u++) w[u] = (T)src[i0 + u];
                uint4 q;
                __builtin_memcpy(&q, w, 16);
                *reinterpret_cast<uint4*>(dst + i0) = q;
            }
            for (int32_t i = h + nv * V + (int32_t)threadIdx.x; i < b; i += blockDim.x) dst[i] = (T)src[i];
            lds_barrier();
            continue;
        }
        const int32_t* pr = reinterpret_cast<const int32_t*>(prog + tk);   // the group's progress at the push
        const int32_t nseg = ld_coh(pr) & INT32_MAX;       // (sign bit: the group made single steps)
        const int32_t ns = ld_coh(pr + 1);
        int32_t at = a, q = s_seg0;
        const int32_t end = min(b, ns);
        int32_t q0 = 0, qn = 0;                           // segments [q0, q0 + qn) cached in LDS
        while (at < end) {
            int32_t lim = end, src_off = 0;
            bool from_seg = false;
            if (q < nseg && (q < q0 || q >= q0 + qn)) {
                // the next 64 segments, loaded together (one round trip instead of one per segment)
                lds_barrier();                             // every thread is done with the old ones
                if (threadIdx.x < 64 && q + (int32_t)threadIdx.x < nseg) s_segs[threadIdx.x] = ld_seg(gs + q + threadIdx.x);
                q0 = q;
                qn = min(64, nseg - q);
                lds_barrier();
            }
            if (q < nseg) {
                const Seg sg = s_segs[q - q0];
                if (sg.dst <= at) {                            // inside segment q
                    from_seg = true;
                    src_off = sg.src - sg.dst;
                    lim = min(end, sg.dst + sg.len);
                    q++;
                } else {
                    lim = min(end, sg.dst);                    // single placements before it
                }
            }
            for (int32_t i = at + (int32_t)threadIdx.x; i < lim; i += blockDim.x)
                pub[gm.off + i] = (T)(from_seg ? spod[soff + src_off + i]
                                               : ids_ready ? spod[soff + ld_coh(sched_dev + gm.off + i)]
                                                           : sched_dev[gm.off + i]);
            at = lim;
        }
        for (int32_t i = max(a, ns) + (int32_t)threadIdx.x; i < b; i += blockDim.x) pub[gm.off + i] = (T)-1;
        lds_barrier();
    }
}

// One workgroup of CW (4) waves per node group (see ChainRed above: the waves share the
// row loops, the control flow is uniform).  LDS: NodeRec rows[kcap], block summaries[kcap/64]
// (per-dimension maxima over a 64-row block, allowed to be stale-high), the per-run
// scratch CAPA/ALIVE[kcap], and the optional port / scalar columns.
//
// The sequential loop of binpacking_estimator.go:86-141 runs pod by pod, except that a
// run of identical resource-only pods (SF_BATCH) is placed in closed form: the rotating
// first fit of schedulerbased.go:114-131 with identical pods visits the nodes that still
// have room in rotated order, one pod per node per revolution, so revolution r serves
// the nodes with c_j >= r copies left, and the run costs O(k/64) wave steps plus one
// step per node it opens instead of one k-node scan per pod.  Evals are exact: the t-th
// placement's scan ends at unwrapped position (rev-1)*k + rank, so a batch costs
// (r_last-1)*k + rank(last)+1 filter calls.  assign[pos] receives the new-node index of
// every placed stream position (-1 = not scheduled).
// PS: the batch has pods with host ports or extended-resource requests (their columns and
// checks compile out of the common instantiation)
// TB: the run-table chain (decoupled stream from per-class counts, run batching on).  The
// stable order is the group's classes in rank order and every pod of a class is the same
// record, so k_run_table's rows rstart[g][0..U] / rsp[g][0..U) are the whole stream: the
// prologue copies them to LDS (at byte tab_off of the dynamic LDS, behind the rows) and
// lists the ranks that start a run — present ranks, adjacent batchable ranks of equal
// record merged under k_emit_runs' SF_HEAD rule — and the loop walks that list: a run's
// record, first position and end come from LDS, `stream` and `heads` are never read and
// the loop issues no global load (k_emit_runs is not launched).  A non-batchable rank is a
// run of `count` single pods of one record.
// LEAN (with TB, rows in LDS, no PS): the headline's case — no node ordinals wanted, every
// group of at most 2^20 pods, every template free value and request below 2^53 (a plan
// fact).  Such a call never takes the integer rec_copies path, the rem > 2^20 path or the
// placement list, so they are not instantiated, and a run's float64 requests and reciprocals
// come from the table (rdiv, k_run_table) instead of three divisions and the conversions at
// its entry, as does the copy count of its pod on a fresh template copy.  Its runs have a body
// of their own: every 64-row block belongs to one wave for the whole kernel, so a run costs
// one barrier (the exchange) where the generic body needs two (the invariants: at its top).
// Every other call runs the generic instantiations, the in-tree reference of the lean one
// (CASIM_LEAN_CHAIN=0).
template <bool GROWS, bool PS, bool TB, bool LEAN = false>
__global__ void __launch_bounds__(CT) k_ffd_chain(
    const GroupMeta* __restrict__ groups, const StreamPod* __restrict__ stream, const uint64_t* __restrict__ heads,
    const ca_template* __restrict__ tmpls, const ca_pod_spec* __restrict__ specs, const PodHot* __restrict__ ph,
    const int32_t* __restrict__ lin_arr, const uint8_t* __restrict__ need, const uint32_t* __restrict__ group_unsup,
    int32_t n_base, int32_t max_nodes, int32_t kcap, int32_t use_ports, int32_t use_scalar, int32_t batch_runs,
    int32_t* __restrict__ sched_pod, int32_t* __restrict__ sched_node, Seg* __restrict__ segs,
    int64_t* __restrict__ tickets, int32_t* __restrict__ qctl, int32_t nsub, int2* __restrict__ prog, int32_t pch,
    ChainOut* __restrict__ outs, const int32_t* __restrict__ gmap, unsigned char* __restrict__ gslab,
    const int64_t* __restrict__ slab_off, const int32_t* __restrict__ gkcap, int32_t pos_out,
    ChainOut* __restrict__ hout, int32_t* __restrict__ hflags, const int32_t* __restrict__ rstart,
    const StreamPod* __restrict__ rsp, int32_t U, int32_t tab_off, const double* __restrict__ rdiv) {
    static_assert(!LEAN || (TB && !GROWS && !PS), "the lean chain: run table, rows in LDS, no ports or scalars");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int g = GSEL(blockIdx.x);
    // GROWS: the group's rows live in its own HBM slab (kcap = the group's pod count, for an
    // unlimited estimate too large for LDS); else in LDS with the batch-wide kcap
    if (GROWS) kcap = gkcap[g];
    unsigned char* const row_base = GROWS ? gslab + slab_off[g] : smem_raw;
    // TB: the group's rank starts, requested first so they arrive with the group's record
    const int32_t* const t_rs = TB ? rstart + (size_t)g * (U + 1) : nullptr;
    int32_t t_a0 = 0, t_b0 = 0;
    if (TB && (int32_t)threadIdx.x < U) { t_a0 = t_rs[threadIdx.x]; t_b0 = t_rs[threadIdx.x + 1]; }
    if (!need[g]) return;
    if (tickets && threadIdx.x == 0)              // a publisher may wait on this batch now
        __hip_atomic_store(&qctl[4], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t t_begin = wall_clock64();      // diagnostics: ca_estimate_plan_group_ticks
    __builtin_amdgcn_s_setprio(3);                // the chain is the critical path: win issue over k_publish
#ifdef CASIM_PROF
    const uint64_t t_cyc0 = clock64();
#endif
    uint32_t n_single = 0;
#ifdef CASIM_PROF
    uint64_t prof[NPROF] = {};
#endif
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;          // wave of the workgroup
    const bool w0 = wv == 0;          // the wave that stores single-pod results
    __shared__ ChainRed cred;
    __shared__ LeanX lx;              // (the lean chain's exchange; unused and dropped elsewhere)
    int par = 0;
    const GroupMeta gm = groups[g];
    const int32_t lin = lin_arr[g];
    ChainOut res;
    res.node_count = 0; res.n_sched = 0; res.nodes_added = 0; res.lin = lin; res.lout = lin;
    res.status = CA_OK; res.sensitive = 0; res.had_success = 0; res.evals = 0; res.pad = 0;
    res.nseg = 0; res.pad2[0] = res.pad2[1] = res.pad2[2] = 0;
    if (group_unsup[g] || (gm.tflags & CA_NODE_ANTI_AFFINITY_PODS)) {
        res.status = CA_EUNSUPPORTED;
        if (tid == 0) { outs[g] = res; hout[g] = res; }
        if (tickets && w0) push_chunks(g, 0, (gm.count + pch - 1) / pch, nsub, tickets, qctl, prog, 0, 0, lane);
        return;
    }
    const int nb_cap = (kcap + 63) >> 6;
    NodeRec* R = reinterpret_cast<NodeRec*>(row_base);
    NodeRec* SUM = R + kcap;
    int32_t* CAPA = reinterpret_cast<int32_t*>(SUM + nb_cap);                   // [kcap]
    int32_t* ALIVE = CAPA + kcap;                                               // [kcap]
    uint64_t* PORTS = reinterpret_cast<uint64_t*>(ALIVE + kcap);                // [kcap][CA_PORT_WORDS]
    int64_t* SC = reinterpret_cast<int64_t*>(PORTS + (use_ports ? (size_t)CA_PORT_WORDS * kcap : 0));
    if (!PS) use_ports = use_scalar = 0;  // [8][kcap]

    const ca_template& tp = tmpls[gm.tmpl];
    NodeRec trec;                 // a fresh template copy
    trec.cpu = gm.tcpu; trec.mem = gm.tmem; trec.eph = gm.teph; trec.pods = gm.tpods; trec.used = 0;

    int32_t k = 0;              // new nodes so far
    int32_t granted = 0;        // limiter.nodes
    int32_t last_node = -1;     // lastNodeName
    // LEAN: R[last_node].used in a uniform register (known at every opening, derived from the
    // copy counts at every placement), the kind of the previous step (1 a run, 2 one pod: a
    // barrier separates the two), and the parities of the exchange buffers and of CAPA / ALIVE
    bool l_used = false;
    int prev_step = 0, lpar = 0, lcap = 0;
    int32_t L = lin;            // the checker's lastIndex
    int32_t nsched = 0;
    uint64_t evals = 0;
    bool first_success = false, sensitive = false;

    const int32_t P = gm.count;
    const StreamPod* gs = stream + gm.off;
    const uint64_t* hm = heads + gm.moff;
    // outputs in processing order (binpacking_estimator.go:143): the i-th scheduled pod of
    // the group and its new-node ordinal go to index i; placements happen in stream order
    Seg* gseg = segs + gm.off;
    int32_t nseg = 0;
    int32_t* so_pod = sched_pod + gm.off;
    int32_t* const so_node = (!LEAN && sched_node) ? sched_node + gm.off : nullptr;
    // Stream double buffer: lane l holds entry (wbase + l) in `cur` and (wbase + 64 + l)
    // in `nxt`.  Single-pod placements are kept in the lane of their stream position and
    // stored when the window moves on, so no step waits on a store (vmcnt counts both).
    int32_t wbase = 0;
    StreamPod cur = {}, nxt = {};
    if (!TB) {
        if (lane < P) cur = gs[lane];
        if (64 + lane < P) nxt = gs[64 + lane];
    }
    int32_t out_node = -1, out_idx = 0;
    bool pend = false;
    bool stop = false;
    // Prefetch for the next run head, issued when a run starts: the stream window at the
    // run's end (pf_base, -1 none) and the head words from there (pf_hc, lane l holds word
    // pf_hc + l), so the global latency overlaps the run's LDS work instead of following it.
    int32_t pf_base = -1, pf_hc = -1;
    StreamPod pf_cur = {}, pf_nxt = {};
    uint64_t pf_hw = 0;
    const int32_t nhc = (P + 63) >> 6;
    // TB: the group's table in LDS — TREC[r] the record of rank r (present ranks only),
    // TST[r] its first position (TST[U] = P), TRUN[i] = (the rank that starts run i, its
    // first position); TRUN[n_runs] = (0, P): a run ends where the next one starts.  The
    // loop keeps the next run's record (t_nrec) and the entry after it (t_npair: the next
    // run's end, the rank of the run after) in registers, read from LDS when the run before
    // started, so taking a run waits for nothing.
    // LEAN: TDIV[r] behind TREC — the rank's three requests and their reciprocals in float64
    // (48 B), kept in registers one run ahead like the record (t_ndiv), and TRCT[r] behind TST:
    // the copies of the rank's pod on a fresh template copy (k_run_table's rdiv[.][6]; t_nct).
    struct RankDiv { double v[6]; };
    StreamPod* const TREC = reinterpret_cast<StreamPod*>(smem_raw + tab_off);
    RankDiv* const TDIV = reinterpret_cast<RankDiv*>(TREC + (TB ? U : 0));
    int2* const TRUN = reinterpret_cast<int2*>(TDIV + (LEAN ? U : 0));
    int32_t* const TST = reinterpret_cast<int32_t*>(TRUN + (TB ? U + 1 : 0));
    int32_t* const TRCT = TST + (TB ? U + 1 : 0);
    int32_t t_next = 0, t_end = 0, n_runs = 0;     // the next run of the list; the current run's end
    StreamPod t_nrec = {};
    RankDiv t_ndiv = {}, t_div = {};
    int32_t t_nct = 0, t_ct = 0;
    int2 t_npair = make_int2(0, 0);
    if (TB) {
        const StreamPod* rp = rsp + (size_t)g * U;
        const double* dp = LEAN ? rdiv + (size_t)g * U * RDIV_N : nullptr;
        for (int32_t r = tid; r < U; r += CT) {
            // (the first CT ranks' starts were requested at the kernel's entry)
            const int32_t a = r < CT ? t_a0 : t_rs[r], b = r < CT ? t_b0 : t_rs[r + 1];
            TST[r] = a;
            if (b > a) TREC[r] = rp[r];        // (an absent rank's record was never written)
            if (LEAN && b > a) {
                RankDiv dr;
                for (int i = 0; i < 6; i++) dr.v[i] = dp[(size_t)r * RDIV_N + i];
                TDIV[r] = dr;
                TRCT[r] = (int32_t)dp[(size_t)r * RDIV_N + 6];
            }
        }
        if (tid == 0) TST[U] = P;
        cbar<GROWS>();
        for (int32_t b = 0; b < U; b += CT) {
            const int32_t r = b + tid;
            bool head = r < U && TST[r + 1] > TST[r];
            if (head) {
                int32_t q = r - 1;             // the present rank before r
                while (q >= 0 && TST[q + 1] == TST[q]) q--;
                if (q >= 0) {
                    const StreamPod x = TREC[q], y = TREC[r];
                    head = !((x.flags & y.flags & SF_BATCH) && (x.flags & ~SF_BATCH) == (y.flags & ~SF_BATCH) &&
                             x.cpu == y.cpu && x.mem == y.mem && x.eph == y.eph);
                }
            }
            int32_t tot;
            const int32_t slot = blk_compact<GROWS>(cred, par, wv, head, tot);
            if (head) TRUN[n_runs + slot] = make_int2(r, TST[r]);
            n_runs += tot;
        }
        if (tid == 0) TRUN[n_runs] = make_int2(0, P);
        cbar<GROWS>();
        t_nrec = TREC[TRUN[0].x];
        if (LEAN) { t_ndiv = TDIV[TRUN[0].x]; t_nct = TRCT[TRUN[0].x]; }
        t_npair = TRUN[min(1, n_runs)];
    }

    // add a template copy as new node k (addNewNodeToSnapshot, :146-159)
    // (LDS writes by one thread; a barrier follows before any wave reads the row)
    auto open_node = [&]() -> int32_t {
        const int32_t nn = k;
        if (tid == 0) {
            R[nn] = trec;
            SUM[nn >> 6] = trec;   // a fresh copy is the largest a row can be
        }
        if (use_ports && tid < CA_PORT_WORDS) PORTS[(size_t)nn * CA_PORT_WORDS + tid] = tp.used_ports[tid];
        if (use_scalar && tid < CA_MAX_SCALAR)
            SC[(size_t)tid * kcap + nn] = wsub(tp.node.alloc_scalar[tid], tp.used_scalar[tid]);
        k++;
        last_node = nn;
        l_used = false;
        return nn;
    };
    auto note_success = [&]() {
        if (!first_success) { first_success = true; sensitive = k >= 2; }
    };
    // publish the chunks whose outputs are all scheduled (wave 0 stores every result in
    // publishing mode: segments by thread 0, single placements by its lanes)
    int32_t tk_next = 0;
    int32_t tk_bound = pch;         // (tk_next + 1) * pch: progress() divides only once it is reached
    // outputs [pure_from, nsched) all come from run segments with stream offset pure_off
    // (pure chunks: push_chunks); a single placement or a segment with another offset
    // restarts the range
    int32_t pure_from = 0, pure_off = 0;
    auto note_segment = [&](int32_t dst, int32_t src) {
        if (src - dst != pure_off || dst < pure_from) { pure_from = dst; pure_off = src - dst; }
    };
    auto progress = [&]() {
        if (!tickets || !w0 || nsched < tk_bound) return;
        const int32_t c1 = nsched / pch;
        tk_bound = (c1 + 1) * pch;
        if (pend) {                       // the pending single placement, stored now
            so_pod[out_idx] = (TB || pos_out) ? wbase + lane : cur.pod;
            pend = false;
        }
        push_chunks(g, tk_next, c1, nsub, tickets, qctl, prog, nseg | (n_single ? INT32_MIN : 0), nsched, lane, pch, pure_from,
                    pure_off);
        tk_next = c1;
    };

    int32_t pos = 0;
#ifdef CASIM_PROF
    prof[14] = clock64() - t_cyc0;
#endif
    while (pos < P && !stop) {
        PROF_T(t_top);
        if (pos >= wbase + 64) {
            if (pend) {
                so_pod[out_idx] = (TB || pos_out) ? wbase + lane : cur.pod;
                if (so_node) so_node[out_idx] = out_node;
            }
            pend = false;
            if (TB) {
                wbase = pos & ~63;          // (the window only names the lanes of pending placements)
            } else if (pos < wbase + 128) {
                cur = nxt;
                wbase += 64;
                nxt = StreamPod{};
                if (wbase + 64 + lane < P) nxt = gs[wbase + 64 + lane];
            } else if ((pos & ~63) == pf_base) {
                wbase = pf_base;            // prefetched when the run that ends here started
                cur = pf_cur;
                nxt = pf_nxt;
            } else {
                wbase = pos & ~63;
                cur = StreamPod{};
                if (wbase + lane < P) cur = gs[wbase + lane];
                nxt = StreamPod{};
                if (wbase + 64 + lane < P) nxt = gs[wbase + 64 + lane];
            }
            pf_base = -1;
        }
        const int sl = pos - wbase;
        if (TB && pos >= t_end) {           // the next run of the table: its record and end
            cur = t_nrec;                   // (every lane: the same record)
            cur.flags |= SF_HEAD;           // a batchable run is entered at its head only
            t_end = rl32(t_npair.y, 0);
            t_next++;
            if (LEAN) { t_div = t_ndiv; t_ndiv = TDIV[t_npair.x]; t_ct = t_nct; t_nct = TRCT[t_npair.x]; }
            t_nrec = TREC[t_npair.x];       // the run after: in flight behind this run's LDS work
            t_npair = TRUN[min(t_next + 1, n_runs)];
        }
        const int rsl = TB ? 0 : sl;
        const int64_t pcpu = rl64(cur.cpu, rsl), pmem = rl64(cur.mem, rsl), peph = rl64(cur.eph, rsl);
        const int32_t pidx = rl32(cur.pod, rsl);
        const uint32_t sf = (uint32_t)rl32((int32_t)cur.flags, rsl);
        const bool zero = (sf & SF_ZERO) != 0;
#ifdef CASIM_PROF
        // (profiling: the stream chain's head loads land here, not in the run; the run-table
        // chain issues no load here and is timed without the drain, so its sections add up)
        if (!TB) __builtin_amdgcn_s_waitcnt(0);
#endif
        PROF_ADD(12, t_top);

        // ---------------- a run of identical resource-only pods ----------------
        // (LEAN: runs are the loop's body; the per-pod path below is laid out behind it)
        const bool is_run = batch_runs && (sf & (SF_BATCH | SF_HEAD)) == (SF_BATCH | SF_HEAD);
        if (LEAN ? __builtin_expect(is_run, true) : is_run) {
            PROF_T(t_re);
            PROF_T(t_run);
            const int32_t e = TB ? t_end : run_end_pf(hm, pos, P, lane, pf_hc, pf_hw);
            if (!TB && e < P) {
                const int32_t pb = e & ~63;
                if (pb >= wbase + 128) {
                    pf_base = pb;
                    pf_cur = StreamPod{};
                    if (pb + lane < P) pf_cur = gs[pb + lane];
                    pf_nxt = StreamPod{};
                    if (pb + 64 + lane < P) pf_nxt = gs[pb + 64 + lane];
                }
                pf_hc = e >> 6;
                pf_hw = pf_hc + lane < nhc ? hm[pf_hc + lane] : 0ull;
            }
            PROF_ADD(0, t_re);
            if constexpr (LEAN) if (e - pos >= 2) {
                // ---- the lean run: wave-owned rows, one barrier per row pass ----
                // 64-row block b belongs to wave co_owner(b) for the whole kernel, whatever k
                // is, and the owner does all row work of its blocks: the row pass, the update
                // after the pick, the single-row update, the rows of an opening.  A wave thus
                // reads back only rows it wrote itself (a wave's LDS operations are ordered),
                // and a run needs no barrier beyond its exchange.  What holds:
                //  * Order-dependent results come from per-block counts (lx.bc, lane = block
                //    after the exchange): the t-th qualifying row in row order is one prefix
                //    over the lanes and one ballot on that block's counts.  Sums, minima and
                //    the last row with room stay per-wave values (lx.v, 32-bit).
                //  * The copy counts alternate between CAPA and ALIVE with each row pass, the
                //    exchange records between the halves of lx with each exchange: a wave that
                //    is ahead writes the next pass's values while another still picks from
                //    this one's.  Between two writes of a shared word by different passes lies
                //    an exchange barrier that every reader of the first value has passed.
                //  * A pick reads counts only in a block whose published count is positive (the
                //    owner wrote every row of it in this pass); CAPA[last_node] likewise.
                //  * R[last_node].used is the uniform l_used, never read from the row here.
                //  * No wave reads a row another wave wrote without a barrier between: the
                //    exhausted path (R[last_node] after an opening), the empty-node path
                //    (open_node: thread 0 writes) and the per-pod path (rows, SUM: entered and
                //    left through a barrier, prev_step) keep barriers of their own, and the
                //    epilogue's count of used rows follows one.  All of these are cold.
                //  * Every barrier is in workgroup-uniform control flow (the conditions are the
                //    exchanged values and the run's uniform state).  A run without exchange has
                //    no barrier at all (k == 0: straight to the opening), so the buffer
                //    parities follow the exchanges and row passes, not the runs.
                PROF_INC(7);
                PROF_T(t_pro);
                if (prev_step == 2) { PROF_INC(23); cbar<false>(); }      // the per-pod path's row and SUM writes
                prev_step = 1;
                const int32_t RN = e - pos;
                const uint64_t kev = (sf & SF_EVAL) ? 1u : 0u;
                RunDiv dv;      // from the table: no division and no conversion at a run's entry
                for (int i = 0; i < 3; i++) { dv.reqd[i] = t_div.v[i]; dv.rcpd[i] = t_div.v[3 + i]; }
                dv.f64 = true;
                int32_t done = 0;
                bool exhausted = false;          // every row but last_node has no room left
                PROF_ADD(8, t_pro);
                while (done < RN) {
                    const int32_t rem = RN - done;
                    const int32_t len = n_base + k;
                    int32_t placed = 0;
                    if ((sf & SF_FA_OK) && k > 0) {
                        int32_t s0 = L;
                        if (s0 >= len) s0 = (int32_t)((uint32_t)s0 % (uint32_t)len);
                        const int32_t j0 = s0 > n_base ? s0 - n_base : 0;   // first new node visited
                        const int32_t nbw = co_wave_blocks(k, wv, CW);      // this wave's blocks
                        int32_t one = -1, n_one = 0, nalive = 0, S = 0;
                        int32_t lv_cmin = 0;      // revolution 1: fewest copies among rows with room
                        int32_t lv_s = 0;         // ... and how many of them lie before j0
                        int32_t bc1 = 0;          // lane = block: its rows with room
                        uint64_t adm_w = 0;       // bit i: the wave's i-th block has copy counts
                        int32_t* CAP = CAPA;      // this pass's copy counts
                        if (exhausted) {
                            PROF_T(t_ex);
                            PROF_ADDN(23, 2);
                            cbar<false>();    // the row's last write (an opening, open_node) is visible
                            const NodeRec rl_ = R[last_node];
                            const int32_t c = rec_copies_run<true>(rl_, dv, zero, rem, pcpu, pmem, peph);
                            cbar<false>();    // every wave has read the row before its owner changes it
                            if (c > 0) { one = last_node; n_one = c; nalive = 1; }
                            PROF_ADD(10, t_ex);
                        } else {
                            PROF_T(t_ca);
                            CAP = lcap ? ALIVE : CAPA;
                            lcap ^= 1;
                            wave_lds_order();     // rows this wave's other lanes opened or updated
                            // copies per row of the wave's blocks (two in flight), only where some
                            // row fits (rec_fits: compares only); for revolution 1 (rows with
                            // room): count per block, last such row, fewest copies, count below j0
                            int32_t s32 = 0, cm = INT32_MAX;          // copies (<= 2^24 per lane), fewest
                            int32_t na_w = 0, lt_w = 0, a1_w = -1;    // wave-uniform
                            int32_t cnt_l = 0;                        // lane i: rows with room in the wave's i-th block
                            auto acc = [&](int32_t i, int32_t b, int32_t c, bool in) -> int32_t {   // row 64 b + lane
                                if (in) CAP[(b << 6) + lane] = c;
                                const bool room = in && c > 0;
                                cm = room ? min(cm, c) : cm;
                                const uint64_t m = __ballot(room);
                                const int32_t pc = __builtin_popcountll(m);
                                na_w += pc;
                                lt_w += __builtin_popcountll(m & lanes_below(j0 - (b << 6)));
                                if (m) a1_w = (b << 6) + hibit(m);
                                cnt_l = lane == i ? pc : cnt_l;
                                return in ? c : 0;
                            };
                            for (int32_t i = 0; i < nbw; i += 2) {
                                const int32_t b0 = co_wave_block(wv, i, CW), b1 = co_wave_block(wv, i + 1, CW);
                                const int32_t ja = (b0 << 6) + lane, jb = (b1 << 6) + lane;
                                const bool in0 = ja < k, in1 = i + 1 < nbw && jb < k;
                                // (a lane past the rows reads the wave's own first row of the pair)
                                const NodeRec r0 = R[in0 ? ja : b0 << 6], r1 = R[in1 ? jb : b0 << 6];
                                const uint64_t f0 = __ballot(in0 && rec_fits(r0, pcpu, pmem, peph, zero));
                                const uint64_t f1 = __ballot(in1 && rec_fits(r1, pcpu, pmem, peph, zero));
                                PROF_ADDN(15, 1 + (i + 1 < nbw));
                                PROF_ADDN(16, (f0 != 0) + (f1 != 0));
                                if (f0) {
                                    adm_w |= 1ull << i;
                                    s32 += acc(i, b0, rec_copies_run(r0, dv, zero, rem, pcpu, pmem, peph), in0);
                                }
                                if (f1) {
                                    adm_w |= 1ull << (i + 1);
                                    s32 += acc(i + 1, b1, rec_copies_run(r1, dv, zero, rem, pcpu, pmem, peph), in1);
                                }
                            }
                            PROF_ADD(18, t_ca);
                            PROF_T(t_wr);
                            // S (each part saturated at rem), rows with room, last such row,
                            // fewest copies, rows < j0; and the per-block counts
                            const int32_t xs = min(__ockl_wfred_add_i32(s32), rem), xm = wave_min32(cm);
                            if (lane == 0) {
                                int32_t* v = lx.v[lpar][wv];
                                v[0] = xs; v[1] = na_w; v[2] = a1_w; v[3] = xm; v[4] = lt_w;
                            }
                            if (lane < nbw) lx.bc[lpar][co_wave_block(wv, lane, CW)] = cnt_l;
                            PROF_INC(23);
                            cbar<false>();            // + this pass's copy counts visible
                            int32_t a1 = -1;
                            lv_cmin = INT32_MAX;
                            for (int w = 0; w < CW; w++) {
                                const int32_t* v = lx.v[lpar][w];
                                S += v[0]; nalive += v[1]; a1 = max(a1, v[2]); lv_cmin = min(lv_cmin, v[3]); lv_s += v[4];
                            }
                            bc1 = lane < co_blocks(k) ? lx.bc[lpar][lane] : 0;
                            lpar ^= 1;
                            PROF_ADD(19, t_wr);
                            if (nalive == 1) { one = a1; n_one = min(S, rem); }
                            PROF_ADD(1, t_ca);
                        }
                        if (nalive == 1) {
                            // every remaining copy goes to the one row with room; its owner writes it
                            int32_t rho = one - j0;
                            if (rho < 0) rho += k;
                            evals += (uint64_t)rho + 1 + (uint64_t)(n_one - 1) * (uint64_t)k;
                            if (wv == co_owner(one >> 6, CW) && lane == 0) {
                                NodeRec r = R[one];
                                r.cpu -= (int64_t)n_one * pcpu;
                                r.mem -= (int64_t)n_one * pmem;
                                r.eph -= (int64_t)n_one * peph;
                                r.pods -= n_one;
                                r.used = 1;
                                R[one] = r;
                            }
                            L = n_base + one + 1;
                            if (L >= len) L -= len;
                            note_success();
                            placed = n_one;
                            l_used |= one == last_node;
                        } else if (nalive > 1) {
                            const int32_t n = min(S, rem);
                            PROF_T(t_rv);
                            // A level (revolutions r..cmin, rows with >= r copies) is a count, and
                            // only the last placement's row matters: the m-th row of its revolution
                            // in rotated order, i.e. the t-th qualifying row in row order, found by
                            // every wave from the blocks' counts and one ballot: no barrier.
                            int32_t got = 0, r = 1, last = -1;
                            int32_t lv_na = nalive, lv_bc = bc1;
                            for (;;) {
                                const int64_t avail = (int64_t)(lv_cmin - r + 1) * (int64_t)lv_na;
                                if ((int64_t)got + avail >= n) {
                                    const int32_t m0 = n - got;
                                    r += (m0 - 1) / lv_na;
                                    const int32_t m = (m0 - 1) % lv_na + 1;        // rank in rotated order
                                    const int32_t t = co_row_rank(m, lv_na, lv_s); // rank in row order (1-based)
                                    const int32_t incl = lane_incl_scan(lv_bc);
                                    const int32_t b = __builtin_ctzll(__ballot(co_block_holds(incl, lv_bc, t)));
                                    const int32_t tb = co_rank_in_block(rl32(incl, b), rl32(lv_bc, b), t);
                                    const int32_t j = (b << 6) + lane;
                                    const uint64_t bm = __ballot(j < k && CAP[j] >= r);
                                    const bool hit = ((bm >> lane) & 1ull) && mbcnt(bm) == tb - 1;
                                    last = (b << 6) + __builtin_ctzll(__ballot(hit));
                                    got = n;
                                    PROF_INC(6);
                                    break;
                                }
                                got += (int32_t)avail;
                                r = lv_cmin + 1;
                                // the next level: rows with at least r copies (one more exchange)
                                int32_t cnt_w = 0, lt2 = 0, cm2 = INT32_MAX, cnt_l = 0;
                                for (int32_t i = 0; i < nbw; i++) {
                                    if (!((adm_w >> i) & 1ull)) continue;
                                    const int32_t b = co_wave_block(wv, i, CW);
                                    const int32_t j = (b << 6) + lane;
                                    const int32_t c = j < k ? CAP[j] : 0;
                                    const bool q = c >= r;
                                    cm2 = q ? min(cm2, c) : cm2;
                                    const uint64_t m = __ballot(q);
                                    const int32_t pc = __builtin_popcountll(m);
                                    cnt_w += pc;
                                    lt2 += __builtin_popcountll(m & lanes_below(j0 - (b << 6)));
                                    cnt_l = lane == i ? pc : cnt_l;
                                }
                                const int32_t xm = wave_min32(cm2);
                                if (lane == 0) {
                                    int32_t* v = lx.v[lpar][wv];
                                    v[1] = cnt_w; v[3] = xm; v[4] = lt2;
                                }
                                if (lane < nbw) lx.bc[lpar][co_wave_block(wv, lane, CW)] = cnt_l;
                                PROF_INC(23);
                                cbar<false>();
                                lv_na = 0; lv_cmin = INT32_MAX; lv_s = 0;
                                for (int w = 0; w < CW; w++) {
                                    const int32_t* v = lx.v[lpar][w];
                                    lv_na += v[1]; lv_cmin = min(lv_cmin, v[3]); lv_s += v[4];
                                }
                                lv_bc = lane < co_blocks(k) ? lx.bc[lpar][lane] : 0;
                                lpar ^= 1;
                                PROF_INC(6);
                            }
                            PROF_ADD(2, t_rv);
                            PROF_T(t_up);
                            int32_t rl = last - j0;
                            if (rl < 0) rl += k;
                            evals += (uint64_t)(r - 1) * (uint64_t)k + (uint64_t)rl + 1;
                            // the wave's own rows, blocks with counts only (others: no room)
                            for (int32_t i = 0; i < nbw; i++) {
                                if (!((adm_w >> i) & 1ull)) continue;
                                const int32_t j = (co_wave_block(wv, i, CW) << 6) + lane;
                                const int32_t c = j < k ? CAP[j] : 0;
                                int32_t rj = j - j0;
                                if (rj < 0) rj += k;
                                const int32_t nj = min(c, r - 1) + ((c >= r && rj <= rl) ? 1 : 0);
                                if (nj > 0) {
                                    NodeRec q = R[j];
                                    q.cpu -= (int64_t)nj * pcpu;
                                    q.mem -= (int64_t)nj * pmem;
                                    q.eph -= (int64_t)nj * peph;
                                    q.pods -= nj;
                                    q.used = 1;
                                    R[j] = q;
                                }
                            }
                            PROF_ADD(3, t_up);
                            if (last_node >= 0 && !l_used) {      // (the update's nj of last_node)
                                const int32_t c = rl32(bc1, last_node >> 6) > 0 ? CAP[last_node] : 0;
                                int32_t rj = last_node - j0;
                                if (rj < 0) rj += k;
                                l_used = min(c, r - 1) + ((c >= r && rj <= rl) ? 1 : 0) > 0;
                            }
                            L = n_base + last + 1;
                            if (L >= len) L -= len;
                            note_success();
                            placed = n;
                        }
                    }
                    PROF_T(t_pb);
                    // (no barrier here: the rows updated above are read by their owners only)
                    if (tid == 0 && placed > 0) gseg[nseg] = Seg{nsched, pos + done, placed, 0};
                    if (placed > 0) note_segment(nsched, pos + done);
                    nseg += placed > 0 ? 1 : 0;
                    nsched += placed;
                    done += placed;
                    progress();
                    if (done == RN) break;
                    exhausted = true;
                    // the next pod of the run fails FitsAnyNode: every new node visited
                    evals += kev * (uint64_t)k;
                    if (max_nodes > 0 && granted >= max_nodes) { stop = true; break; }
                    granted++;
                    PROF_ADD(9, t_pb);
                    if (last_node >= 0 && !l_used) {
                        // :114-116 — and every later pod of the run repeats this pod's fate
                        done++;
                        const int32_t q = RN - done;
                        if (max_nodes > 0 && q > max_nodes - granted) {
                            const int32_t allowed = max_nodes - granted;
                            evals += (uint64_t)(allowed + 1) * kev * (uint64_t)k;
                            granted = max_nodes;
                            stop = true;
                            break;
                        }
                        evals += (uint64_t)q * kev * (uint64_t)k;
                        granted += q;
                        done = RN;
                        break;
                    }
                    if (k >= kcap) { res.status = CA_ECAPACITY; stop = true; break; }
                    const int32_t rem2 = RN - done;
                    if (!((sf & SF_CP_OK) && rec_fits(trec, pcpu, pmem, peph, zero))) {
                        // CheckPredicates on the new node fails: it stays empty and the next pod
                        // of the run takes the empty-node skip above.  Thread 0 writes the row
                        // and its block's summary, whoever owns them: between barriers.
                        PROF_ADDN(23, 2);
                        cbar<false>();
                        open_node();
                        if (sf & SF_CP_EVAL) evals++;
                        done++;
                        cbar<false>();
                        continue;
                    }
                    // Every row is full for this pod, so each remaining pod group opens a fresh
                    // template copy (the closed form of the generic body below); ct, the copies
                    // on a fresh copy, is the table's constant clipped to the pods left.
                    PROF_T(t_op);
                    const int32_t ct = !(sf & SF_FA_OK) ? 1 : min(t_ct, rem2);
                    PROF_ADD(20, t_op);
                    PROF_T(t_ow);
                    int32_t n_open = (rem2 + ct - 1) / ct;
                    if (max_nodes > 0) n_open = min(n_open, 1 + (max_nodes - granted));
                    n_open = min(n_open, kcap - k);
                    const int32_t k0 = k;
                    const int32_t placed2 = min(rem2, n_open * ct);
                    const int32_t len0 = n_base + k0 + 1;
                    int32_t s00 = L;
                    if (s00 >= len0) s00 = (int32_t)((uint32_t)s00 % (uint32_t)len0);
                    const int32_t j00 = s00 > n_base ? s00 - n_base : 0;
                    // each wave writes the opened rows of its blocks, and those blocks' summaries
                    for (int32_t b = co_first_block(k0 >> 6, wv, CW); (b << 6) < k0 + n_open; b += CW) {
                        int32_t lo, hi;
                        co_open_rows(k0, n_open, b, lo, hi);
                        const int32_t j = (b << 6) + lane;
                        if (j >= lo && j < hi) {
                            const int32_t i = j - k0;
                            const int32_t pi = (i == n_open - 1) ? placed2 - i * ct : ct;
                            NodeRec r = trec;
                            r.cpu -= (int64_t)pi * pcpu;
                            r.mem -= (int64_t)pi * pmem;
                            r.eph -= (int64_t)pi * peph;
                            r.pods -= pi;
                            r.used = 1;
                            R[j] = r;
                        }
                        if (lane == 0) SUM[b] = trec;
                    }
                    PROF_ADD(21, t_ow);
                    PROF_T(t_oe);
                    evals += open_evals(n_open, ct, placed2, k0, j00, kev, (sf & SF_CP_EVAL) != 0);
                    if (tid == 0 && placed2 > 0) gseg[nseg] = Seg{nsched, pos + done, placed2, 0};
                    if (placed2 > 0) note_segment(nsched, pos + done);
                    nseg += placed2 > 0 ? 1 : 0;
                    if (ct >= 2 && placed2 >= 2) {
                        if (!first_success) { first_success = true; sensitive = k0 + 1 >= 2; }
                        L = 0;       // n_base + (last row) + 1 == len
                    }
                    k = k0 + n_open;
                    last_node = k - 1;
                    l_used = true;       // every opened row holds at least one pod of the run
                    granted += n_open - 1;
                    nsched += placed2;
                    done += placed2;
                    progress();
                    PROF_ADD(22, t_oe);
                    PROF_ADD(4, t_op);
                }
                pos = e;
                PROF_ADD(11, t_run);
                continue;
            }
            if (!LEAN && e - pos >= 2) {     // (the generic run: two barriers, rows dealt out from k)
                PROF_INC(7);
                PROF_T(t_pro);
                const int32_t RN = e - pos;
                const uint64_t kev = (sf & SF_EVAL) ? 1u : 0u;
                // the pod's reciprocals, once per run (copy counts of every row, the last
                // row and the template: fast path while the cap is <= 2^20)
                const RunDiv dv = run_div(pcpu, pmem, peph, max(trec.cpu, max(trec.mem, trec.eph)));
                int32_t done = 0;
                bool exhausted = false;          // every row but last_node has no room left
                PROF_ADD(8, t_pro);
                while (done < RN) {
                    const int32_t rem = RN - done;
                    const int32_t len = n_base + k;
                    int32_t placed = 0;
                    // last_node's used bit after this iteration: its bit now (every row is
                    // visible here: a barrier ended the previous step) or a placement on it, so
                    // the empty-node check below needs no barrier after the row updates
                    bool last_used = last_node >= 0 && R[last_node].used;
                    if ((sf & SF_FA_OK) && k > 0) {
                        int32_t s0 = L;
                        if (s0 >= len) s0 = (int32_t)((uint32_t)s0 % (uint32_t)len);
                        const int32_t j0 = s0 > n_base ? s0 - n_base : 0;   // first new node visited
                        int32_t one = -1, n_one = 0, nalive = 0;
                        int64_t S = 0;
                        int64_t lv_cmin = 0;      // revolution 1: fewest copies among rows with room
                        int32_t lv_s = 0;         // ... and how many of them lie before j0
                        // blocks of this wave's row range whose copy counts were computed
                        // (bit i: rows [lo + 64 i, +64)); every other row has no room
                        uint64_t adm_w = 0;
                        if (exhausted) {
                            PROF_T(t_ex);
                            const NodeRec rl_ = R[last_node];
                            const int32_t c = rem <= (1 << 20) ? rec_copies_run(rl_, dv, zero, rem, pcpu, pmem, peph)
                                                               : rec_copies(rl_, pcpu, pmem, peph, zero, rem);
                            PROF_INC(23);
                            cbar<GROWS>();    // every wave has read the row before it changes
                            if (c > 0) { one = last_node; n_one = c; nalive = 1; }
                            PROF_ADD(10, t_ex);
                        } else {
                            PROF_T(t_ca);
                            // copies per row, and for revolution 1 (rows with room): count,
                            // last such row, fewest copies, count below j0 (rotation split)
                            int32_t lo, hi;
                            wave_rows(k, wv, lo, hi);
                            // counts, last row with room and the rotation split come from
                            // ballots (scalar); only the copy sum and minimum need reductions
                            int64_t s64 = 0;                          // copies (rem > 2^20 path)
                            int32_t s32 = 0, cm = INT32_MAX;          // copies (<= 2^24 per lane), fewest
                            int32_t na_w = 0, lt_w = 0, a1_w = -1;    // wave-uniform
                            auto acc = [&](int32_t b, int32_t c, bool in) -> int32_t {   // row b + lane
                                if (in) CAPA[b + lane] = c;
                                const bool room = in && c > 0;
                                cm = room ? min(cm, c) : cm;
                                const uint64_t m = __ballot(room);
                                na_w += __builtin_popcountll(m);
                                lt_w += __builtin_popcountll(m & lanes_below(j0 - b));
                                if (m) a1_w = b + hibit(m);
                                return in ? c : 0;
                            };
                            const bool fast = rem <= (1 << 20);
                            if (fast) {
                                // Block skip: a row has room for a copy iff the pod fits it
                                // (rec_fits: compares only), so the float64 copy counts run
                                // only for 64-row blocks where some row fits — in FFD most rows
                                // are full for most later pods (C2: ~5% of rows have room per
                                // pass).  The placement-list path (node ordinals) reads every
                                // row's count, so it computes them all.  Two blocks in flight.
                                const bool all = so_node != nullptr;
                                for (int32_t b = lo; b < hi; b += 128) {
                                    const int32_t j = b + lane;
                                    const bool in0 = j < hi, in1 = j + 64 < hi;
                                    const NodeRec r0 = R[in0 ? j : 0], r1 = R[in1 ? j + 64 : 0];
                                    const uint64_t f0 = __ballot(in0 && (all || rec_fits(r0, pcpu, pmem, peph, zero)));
                                    const uint64_t f1 = __ballot(in1 && (all || rec_fits(r1, pcpu, pmem, peph, zero)));
                                    PROF_ADDN(15, (b < hi) + (b + 64 < hi));
                                    PROF_ADDN(16, (f0 != 0) + (f1 != 0));
                                    if (f0) {
                                        adm_w |= 1ull << ((b - lo) >> 6);
                                        s32 += acc(b, rec_copies_run(r0, dv, zero, rem, pcpu, pmem, peph), in0);
                                    } else if (in0) {
                                        CAPA[j] = 0;      // (read by the other waves' pick)
                                    }
                                    if (f1) {
                                        adm_w |= 1ull << ((b + 64 - lo) >> 6);
                                        s32 += acc(b + 64, rec_copies_run(r1, dv, zero, rem, pcpu, pmem, peph), in1);
                                    } else if (in1) {
                                        CAPA[j + 64] = 0;
                                    }
                                }
                            } else {
                                adm_w = ~0ull;
                                for (int32_t b = lo; b < hi; b += 64) {
                                    const int32_t j = b + lane;
                                    const bool in = j < hi;
                                    s64 += acc(b, rec_copies(R[in ? j : 0], pcpu, pmem, peph, zero, rem), in);
                                }
                            }
                            PROF_ADD(18, t_ca);
                            PROF_T(t_wr);
                            int64_t x[RED_N];          // S, rows with room, last such row, fewest copies, rows < j0
                            x[0] = fast ? (int64_t)__ockl_wfred_add_i32(s32) : wave_sum64(s64);
                            x[1] = na_w; x[2] = a1_w; x[3] = wave_min32(cm); x[4] = lt_w;
                            constexpr int OPS[RED_N] = {R_SUM, R_SUM, R_MAX, R_MIN, R_SUM};
                            PROF_INC(23);
                            blk_xchg5<GROWS>(cred, par, wv, lane, x, OPS);     // + CAPA visible
                            PROF_ADD(19, t_wr);
                            S = x[0];
                            nalive = (int32_t)x[1];
                            lv_cmin = x[3];
                            lv_s = (int32_t)x[4];
                            if (nalive == 1) { one = (int32_t)x[2]; n_one = (int32_t)min(S, (int64_t)rem); }
                            PROF_ADD(1, t_ca);
                        }
                        if (nalive == 1) {
                            // every remaining copy goes to the one row with room
                            int32_t rho = one - j0;
                            if (rho < 0) rho += k;
                            evals += (uint64_t)rho + 1 + (uint64_t)(n_one - 1) * (uint64_t)k;
                            if (tid == 0) {
                                NodeRec r = R[one];
                                r.cpu -= (int64_t)n_one * pcpu;
                                r.mem -= (int64_t)n_one * pmem;
                                r.eph -= (int64_t)n_one * peph;
                                r.pods -= n_one;
                                r.used = 1;
                                R[one] = r;
                            }
                            if (so_node) for (int32_t t = tid; t < n_one; t += CT) so_node[nsched + t] = one;
                            L = n_base + one + 1;
                            if (L >= len) L -= len;
                            note_success();
                            placed = n_one;
                            last_used |= one == last_node;
                        } else if (nalive > 1) {
                            const int32_t n = (int32_t)min(S, (int64_t)rem);
                            PROF_T(t_rv);
                            int32_t got = 0, r = 1, last = -1;
                            int32_t* gdst = so_node ? so_node + nsched : nullptr;
                            if (!gdst) {
                            // Without node ordinals no placement list is needed: a level
                            // (revolutions r..cmin, rows with >= r copies) is a count, and
                            // only the last placement's row matters — the m-th row of its
                            // revolution in rotated order, i.e. the t-th qualifying row in
                            // row order, found from the waves' counts and one wave's ballots.
                            int32_t lv_na = nalive;
                            int lv_buf = par ^ 1;     // per-wave partial counts of this level (x[1])
                            for (;;) {
                                const int64_t avail = (lv_cmin - r + 1) * (int64_t)lv_na;
                                if ((int64_t)got + avail >= n) {
                                    const int32_t m0 = n - got;
                                    r += (m0 - 1) / lv_na;
                                    const int32_t m = (m0 - 1) % lv_na + 1;        // rank in rotated order
                                    const int32_t hiN = lv_na - lv_s;              // qualifying rows >= j0
                                    int32_t t = m <= hiN ? lv_s + m : m - hiN;     // rank in row order (1-based)
                                    int w = 0;
                                    for (; w < CW - 1; w++) {
                                        const int32_t cw_ = (int32_t)cred.v[lv_buf][w][1];
                                        if (t <= cw_) break;
                                        t -= cw_;
                                    }
                                    {   // every wave finds it in wave w's counts: no barrier
                                        int32_t lo, hi;
                                        wave_rows(k, w, lo, hi);
                                        for (int32_t b = lo; b < hi; b += 64) {
                                            const int32_t j = b + lane;
                                            const uint64_t bm = __ballot(j < hi && CAPA[j] >= r);
                                            const int32_t pc = __builtin_popcountll(bm);
                                            if (t <= pc) {
                                                const bool hit = ((bm >> lane) & 1ull) && mbcnt(bm) == t - 1;
                                                last = b + __builtin_ctzll(__ballot(hit));
                                                break;
                                            }
                                            t -= pc;
                                        }
                                    }
                                    got = n;
                                    PROF_INC(6);
                                    break;
                                }
                                got += (int32_t)avail;
                                r = (int32_t)lv_cmin + 1;
                                // the next level: rows with at least r copies
                                int32_t lo, hi;
                                wave_rows(k, wv, lo, hi);
                                int32_t cnt_w = 0, lt2 = 0, cm2 = INT32_MAX;
                                for (int32_t b = lo; b < hi; b += 64) {
                                    if (!((adm_w >> ((b - lo) >> 6)) & 1ull)) continue;
                                    const int32_t j = b + lane;
                                    const int32_t c = j < hi ? CAPA[j] : 0;
                                    const bool q = c >= r;
                                    cm2 = q ? min(cm2, c) : cm2;
                                    const uint64_t m = __ballot(q);
                                    cnt_w += __builtin_popcountll(m);
                                    lt2 += __builtin_popcountll(m & lanes_below(j0 - b));
                                }
                                int64_t y[RED_N] = {0, cnt_w, 0, wave_min32(cm2), lt2};   // -, count, -, min, count < j0
                                constexpr int OPS2[RED_N] = {R_SUM, R_SUM, R_SUM, R_MIN, R_SUM};
                                PROF_INC(23);
                                blk_xchg5<GROWS>(cred, par, wv, lane, y, OPS2);
                                lv_buf = par ^ 1;
                                lv_na = (int32_t)y[1];
                                lv_cmin = y[3];
                                lv_s = (int32_t)y[4];
                                PROF_INC(6);
                            }
                            } else {
                            // revolution 1: rows with room, in rotated order from j0
                            int32_t na = 0;
                            int64_t cmin = INT32_MAX, z0 = 0, z1 = 0;
                            for (int32_t b = 0; b < k; b += CT) {
                                const int32_t rr = b + tid;
                                int32_t j = j0 + rr;
                                if (j >= k) j -= k;
                                const int32_t c = rr < k ? CAPA[j] : 0;
                                const bool keep = c >= 1;
                                int32_t tot;
                                const int32_t slot = blk_compact<GROWS>(cred, par, wv, keep, tot);
                                if (keep) { ALIVE[na + slot] = j; cmin = min(cmin, (int64_t)c); }
                                na += tot;
                            }
                            blk_red3<R_MIN, R_SUM, R_SUM, GROWS>(cred, par, wv, lane, cmin, z0, z1);   // + ALIVE visible
                            // Revolutions r..cmin serve the same alive list (no row runs out
                            // before cmin), so the list is compacted once per distinct copy
                            // level, and the placements of those revolutions are the list
                            // repeated: placement t of the level goes to ALIVE[t % na].
                            for (;;) {
                                const int64_t avail = (int64_t)(cmin - r + 1) * na;
                                const bool fin = got + avail >= n;
                                const int32_t cnt = fin ? n - got : (int32_t)avail;
                                if (gdst) {
                                    const int32_t st = CT % na;
                                    int32_t q = tid % na;
                                    for (int32_t t = tid; t < cnt; t += CT) {
                                        gdst[got + t] = ALIVE[q];
                                        q += st;
                                        if (q >= na) q -= na;
                                    }
                                }
                                if (fin) {
                                    r += (cnt - 1) / na;                    // revolution of the last placement
                                    last = ALIVE[(cnt - 1) % na];
                                    got = n;
                                    PROF_INC(6);
                                    break;
                                }
                                got += cnt;
                                r = cmin + 1;
                                // the rows with at least r copies stay
                                // (in place: a chunk's writes land below its end, and the
                                // barrier in blk_compact orders them after the chunk's reads)
                                int32_t nn2 = 0;
                                int64_t cm2 = INT32_MAX;
                                for (int32_t b = 0; b < na; b += CT) {
                                    const int32_t i = b + tid;
                                    const int32_t j = i < na ? ALIVE[i] : 0;
                                    const int32_t c = i < na ? CAPA[j] : 0;
                                    const bool keep = c >= r;
                                    int32_t tot;
                                    const int32_t slot = blk_compact<GROWS>(cred, par, wv, keep, tot);
                                    if (keep) { ALIVE[nn2 + slot] = j; cm2 = min(cm2, (int64_t)c); }
                                    nn2 += tot;
                                }
                                na = nn2;
                                blk_red3<R_MIN, R_SUM, R_SUM, GROWS>(cred, par, wv, lane, cm2, z0, z1);   // + ALIVE visible
                                cmin = cm2;
                                PROF_INC(6);
                            }
                            }
                            PROF_ADD(2, t_rv);
                            PROF_T(t_up);
                            int32_t rl = last - j0;
                            if (rl < 0) rl += k;
                            evals += (uint64_t)(r - 1) * (uint64_t)k + (uint64_t)rl + 1;
                            {   // the wave's own rows, blocks with counts only (others: no room)
                                int32_t lo, hi;
                                wave_rows(k, wv, lo, hi);
                                for (int32_t b = lo; b < hi; b += 64) {
                                    if (!((adm_w >> ((b - lo) >> 6)) & 1ull)) continue;
                                    const int32_t j = b + lane;
                                    const int32_t c = j < hi ? CAPA[j] : 0;
                                    int32_t rj = j - j0;
                                    if (rj < 0) rj += k;
                                    const int32_t nj = min(c, r - 1) + ((c >= r && rj <= rl) ? 1 : 0);
                                    if (nj > 0) {
                                        NodeRec q = R[j];
                                        q.cpu -= (int64_t)nj * pcpu;
                                        q.mem -= (int64_t)nj * pmem;
                                        q.eph -= (int64_t)nj * peph;
                                        q.pods -= nj;
                                        q.used = 1;
                                        R[j] = q;
                                    }
                                }
                            }
                            PROF_ADD(3, t_up);
                            if (last_node >= 0 && !last_used) {      // (the update's nj of last_node)
                                const int32_t c = CAPA[last_node];
                                int32_t rj = last_node - j0;
                                if (rj < 0) rj += k;
                                last_used = min(c, r - 1) + ((c >= r && rj <= rl) ? 1 : 0) > 0;
                            }
                            L = n_base + last + 1;
                            if (L >= len) L -= len;
                            note_success();
                            placed = n;
                        }
                    }
                    PROF_T(t_pb);
                    // The row updates become visible to every wave at the next barrier: right
                    // below when the run ends here, else the node opening's (its rows are new,
                    // beyond every row read or written above)
                    if (tid == 0 && placed > 0) gseg[nseg] = Seg{nsched, pos + done, placed, 0};
                    if (placed > 0) note_segment(nsched, pos + done);
                    nseg += placed > 0 ? 1 : 0;
                    nsched += placed;
                    done += placed;
                    progress();
                    if (done == RN) { PROF_INC(23); cbar<GROWS>(); break; }
                    exhausted = true;
                    // the next pod of the run fails FitsAnyNode: every new node visited
                    evals += kev * (uint64_t)k;
                    if (max_nodes > 0 && granted >= max_nodes) { stop = true; break; }
                    granted++;
                    PROF_ADD(9, t_pb);
                    if (last_node >= 0 && !last_used) {
                        // :114-116 — and every later pod of the run repeats this pod's fate
                        done++;
                        const int32_t q = RN - done;
                        if (max_nodes > 0 && q > max_nodes - granted) {
                            const int32_t allowed = max_nodes - granted;
                            evals += (uint64_t)(allowed + 1) * kev * (uint64_t)k;
                            granted = max_nodes;
                            stop = true;
                            break;
                        }
                        evals += (uint64_t)q * kev * (uint64_t)k;
                        granted += q;
                        done = RN;
                        PROF_INC(23);
                        cbar<GROWS>();
                        break;
                    }
                    if (k >= kcap) { res.status = CA_ECAPACITY; stop = true; break; }
                    const int32_t rem2 = RN - done;
                    if (!((sf & SF_CP_OK) && rec_fits(trec, pcpu, pmem, peph, zero))) {
                        // CheckPredicates on the new node fails: it stays empty and the
                        // next pod of the run takes the empty-node skip above
                        open_node();
                        if (sf & SF_CP_EVAL) evals++;
                        done++;
                        PROF_INC(23);
                        cbar<GROWS>();
                        continue;
                    }
                    // Every row is full for this pod, so each remaining pod group opens a
                    // fresh template copy: pod 1 by CheckPredicates (:132-135), the next
                    // ct-1 by FitsAnyNode, whose scan ends at the new (last) row, so after
                    // the first one lastIndex wraps to 0 and each costs k evals.  A
                    // node's opening pod first fails FitsAnyNode over the k rows before it
                    // and takes one limiter grant.  Closed form over n_open nodes.
                    PROF_T(t_op);
                    const int32_t ct = !(sf & SF_FA_OK) ? 1
                                       : rem2 <= (1 << 20) ? rec_copies_run(trec, dv, zero, rem2, pcpu, pmem, peph)
                                                           : rec_copies(trec, pcpu, pmem, peph, zero, rem2);
                    PROF_ADD(20, t_op);
                    PROF_T(t_ow);
                    int32_t n_open = (rem2 + ct - 1) / ct;
                    if (max_nodes > 0) n_open = min(n_open, 1 + (max_nodes - granted));
                    n_open = min(n_open, kcap - k);
                    const int32_t k0 = k;
                    const int32_t placed2 = min(rem2, n_open * ct);
                    const int32_t len0 = n_base + k0 + 1;
                    int32_t s00 = L;
                    if (s00 >= len0) s00 = (int32_t)((uint32_t)s00 % (uint32_t)len0);
                    const int32_t j00 = s00 > n_base ? s00 - n_base : 0;
                    for (int32_t i = tid; i < n_open; i += CT) {
                        const int32_t pi = (i == n_open - 1) ? placed2 - i * ct : ct;
                        NodeRec r = trec;
                        r.cpu -= (int64_t)pi * pcpu;
                        r.mem -= (int64_t)pi * pmem;
                        r.eph -= (int64_t)pi * peph;
                        r.pods -= pi;
                        r.used = 1;
                        R[k0 + i] = r;
                    }
                    for (int32_t b = (k0 >> 6) + tid; b <= ((k0 + n_open - 1) >> 6); b += CT) SUM[b] = trec;
                    if (use_ports) {
                        for (int32_t i = tid; i < n_open * CA_PORT_WORDS; i += CT)
                            PORTS[(size_t)k0 * CA_PORT_WORDS + i] = tp.used_ports[i % CA_PORT_WORDS];
                    }
                    if (use_scalar) {
                        for (int32_t i = tid; i < n_open * CA_MAX_SCALAR; i += CT) {
                            const int32_t sc = i / n_open, node = k0 + i % n_open;
                            SC[(size_t)sc * kcap + node] = wsub(tp.node.alloc_scalar[sc], tp.used_scalar[sc]);
                        }
                    }
                    PROF_INC(23);
                    cbar<GROWS>();                                                  // new rows visible
                    PROF_ADD(21, t_ow);
                    PROF_T(t_oe);
                    evals += open_evals(n_open, ct, placed2, k0, j00, kev, (sf & SF_CP_EVAL) != 0);
                    if (so_node) for (int32_t t = tid; t < placed2; t += CT) so_node[nsched + t] = k0 + t / ct;
                    if (tid == 0 && placed2 > 0) gseg[nseg] = Seg{nsched, pos + done, placed2, 0};
                    if (placed2 > 0) note_segment(nsched, pos + done);
                    nseg += placed2 > 0 ? 1 : 0;
                    if (ct >= 2 && placed2 >= 2) {
                        if (!first_success) { first_success = true; sensitive = k0 + 1 >= 2; }
                        L = 0;       // n_base + (last row) + 1 == len
                    }
                    k = k0 + n_open;
                    last_node = k - 1;
                    granted += n_open - 1;
                    nsched += placed2;
                    done += placed2;
                    progress();
                    PROF_ADD(22, t_oe);
                    PROF_ADD(4, t_op);
                }
                pos = e;
                PROF_ADD(11, t_run);
                continue;
            }
        }

        // ---------------- one pod ----------------
        // rare per-pod data (ports / scalars) from the full record
        uint64_t pconf[CA_PORT_WORDS] = {0, 0}, puse[CA_PORT_WORDS] = {0, 0};
        int64_t psc[CA_MAX_SCALAR];
        for (int i = 0; i < CA_MAX_SCALAR; i++) psc[i] = 0;
        if (PS && (sf & (SF_PORTS | SF_SCALAR))) {
            const ca_pod_spec& s = specs[ph[pidx].spec];
            for (int w = 0; w < CA_PORT_WORDS; w++) { pconf[w] = s.port_conflict[w]; puse[w] = s.port_use[w]; }
            for (int i = 0; i < CA_MAX_SCALAR; i++) psc[i] = s.req_scalar[i];
        }
        pos++;
        n_single++;
        if (LEAN) {     // the run before wrote rows and summaries with no barrier behind them
            if (prev_step == 1) { PROF_INC(23); cbar<false>(); }
            prev_step = 2;
        }

        // ---- FitsAnyNodeMatching(newNodeNames) (binpacking_estimator.go:91-93) ----
        int32_t found = -1;
        if ((sf & SF_EVAL) && k > 0) {
            if (sf & SF_FA_OK) {
                const int32_t len = n_base + k;
                int32_t s0 = L;                                                // (lastIndex+i) % len at i = 0
                if (s0 >= len) s0 = (int32_t)((uint32_t)s0 % (uint32_t)len);   // only for a caller-supplied L
                const int32_t j0 = s0 > n_base ? s0 - n_base : 0;              // first new node visited
                const int32_t nb = (k + 63) >> 6;
                const int32_t b0 = j0 >> 6;
                const bool lower_part = (j0 & 63) != 0;    // block b0 is visited twice (>= j0, then < j0)
                for (int32_t rbase = 0; rbase <= nb && found < 0; rbase += 64) {
                    // visit order: rotated block r -> block (b0 + r) mod nb; r == nb is b0's lower part
                    const int32_t rb = rbase + lane;
                    int32_t b = rb < nb ? b0 + rb : b0;
                    if (b >= nb) b -= nb;
                    const bool rb_ok = (rb < nb) | ((rb == nb) & lower_part);
                    const NodeRec sr = SUM[rb_ok ? b : 0];
                    const bool adm = rb_ok & rec_fits(sr, pcpu, pmem, peph, zero);
                    uint64_t amask = __ballot(adm);
                    while (amask && found < 0) {
                        const int l = __builtin_ctzll(amask);
                        amask &= amask - 1;
                        const int32_t r = rbase + l;
                        int32_t bb = r < nb ? b0 + r : b0;
                        if (bb >= nb) bb -= nb;
                        const int32_t j = (bb << 6) + lane;
                        const bool valid = (j < k) & ((r != 0) | (j >= j0)) & ((r != nb) | (j < j0));
                        const NodeRec nr = R[j < k ? j : 0];
                        bool fit = valid & rec_fits(nr, pcpu, pmem, peph, zero);
                        if (PS && (sf & SF_SCALAR)) {
                            for (int i = 0; i < CA_MAX_SCALAR; i++)
                                fit = fit & !((psc[i] != 0) & (j < k) && psc[i] > SC[(size_t)i * kcap + (j < k ? j : 0)]);
                        }
                        if (PS && (sf & SF_PORTS)) {
                            uint64_t c = 0;
                            for (int w = 0; w < CA_PORT_WORDS; w++) c |= PORTS[(size_t)(j < k ? j : 0) * CA_PORT_WORDS + w] & pconf[w];
                            fit = fit & (c == 0);
                        }
                        const uint64_t fmask = __ballot(fit);
                        if (fmask) {
                            found = (bb << 6) + __builtin_ctzll(fmask);
                        } else {
                            // no row of the visited part fits: tighten the block summary
                            // to the exact per-dimension maxima of the whole block
                            const bool in = j < k;
                            const int64_t mc = wave_max64(in ? nr.cpu : INT64_MIN);
                            const int64_t mm = wave_max64(in ? nr.mem : INT64_MIN);
                            const int64_t me = wave_max64(in ? nr.eph : INT64_MIN);
                            const int32_t mp = wave_max32(in ? nr.pods : INT32_MIN);
                            // (one writer; another wave may read either value of any field:
                            // both bound every row of the block, so its `found` is the same)
                            if (tid == 0) {
                                NodeRec sm;
                                sm.cpu = mc; sm.mem = mm; sm.eph = me; sm.pods = mp; sm.used = 0;
                                SUM[bb] = sm;
                            }
                        }
                    }
                }
                if (found >= 0) {
                    int32_t off = found - j0;                                  // rotated offset among new nodes
                    if (off < 0) off += k;
                    evals += (uint64_t)off + 1;
                    note_success();
                    L = n_base + found + 1;                                    // schedulerbased.go:131
                    if (L >= len) L -= len;
                } else {
                    evals += (uint64_t)k;
                }
            } else {
                evals += (uint64_t)k;                  // every new node visited, filters fail
            }
        }
        if (found < 0) {
            // PermissionToAddNode (threshold_based_limiter.go:46-56), before the empty-node skip
            if (max_nodes > 0 && granted >= max_nodes) break;
            granted++;
            if (last_node >= 0 && !(LEAN ? l_used : R[last_node].used != 0)) continue;   // :114-116
            if (k >= kcap) { res.status = CA_ECAPACITY; break; }
            PROF_INC(23);
            cbar<GROWS>();                    // every wave's scan is done before rows change
            const int32_t nn = open_node();
            // CheckPredicates(pod, newNode) (:132-134)
            if (sf & SF_CP_EVAL) evals++;
            bool ok = (sf & SF_CP_OK) != 0;
            if (ok) {
                ok = rec_fits(trec, pcpu, pmem, peph, zero);
                if (PS && ok && (sf & SF_SCALAR)) {
                    for (int i = 0; i < CA_MAX_SCALAR; i++)
                        if (psc[i] != 0 && psc[i] > wsub(tp.node.alloc_scalar[i], tp.used_scalar[i])) ok = false;
                }
                if (PS && ok && (sf & SF_PORTS)) {
                    uint64_t c = 0;
                    for (int w = 0; w < CA_PORT_WORDS; w++) c |= tp.used_ports[w] & pconf[w];
                    ok = c == 0;
                }
            }
            if (!ok) { PROF_INC(23); cbar<GROWS>(); continue; }
            found = nn;
        }
        PROF_INC(23);
        cbar<GROWS>();                        // every wave's scan is done before R[found] changes
        // AddPod(pod, node) (:96 / :135) — NodeInfo.update on the new-node row
        if (tid == 0) {
            NodeRec r = R[found];
            r.cpu = wsub(r.cpu, pcpu);
            r.mem = wsub(r.mem, pmem);
            r.eph = wsub(r.eph, peph);
            r.pods -= 1;
            r.used = 1;
            R[found] = r;
        }
        l_used |= found == last_node;
        if (w0 && lane == sl) { out_node = found; out_idx = nsched; pend = true; }
        if (PS && (sf & SF_SCALAR)) {
            if (tid < CA_MAX_SCALAR) {
                const size_t ix = (size_t)tid * kcap + found;
                SC[ix] = wsub(SC[ix], psc[tid]);
            }
        }
        if (PS && (sf & SF_PORTS)) {
            if (tid < CA_PORT_WORDS) PORTS[(size_t)found * CA_PORT_WORDS + tid] |= puse[tid];
        }
        nsched++;
        pure_from = nsched;                   // a single placement: written by the chain itself
        progress();
        PROF_INC(23);
        cbar<GROWS>();                        // the placement is visible to every wave
    }
    PROF_T(t_epi);
    if (pend) {
        so_pod[out_idx] = (TB || pos_out) ? wbase + lane : cur.pod;
        if (so_node) so_node[out_idx] = out_node;
    }
#ifdef CASIM_PROF
    __shared__ unsigned long long s_blk[CW][2];     // each wave's block counters, for the busiest one
    if (lane == 0) { s_blk[wv][0] = prof[15]; s_blk[wv][1] = prof[16]; }
#endif
    // newNodesWithPods
    cbar<GROWS>();
    int64_t cnt = 0, z0 = 0, z1 = 0;
    for (int32_t j = tid; j < k; j += CT) cnt += R[j].used;
    blk_red3<R_SUM, R_SUM, R_SUM, GROWS>(cred, par, wv, lane, cnt, z0, z1);
    if (tid == 0) {
        res.node_count = (int32_t)cnt;
        res.n_sched = nsched;
        res.nodes_added = k;
        res.lout = L;
        res.sensitive = sensitive ? 1 : 0;
        res.had_success = first_success ? 1 : 0;
        res.evals = evals;
        res.nseg = nseg;
        res.pad = (uint64_t)(uint32_t)(wall_clock64() - t_begin) | ((uint64_t)n_single << 32);
        outs[g] = res;
        hout[g] = res;                          // zero-copy: the host reads it after the round's event
    }
    if (tickets) {
        __threadfence();                        // every wave's result stores, before the release
        __syncthreads();
        if (w0) {
            const bool ok = res.status == CA_OK;
            // a group that failed after publishing chunks: the host falls back to the copy
            if (!ok && tk_next > 0 && lane == 0) { atomicExch(&qctl[3], 1); hflags[3] = 1; }
            // every pod scheduled: the tail chunks are pure when one segment offset covers them
            // (the publisher copies them straight from the stream's ids, no segment reads)
            const bool all = ok && nsched == P;
            push_chunks(g, tk_next, (P + pch - 1) / pch, nsub, tickets, qctl, prog,
                        ok ? nseg | (n_single ? INT32_MIN : 0) : 0, ok ? nsched : 0, lane,
                        all ? pch : 0, all ? pure_from : INT32_MAX, pure_off);
        }
    }
    if (tid == 0) {
#ifdef CASIM_PROF
        prof[13] = clock64() - t_epi;
        prof[5] = clock64() - t_cyc0;
        int bw = 0;
        for (int w = 1; w < CW; w++) if (s_blk[w][1] > s_blk[bw][1]) bw = w;
        prof[15] = s_blk[bw][0]; prof[16] = s_blk[bw][1]; prof[17] = (unsigned long long)bw;
        if (g < 1024) for (int i = 0; i < NPROF; i++) g_chain_prof[g][i] = prof[i];
#endif
    }
}

// Round-1 state of a batch in one launch instead of five copies/fills on the critical
// path: every group needed, every group from the caller's lastIndex, no unsupported
// group yet, publisher tickets empty, queue counters zero.
__global__ void __launch_bounds__(256) k_round_init(int32_t G, int32_t lin0, int32_t* __restrict__ lin,
                                                   uint8_t* __restrict__ need, uint32_t* __restrict__ unsup,
                                                   int64_t* __restrict__ tickets, int32_t n_tickets,
                                                   int32_t* __restrict__ qctl) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    const int32_t stride = (int32_t)(gridDim.x * blockDim.x);
    for (int32_t g = i; g < G; g += stride) { lin[g] = lin0; need[g] = 1; unsup[g] = 0; }
    if (tickets)
        for (int32_t t = i; t < n_tickets; t += stride) tickets[t] = -1;
    if (qctl && i < 6) qctl[i] = 0;
}

// 5. scheduled pods of the run placements: sched_pod[dst + t] = stream pod at src + t.
// Output i of a group lies in the last segment with dst <= i, or was written directly
// by the chain (single-pod placements).  One block per CPY_PER_BLOCK outputs: one
// binary search for the first segment reaching the block's range, then the segments
// of the range are copied in turn (coalesced reads of the stream's pod ids).
constexpr int CPY_PER_BLOCK = 2048;
__global__ void __launch_bounds__(256) k_copy_segments(const GroupMeta* __restrict__ groups,
                                                      const ChainOut* __restrict__ outs, const Seg* __restrict__ segs,
                                                      const int32_t* __restrict__ spod, int32_t* __restrict__ sched_pod,
                                                      int32_t* __restrict__ sched_node, int32_t map_singles) {
    const GroupMeta gm = groups[blockIdx.y];
    const ChainOut o = outs[blockIdx.y];
    const int32_t base = (int32_t)blockIdx.x * CPY_PER_BLOCK;
    if (base >= gm.count) return;
    const int32_t end = min(base + CPY_PER_BLOCK, gm.count);
    const int32_t ns = o.status == CA_OK ? o.n_sched : 0;
    const int32_t nseg = o.status == CA_OK ? o.nseg : 0;
    const Seg* gs = segs + gm.off;
    int32_t* sp = sched_pod + gm.off;
    const int32_t* src = spod + (map_singles ? gm.ids_off : gm.off);   // (decoupled: maybe a shared sort's ids)
    // past n_scheduled (or a failed group): -1, also over what an earlier speculation
    // round of the group wrote
    for (int32_t i = max(base, ns) + (int32_t)threadIdx.x; i < end; i += blockDim.x) {
        sp[i] = -1;
        if (sched_node) sched_node[gm.off + i] = -1;
    }
    const int32_t lim = min(end, ns);
    if (base >= lim) return;
    int32_t lo = 0, hi = nseg;                     // first segment ending after base
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        const Seg sg = gs[mid];
        if (sg.dst + sg.len <= base) lo = mid + 1; else hi = mid;
    }
    int32_t at = base;                              // single placements before segment q
    for (int32_t q = lo; q <= nseg && at < lim; q++) {
        const Seg sg = q < nseg ? gs[q] : Seg{lim, 0, 0};
        const int32_t gap_end = min(lim, max(at, sg.dst));
        if (map_singles)                            // stream positions -> pod ids (decoupled Go order)
            for (int32_t i = at + (int32_t)threadIdx.x; i < gap_end; i += blockDim.x) sp[i] = src[sp[i]];
        if (q == nseg || sg.dst >= lim) break;
        const int32_t a = max(base, sg.dst), b = min(lim, sg.dst + sg.len);
        const int32_t off = sg.src - sg.dst;
        for (int32_t i = a + (int32_t)threadIdx.x; i < b; i += blockDim.x) sp[i] = src[off + i];
        at = max(at, b);
    }
}

}  // namespace casim

using namespace casim;

struct ca_estimate_plan {
    ca_mirror* m = nullptr;
    const ca_podset* s = nullptr;
    int32_t G = 0;
    int32_t total = 0;
    int32_t max_count = 0;
    std::vector<int32_t> h_off;
    std::vector<ca_template> h_tmpl;
    std::vector<GroupMeta> h_meta;
    bool use_ports = false, use_scalar = false;
    int32_t n_masks = 0, n_tiles = 0;
    DevBuf d_meta, d_pod_idx, d_tmpl, d_sortA, d_sortB, d_stream, d_spod, d_seg, d_heads, d_unsup, d_lin, d_need,
        d_out, d_sched_pod, d_sched_node, d_crank, d_hist, d_sched16;
    // Go sort.Slice order (k_pdq_sort): element store, list scratch, frame stacks, and the
    // per-position ranks of the comparison path
    DevBuf d_pdq_e, d_pdq_scr, d_pdq_stack, d_item_rank;
    // decoupled Go order (uniform classes): the chains run on the stable class order while
    // k_pdq_sort on st3 writes the Go-order ids into d_spod_go (d_sortC: the
    // permutation; d_ids_ready: per group, the run epoch whose ids are final there)
    DevBuf d_sortC, d_ids_ready, d_spod_go, d_crank2;
    DevBuf d_rstart, d_rsp;        // decoupled: per group, each rank's first stream position and record
    DevBuf d_rdiv;                 // ... and its requests and their reciprocals in float64 (RDIV_N per rank: the lean chain)
    // every template's free values and every pod's requests are below 2^53: float64 copy
    // counts are exact for every run of this plan (a condition of the lean chain)
    bool f64_exact = false;
    DevBuf d_item_cls;             // bucket path: the score class of every (group, pod) item, uploaded with the lists
    // ... with uniform classes: [G][n_cls] items of each class in each list (k_cls_hist), in
    // the tail of d_item_cls (one allocation: a hipMalloc costs more than the histogram)
    bool has_cls_cnt = false;
    int32_t* cls_cnt() const { return d_item_cls.as<int32_t>() + total; }
    float opt_lists_ms = 0.f;      // option form: device time of k_option_lists at creation (0 otherwise)
    int32_t ids_epoch = 0;
    // The Go-order ids belong to the plan: `ids` records the epoch and the
    // settings d_spod_go / d_ids_ready were last sorted under, and a decoupled run whose
    // settings match launches no sort.  Every run clears ids.valid on entry and only a
    // decoupled run that returns CA_OK sets it again, so an error, the coupled Go sort and
    // the radix / merge paths (which share d_pdq_e / d_pdq_scr / d_pdq_stack with the sort)
    // all leave it invalid.  ids_sorts / ids_fan: what that sort launched (timings [10], [11]).
    // ids_done: the host has seen the sort finished (ev_ids), so every flag is up.
    casim::GoSortRecord ids;
    int32_t ids_sorts = 0, ids_fan = 0;
    bool ids_done = false;
    int32_t ran_reused = 0;        // last run launched no Go-order sort
    // shared sorts (sort_classes): the number of sort classes — when below G their
    // representatives, in group order, follow the G records of d_meta as k_pdq_sort's group
    // map — and the number of sorts the last run launched
    int32_t n_sorts = 0, ran_sorts = 0;
    // two-launch sort (k_pdq_sort + k_pdq_sort_parts): d_ids_ready holds
    // one fan record per group (pdqsort.h FAN_*), d_fan_map the representatives whose lists
    // are longer than fan_min, d_pdq_pstack the part workgroups' own frame areas
    int32_t fan_parts = 0, fan_min = 0, fan_steps = 0, n_fan = 0, ran_fan = 0;
    DevBuf d_fan_map, d_pdq_pstack;
    hipStream_t st3 = nullptr;
    hipEvent_t ev_emitA = nullptr, ev_emitB = nullptr, ev_ids = nullptr;
    // HBM-slab rows (k_ffd_chain<true>): per group kcap and slab offset, for the limiter
    // setting they were sized for (slab_max_nodes)
    DevBuf d_slab, d_slab_off, d_gkcap;
    int32_t slab_max_nodes = -2;
    int32_t n_hist = 0, max_rtiles = 0;
    bool bucket = false;           // bucket sort over score classes (podset has <= CLS_MAX classes)
    // decoupled Go order allowed: uniform classes, bucket path, and no
    // group holds two classes whose float64 scores against its template are equal
    bool decouple_ok = false;
    Stats stats;
    // per-phase device timings of the last run (ms): score, merge, emit, chain (all
    // rounds), compact, d2h; and the host wall time of the call
    enum { EV_START, EV_SCORE, EV_MERGE, EV_EMIT, EV_CHAIN0, EV_CHAIN1, EV_COMPACT, EV_D2H, EV_N };
    hipEvent_t ev[EV_N] = {};
    float t_ms[7] = {};
    int32_t pub_state = 0;         // last run: 0 results copied, 1 published zero-copy, 2 publisher gave up
    // the publisher's tickets are all -1 and its control words zero on the device: every
    // publisher consumed and reset its tickets and its last block cleared the words (round 1
    // then needs no k_round_init; false at first and after a publisher gave up)
    bool pub_clean = false;
    int32_t ran_decoupled = 0;     // last run took the decoupled Go order
    int32_t ran_table_chain = 0;   // ... and its chains walked the run table (k_ffd_chain<.., TB>)
    int32_t ran_lean_chain = 0;    // ... with the lean instantiation (k_ffd_chain<.., TB, LEAN>)
    bool phase_events = true;      // record the per-phase timing events (ca_estimate_plan_set_phase_timing)
    std::vector<uint64_t> diag;     // per group: chain ticks (100 MHz) | single-pod steps << 32
    std::vector<uint8_t> grp_succ;  // last run, per group: a FitsAnyNode call succeeded (moved lastIndex)
    // zero-copy publishing (k_publish on its own stream, concurrent with the chains)
    hipStream_t pub_stream = nullptr;
    hipEvent_t ev_go = nullptr, ev_pub = nullptr;
    DevBuf d_tickets, d_qctl;
    int32_t n_tickets = 0, nsub = 0, pch = PCH;
    DevBuf d_prog;                 // progress record per ticket slot (segments, pods scheduled)
    // page-locked landing buffers of the per-round readback (chain outputs + publisher
    // counters): one small D2H each and one synchronisation per round
    HostBuf h_out, h_qc;
    // Heavy groups first: the chains of the groups whose closed-form FFD
    // runs longest start as soon as their own sort is done, while the other groups sort
    // on a second, lower-priority stream.  demand[g] = template copies the group's pods
    // need (max over cpu, memory, pod slots of sum / template free); the map
    // [heavy..., rest...] is rebuilt when the limiter's max_nodes changes.
    std::vector<double> demand;
    hipStream_t st2 = nullptr;
    hipEvent_t ev_init = nullptr, ev_b = nullptr, ev_rb = nullptr;
    DevBuf d_gmap;
    int32_t map_max_nodes = -1, n_heavy = 0;
    int32_t map_source = 0;        // 1: demand model, 2: the chains' measured times (previous run)
    int32_t res_device = -1;       // the streams and events below came from the pool of this device
    // the last run left its final pod ids in d_sched_pod (not stream positions or the parts
    // a zero-copy publisher did not need), and every group's n_scheduled: what the readers
    // of the resident lists (expander.hip) go by
    bool lists_final = false;
    std::vector<int32_t> last_nsched;
    mutable OptionSumsScratch opt_scratch;
    mutable MissingPodsScratch missing_scratch;      // nodegroupset.hip
    mutable PriceSumsScratch price_scratch;          // expander.hip
    ~ca_estimate_plan();
};

namespace casim {
// Streams and events of an Estimate plan, kept per device after the plan is destroyed and
// handed to the next plan (RunOnce builds a plan per loop: creating three streams and
// sixteen events costs more than a loop's whole Estimate).  The plan's destructor drains its
// three streams first (a run that failed part-way may have left kernels queued), so a
// released set is idle.
struct PlanStreams {
    hipStream_t pub = nullptr, st2 = nullptr, st3 = nullptr;
    hipEvent_t ev[ca_estimate_plan::EV_N] = {};
    hipEvent_t go = nullptr, pub_ev = nullptr, emitA = nullptr, emitB = nullptr, ids = nullptr, init = nullptr, b = nullptr,
               rb = nullptr;
};
static std::mutex g_ps_mu;
static std::vector<std::pair<int32_t, PlanStreams>> g_ps_pool;

static int plan_streams_acquire(int32_t dev, PlanStreams& out) {
    {
        std::lock_guard<std::mutex> lk(g_ps_mu);
        for (size_t i = 0; i < g_ps_pool.size(); i++)
            if (g_ps_pool[i].first == dev) {
                out = g_ps_pool[i].second;
                g_ps_pool.erase(g_ps_pool.begin() + (ptrdiff_t)i);
                return CA_OK;
            }
    }
    PlanStreams ps;
    for (auto& e : ps.ev) CA_HIP_CHECK(hipEventCreate(&e));
    CA_HIP_CHECK(hipEventCreateWithFlags(&ps.go, hipEventDisableTiming));
    CA_HIP_CHECK(hipEventCreateWithFlags(&ps.pub_ev, hipEventDisableTiming));
    CA_HIP_CHECK(hipEventCreateWithFlags(&ps.emitA, hipEventDisableTiming));
    CA_HIP_CHECK(hipEventCreateWithFlags(&ps.emitB, hipEventDisableTiming));
    CA_HIP_CHECK(hipEventCreateWithFlags(&ps.ids, hipEventDisableTiming));
    CA_HIP_CHECK(hipEventCreateWithFlags(&ps.init, hipEventDisableTiming));
    CA_HIP_CHECK(hipEventCreateWithFlags(&ps.b, hipEventDisableTiming));
    CA_HIP_CHECK(hipEventCreateWithFlags(&ps.rb, hipEventDisableTiming));
    CA_HIP_CHECK(hipStreamCreateWithFlags(&ps.pub, hipStreamNonBlocking));
    int lo = 0, hi = 0;
    CA_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    CA_HIP_CHECK(hipStreamCreateWithPriority(&ps.st2, hipStreamNonBlocking, lo));   // light groups: lowest
    CA_HIP_CHECK(hipStreamCreateWithPriority(&ps.st3, hipStreamNonBlocking, hi));   // Go-order sort: highest
    out = ps;
    return CA_OK;
}
}  // namespace casim

ca_estimate_plan::~ca_estimate_plan() {
    casim::PlanStreams ps;
    for (int i = 0; i < EV_N; i++) ps.ev[i] = ev[i];
    ps.go = ev_go; ps.pub_ev = ev_pub; ps.emitA = ev_emitA; ps.emitB = ev_emitB; ps.ids = ev_ids; ps.init = ev_init;
    ps.b = ev_b; ps.rb = ev_rb;
    ps.pub = pub_stream; ps.st2 = st2; ps.st3 = st3;
    // a run that returned early on an error may have left kernels queued on these streams
    // (a publisher polls for up to its deadline): drain them before the set is pooled or
    // destroyed, and before the plan's buffers go back to the allocation cache
    if (res_device >= 0) {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (cur != res_device) (void)hipSetDevice(res_device);
        for (hipStream_t q : {ps.pub, ps.st2, ps.st3}) if (q) (void)hipStreamSynchronize(q);
        if (cur >= 0 && cur != res_device) (void)hipSetDevice(cur);
    }
    if (res_device >= 0 && pub_stream && st2 && st3) {
        std::lock_guard<std::mutex> lk(casim::g_ps_mu);
        casim::g_ps_pool.emplace_back(res_device, ps);
        return;
    }
    for (auto& e : ps.ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {ps.go, ps.pub_ev, ps.emitA, ps.emitB, ps.ids, ps.init, ps.b, ps.rb}) if (e) (void)hipEventDestroy(e);
    for (hipStream_t q : {ps.pub, ps.st2, ps.st3}) if (q) (void)hipStreamDestroy(q);
}

namespace {

// The decoupled Go order runs the chains on the stable class order and takes the pod ids
// from Go's sort.Slice permutation at the same positions.  That is exact only if both
// orders hold the same class at every sorted position of a group: k_class_rank gives two
// classes with equal float64 scores one dense rank, and pdqsort interleaves their pods
// differently from list position.  So: no group may hold two classes of one score
// (binpacking_estimator.go:72-74, 164-193; same float64 operations as k_class_rank,
// -ffp-contract=off).  Per group, the U class scores against the template are sorted;
// only when a tie exists are the group's own classes looked up.
// `mark(g, seen)` sets seen[c] = g for every class c of group g's list (walked only for a
// group whose template has a tie).
bool groups_tie_free(const ca_podset* s, const std::vector<GroupMeta>& meta, const ca_template* templates,
                     const std::function<void(int32_t, std::vector<int32_t>&)>& mark) {
    const int32_t U = s->n_cls;
    if (U < 2) return true;
    std::vector<std::pair<uint64_t, int32_t>> key((size_t)U);
    std::vector<int32_t> seen((size_t)U, -1);
    std::vector<int32_t> runs;                        // classes of tied runs, -1 between runs
    for (size_t g = 0; g < meta.size(); g++) {
        const ca_template& tp = templates[meta[g].tmpl];
        const int64_t acpu = tp.node.alloc_milli_cpu, amem = tp.node.alloc_memory;
        for (int32_t c = 0; c < U; c++) {
            double score = 0.0;
            if (acpu > 0) score += (double)s->h_cls_sc[2 * c] / (double)acpu;
            if (amem > 0) score += (double)s->h_cls_sc[2 * c + 1] / (double)amem;
            uint64_t b;
            std::memcpy(&b, &score, sizeof b);
            key[c] = {b, c};
        }
        std::sort(key.begin(), key.end());
        runs.clear();
        for (int32_t i = 1; i < U; i++) {
            if (key[i].first != key[i - 1].first) continue;
            if (runs.empty() || runs.back() != key[i - 1].second) {
                if (!runs.empty()) runs.push_back(-1);
                runs.push_back(key[i - 1].second);
            }
            runs.push_back(key[i].second);
        }
        if (runs.empty()) continue;
        mark((int32_t)g, seen);
        int32_t present = 0;
        for (size_t i = 0; i <= runs.size(); i++) {
            if (i == runs.size() || runs[i] < 0) { present = 0; continue; }
            if (seen[runs[i]] == (int32_t)g && ++present >= 2) return false;
        }
    }
    return true;
}

// Sort classes of the decoupled Go order.  k_pdq_sort's permutation of a
// group is a function of its pod list and of the dense ranks of the podset's classes on its
// template, and its ids of the list alone besides: two groups with element-wise equal
// pod_idx slices and equal rank vectors over all U classes (same float64 operations and the
// same dense rank as block_class_rank) get the same ids, so one sort serves both.  rep[g] =
// the first group, in group order, of g's class (g itself when it shares with nobody);
// returns the number of classes.  Equality is exact: the signature (count, rank vector,
// a strided sample of the list) only groups the candidates, every match is a full
// comparison of the lists.  The rank vectors cost G * U log U on the host, so a batch with
// G * U above SHARE_MAX_GU keeps one sort per group.  `side` is run once, beside the
// comparisons when they go to the host's workers.  The lists are seen through `src`: a
// signature per group, the exact comparison of two groups of equal count, and what one
// comparison reads (the option form compares matrix rows instead of lists).
constexpr int64_t SHARE_MAX_GU = 1 << 17;
struct ListCompare {
    std::function<uint64_t(int32_t)> sig;               // equal lists give equal signatures
    std::function<bool(int32_t, int32_t)> same;         // the lists of two groups are element-wise equal
    std::function<size_t(int32_t)> bytes;               // bytes one comparison against group g reads
};
int32_t sort_classes(const ca_podset* s, const ListCompare& src, const std::vector<GroupMeta>& meta,
                     const ca_template* templates, std::vector<int32_t>& rep, const std::function<void()>& side) {
    const int32_t G = (int32_t)meta.size(), U = s->n_cls;
    rep.resize((size_t)G);
    for (int32_t g = 0; g < G; g++) rep[g] = g;
    if (G < 2 || (int64_t)G * std::max(U, 1) > SHARE_MAX_GU) { side(); return G; }
    // the rank vector of every distinct (cpu, memory) allocatable, then the distinct vectors
    std::map<std::pair<int64_t, int64_t>, int32_t> by_alloc;
    std::map<std::vector<int32_t>, int32_t> by_ranks;
    std::vector<int32_t> rv((size_t)G);
    std::vector<std::pair<uint64_t, int32_t>> key((size_t)U);
    std::vector<int32_t> ranks((size_t)U);
    for (int32_t g = 0; g < G; g++) {
        const ca_template& tp = templates[meta[g].tmpl];
        const int64_t acpu = tp.node.alloc_milli_cpu, amem = tp.node.alloc_memory;
        const auto it = by_alloc.find({acpu, amem});
        if (it != by_alloc.end()) { rv[g] = it->second; continue; }
        for (int32_t c = 0; c < U; c++) {
            double score = 0.0;               // calculatePodScore, as block_class_rank / groups_tie_free
            if (acpu > 0) score += (double)s->h_cls_sc[2 * c] / (double)acpu;
            if (amem > 0) score += (double)s->h_cls_sc[2 * c + 1] / (double)amem;
            if (score == 0.0) score = 0.0;    // -0 == +0 (ordered_bits)
            uint64_t b;
            std::memcpy(&b, &score, sizeof b);
            b = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
            key[c] = {~b, c};                 // ascending key == descending score
        }
        std::sort(key.begin(), key.end());
        int32_t dense = 0;
        for (int32_t i = 0; i < U; i++) {
            if (i > 0 && key[i].first != key[i - 1].first) dense++;
            ranks[key[i].second] = dense;
        }
        const int32_t id = by_ranks.emplace(ranks, (int32_t)by_ranks.size()).first->second;
        by_alloc.emplace(std::make_pair(acpu, amem), id);
        rv[g] = id;
    }
    // candidates: same count, same rank vector, same signature of the list
    std::map<std::tuple<int32_t, int32_t, uint64_t>, std::vector<int32_t>> cand;
    for (int32_t g = 0; g < G; g++) {
        cand[std::make_tuple(meta[g].count, rv[g], src.sig(g))].push_back(g);
    }
    // the first group of a bucket is a representative; the others are compared with it, every
    // pair of every bucket in one pass over the host's workers (task 0 runs `side` first: the
    // caller's list upload, which then overlaps the comparisons)
    struct Pair { int32_t head, g; size_t bytes; };
    std::vector<Pair> pairs;
    size_t pair_bytes = 0;
    for (auto& kv : cand) {
        const std::vector<int32_t>& v = kv.second;        // (ascending group order)
        const size_t bytes = src.bytes(v[0]);
        for (size_t k = 1; k < v.size(); k++) { pairs.push_back({v[0], v[k], bytes}); pair_bytes += bytes; }
    }
    std::vector<uint8_t> same(pairs.size(), 0);
    auto compare = [&](size_t k) {
        const Pair& q = pairs[k];
        same[k] = meta[q.head].count == 0 || src.same(q.head, q.g);
    };
    if (pair_bytes < ((size_t)1 << 18)) {
        side();
        for (size_t k = 0; k < pairs.size(); k++) compare(k);
    } else {
        std::atomic<size_t> next{0};
        casim::parallel_run(8, [&](int32_t t) {
            if (t == 0) side();
            for (size_t k; (k = next.fetch_add(1, std::memory_order_relaxed)) < pairs.size();) compare(k);
        });
    }
    for (size_t k = 0; k < pairs.size(); k++)
        if (same[k]) rep[pairs[k].g] = pairs[k].head;
    // a candidate unequal to its bucket's first group (the signature matched, the lists differ):
    // those go round among themselves
    int32_t classes = 0;
    for (auto& kv : cand) {
        std::vector<int32_t> v;
        for (size_t k = 0; k < kv.second.size(); k++)
            if (k == 0 || rep[kv.second[k]] == kv.second[k]) v.push_back(kv.second[k]);
        classes++;                                        // (v[0] and the groups equal to it)
        v.erase(v.begin());
        while (!v.empty()) {
            classes++;
            std::vector<int32_t> rest;
            for (size_t k = 1; k < v.size(); k++) {
                if (meta[v[0]].count == 0 || src.same(v[0], v[k])) rep[v[k]] = v[0];
                else rest.push_back(v[k]);
            }
            v.swap(rest);
        }
    }
    return classes;
}

// What plan_prepare needs from the groups' lists, from either form of them: the sort classes,
// the port / extended-resource flags, the summed requests and whether the decoupled Go order
// is exact.  lists_from_host walks the caller's lists (and queues their upload);
// lists_from_options derives the same per equivalence group and combines over the matrix rows.
struct ListFacts {
    std::vector<int32_t> sort_rep;            // empty: one sort per group
    int32_t n_classes = 0;
    std::vector<double> c, mm;                // per group: summed cpu / memory requests
    bool tie_free = false;
};

// ca_estimate_plan_create_options' inputs (validated by the entry point)
struct OptionSrc {
    const int32_t* eg_off;
    const int32_t* eg_pod;
    int32_t n_eg;
    const uint8_t* ok;
    // a ca_pod_groups handle's copies in device memory (ca_estimate_plan_create_groups): the
    // two arrays are read where they lie instead of being uploaded; NULL otherwise
    const int32_t* d_eg_off = nullptr;
    const int32_t* d_eg_pod = nullptr;
};

// shared sorts are looked for (CASIM_SORT_SHARE=0: one sort per group, for tests and A/B)
bool sort_share_wanted(const ca_estimate_plan* p, const ca_podset* s) {
    return p->bucket && s->cls_uniform && p->total > 0 &&
           !(knob_env("CASIM_SORT_SHARE") && atoi(knob_env("CASIM_SORT_SHARE")) == 0);
}

int lists_from_host(ca_estimate_plan* p, const ca_podset* s, const int32_t* group_off, const int32_t* pod_idx,
                    const ca_template* templates, int32_t G, hipStream_t st, ListFacts& lf) {
    int rc;
    const size_t tot = (size_t)std::max(p->total, 1);
    // The sort classes first (sort_classes; CASIM_SORT_SHARE=0: one sort per group, for tests
    // and A/B): groups with equal lists also share what the pass below finds, so it walks
    // each class's first group only — a comparison of two lists costs far less per item than
    // the walk's lookups.
    std::vector<int32_t>& sort_rep = lf.sort_rep;
    int32_t n_classes = G;
    // (the list upload is queued by the caller's thread beside the comparisons, or beside the
    // walk below when there are none)
    hipError_t ce = hipSuccess;
    rc = CA_OK;
    bool uploaded = false;
    auto upload = [&]() {
        if ((rc = p->d_pod_idx.reserve(sizeof(int32_t) * tot)) == CA_OK && p->total)
            ce = hipMemcpyAsync(p->d_pod_idx.ptr, pod_idx, sizeof(int32_t) * p->total, hipMemcpyHostToDevice, st);
        uploaded = true;
    };
    if (sort_share_wanted(p, s)) {
        // candidates by a strided sample of the list (few: every sample of a cold list is a
        // cache miss), every match a full comparison
        const std::vector<GroupMeta>& meta = p->h_meta;
        ListCompare lc;
        lc.sig = [&](int32_t g) {
            constexpr int32_t NS = 8;
            const int32_t n = meta[(size_t)g].count;
            const int32_t* l = pod_idx + meta[(size_t)g].off;
            uint64_t h = 0x9E3779B97F4A7C15ull;
            const int32_t step = std::max(1, n / NS);
            for (int32_t i = 0; i < n; i += step) h = (h ^ (uint32_t)l[i]) * 0x100000001B3ull;
            if (n > 0) h = (h ^ (uint32_t)l[n - 1]) * 0x100000001B3ull;
            return h;
        };
        lc.same = [&](int32_t a, int32_t b) {
            return std::memcmp(pod_idx + meta[(size_t)a].off, pod_idx + meta[(size_t)b].off,
                               sizeof(int32_t) * (size_t)meta[(size_t)a].count) == 0;
        };
        lc.bytes = [&](int32_t g) { return sizeof(int32_t) * (size_t)meta[(size_t)g].count; };
        n_classes = sort_classes(s, lc, p->h_meta, templates, sort_rep, upload);
    }
    if (n_classes == G) sort_rep.clear();
    lf.n_classes = n_classes;
    // One pass over the lists (per-pod summaries of the podset: compact arrays instead of
    // the 208-B records), split over host threads for big batches: index validation, the
    // port / extended-resource flags and each group's summed requests for the demand
    // order.  The lists travel to the device meanwhile (the caller's thread queues the copy);
    // the item classes are gathered there from the podset's class column (k_item_cls).
    {
        // the groups walked and the prefix of their counts: the walk's items, split evenly
        std::vector<int32_t> wg, woff(1, 0);
        for (int32_t g = 0; g < G; g++)
            if (sort_rep.empty() || sort_rep[g] == g) { wg.push_back(g); woff.push_back(woff.back() + p->h_meta[g].count); }
        const int32_t K = (int32_t)wg.size(), wtotal = woff.back();
        const int32_t T = std::max(1, std::min(7, wtotal / (1 << 17)));
        struct Part { bool bad = false; uint8_t fl = 0; std::vector<double> c, mm; };
        std::vector<Part> part((size_t)T);
        const bool want_fl = s->any_ports || s->any_scalar;
        auto work = [&](int32_t t) {
            Part& pt = part[(size_t)t];
            pt.c.assign((size_t)G, 0.0);
            pt.mm.assign((size_t)G, 0.0);
            const int32_t a = (int32_t)((int64_t)wtotal * t / T), b = (int32_t)((int64_t)wtotal * (t + 1) / T);
            int32_t k0 = std::max(0, (int32_t)(std::upper_bound(woff.begin(), woff.end(), a) - woff.begin()) - 1);
            const int32_t np_ = s->t.n_pods;
            const int64_t* req = s->h_req.data();
            for (int32_t v = a; v < b && !pt.bad;) {       // v: position in the walked groups' items
                while (k0 < K - 1 && woff[(size_t)k0 + 1] <= v) k0++;
                const int32_t g = wg[(size_t)k0];
                const int32_t i = group_off[g] + (v - woff[(size_t)k0]);
                const int32_t e = group_off[g] + (std::min(b, woff[(size_t)k0 + 1]) - woff[(size_t)k0]);
                double c0 = 0, c1 = 0, m0 = 0, m1 = 0;   // (two chains each: the adds pipeline)
                bool bad = false;
                int32_t k = i;
                for (; k + 1 < e; k += 2) {
                    const int32_t p0 = pod_idx[k], p1 = pod_idx[k + 1];
                    bad |= (uint32_t)p0 >= (uint32_t)np_ || (uint32_t)p1 >= (uint32_t)np_;
                    if (bad) break;
                    c0 += (double)req[2 * (size_t)p0]; m0 += (double)req[2 * (size_t)p0 + 1];
                    c1 += (double)req[2 * (size_t)p1]; m1 += (double)req[2 * (size_t)p1 + 1];
                }
                if (!bad && k < e) {
                    const int32_t p0 = pod_idx[k];
                    bad = (uint32_t)p0 >= (uint32_t)np_;
                    if (!bad) { c0 += (double)req[2 * (size_t)p0]; m0 += (double)req[2 * (size_t)p0 + 1]; }
                }
                if (bad) { pt.bad = true; break; }
                if (want_fl)
                    for (int32_t q = i; q < e; q++) pt.fl |= s->h_pflags[pod_idx[q]];
                pt.c[(size_t)g] += c0 + c1;
                pt.mm[(size_t)g] += m0 + m1;
                v += e - i;
            }
        };
        // task 0 (the caller's thread) queues the list upload if it is not queued yet,
        // tasks 1..T walk the items
        if (uploaded) casim::parallel_run(T, work);
        else casim::parallel_run(T + 1, [&](int32_t t) { if (t > 0) work(t - 1); else upload(); });
        if (rc != CA_OK) return rc;
        CA_HIP_CHECK(ce);
        bool bad = false;
        std::vector<double>& c = lf.c;
        std::vector<double>& mm = lf.mm;
        c.assign((size_t)G, 0.0);
        mm.assign((size_t)G, 0.0);
        for (const Part& pt : part) {
            bad |= pt.bad;
            if (pt.fl & 1) p->use_ports = true;
            if (pt.fl & 2) p->use_scalar = true;
            for (int32_t g = 0; g < G; g++) { c[(size_t)g] += pt.c[(size_t)g]; mm[(size_t)g] += pt.mm[(size_t)g]; }
        }
        if (bad) {
            CA_HIP_CHECK(hipStreamSynchronize(st));    // (the list copy may still read pod_idx)
            return CA_EINVAL;
        }
        for (int32_t g = 0; g < G && !sort_rep.empty(); g++) {      // equal lists, equal sums
            c[(size_t)g] = c[(size_t)sort_rep[g]];
            mm[(size_t)g] = mm[(size_t)sort_rep[g]];
        }
    }
    lf.tie_free = p->bucket && s->cls_uniform &&
                  groups_tie_free(s, p->h_meta, templates, [&](int32_t g, std::vector<int32_t>& seen) {
                      const GroupMeta& gm = p->h_meta[(size_t)g];
                      for (int32_t i = gm.off; i < gm.off + gm.count; i++) seen[s->h_cls[pod_idx[i]]] = g;
                  });
    return CA_OK;
}

// The same facts without the lists.  Every one of them is a per-equivalence-group quantity
// combined over a matrix row: each group is walked once (O(pending pods)), then the rows are
// combined in O(G * n_eg).  An empty equivalence group adds nothing to a list, so it counts as
// failing everywhere: two rows then give equal lists exactly when they agree on every
// non-empty group (the groups are disjoint), which is what the sort classes compare.  The
// float64 request sums are taken in another order than the item walk's; they only feed the
// demand order, which no result depends on.
int lists_from_options(ca_estimate_plan* p, const ca_podset* s, const OptionSrc& o, const ca_template* templates,
                       int32_t G, ListFacts& lf) {
    const int32_t E = o.n_eg, U = s->n_cls;
    const bool want_fl = s->any_ports || s->any_scalar;
    const bool want_cls = p->bucket && s->cls_uniform && U >= 2;          // (groups_tie_free's readers)
    std::vector<int32_t> len((size_t)E), cl_off(1, 0), cl, stamp(want_cls ? (size_t)U : 0, -1);
    std::vector<uint8_t> fl((size_t)E, 0);
    std::vector<double> ec((size_t)E), em((size_t)E);
    const int64_t* req = s->h_req.data();
    for (int32_t e = 0; e < E; e++) {
        const int32_t a = o.eg_off[e], b = o.eg_off[e + 1];
        len[(size_t)e] = b - a;
        double c0 = 0, m0 = 0;
        uint8_t f = 0;
        for (int32_t i = a; i < b; i++) {
            const size_t pod = (size_t)o.eg_pod[i];
            c0 += (double)req[2 * pod];
            m0 += (double)req[2 * pod + 1];
            if (want_fl) f |= s->h_pflags[pod];
            if (want_cls) {
                const int32_t c = s->h_cls[pod];
                if (stamp[(size_t)c] != e) { stamp[(size_t)c] = e; cl.push_back(c); }
            }
        }
        ec[(size_t)e] = c0; em[(size_t)e] = m0; fl[(size_t)e] = f;
        cl_off.push_back((int32_t)cl.size());
    }
    lf.c.assign((size_t)G, 0.0);
    lf.mm.assign((size_t)G, 0.0);
    std::vector<uint64_t> sig((size_t)G);
    const int32_t T = (int32_t)std::max<int64_t>(1, std::min<int64_t>(std::min(7, G), (int64_t)G * E / (1 << 19)));
    std::vector<uint8_t> tfl((size_t)T, 0);
    casim::parallel_run(T, [&](int32_t t) {
        uint8_t f = 0;
        for (int32_t g = (int32_t)((int64_t)G * t / T); g < (int32_t)((int64_t)G * (t + 1) / T); g++) {
            const uint8_t* row = o.ok + (size_t)g * (size_t)E;
            double c = 0, m = 0;
            uint64_t h = 0x9E3779B97F4A7C15ull;
            for (int32_t e = 0; e < E; e++)
                if (row[e] && len[(size_t)e]) {
                    c += ec[(size_t)e]; m += em[(size_t)e]; f |= fl[(size_t)e];
                    h = (h ^ (uint32_t)e) * 0x100000001B3ull;
                }
            lf.c[(size_t)g] = c; lf.mm[(size_t)g] = m; sig[(size_t)g] = h;
        }
        tfl[(size_t)t] = f;
    });
    for (uint8_t f : tfl) {
        if (f & 1) p->use_ports = true;
        if (f & 2) p->use_scalar = true;
    }
    int32_t n_classes = G;
    if (sort_share_wanted(p, s)) {
        ListCompare lc;
        lc.sig = [&](int32_t g) { return sig[(size_t)g]; };
        lc.same = [&](int32_t a, int32_t b) {
            const uint8_t* ra = o.ok + (size_t)a * (size_t)E;
            const uint8_t* rb = o.ok + (size_t)b * (size_t)E;
            for (int32_t e = 0; e < E; e++)
                if (((ra[e] != 0) != (rb[e] != 0)) && len[(size_t)e]) return false;
            return true;
        };
        lc.bytes = [&](int32_t) { return (size_t)E; };
        n_classes = sort_classes(s, lc, p->h_meta, templates, lf.sort_rep, []() {});
    }
    if (n_classes == G) lf.sort_rep.clear();
    lf.n_classes = n_classes;
    lf.tie_free = p->bucket && s->cls_uniform &&
                  groups_tie_free(s, p->h_meta, templates, [&](int32_t g, std::vector<int32_t>& seen) {
                      const uint8_t* row = o.ok + (size_t)g * (size_t)E;
                      for (int32_t e = 0; e < E; e++)
                          if (row[e])
                              for (int32_t k = cl_off[(size_t)e]; k < cl_off[(size_t)e + 1]; k++) seen[(size_t)cl[(size_t)k]] = g;
                  });
    return CA_OK;
}

// Plan creation: the group records and streams, the facts of the lists (from the caller's
// lists or from the option matrix), then the common tail: demand order, sort sharing,
// buffers, fan map and uploads.  opt != NULL: group_off was derived from the matrix, pod_idx
// is NULL and the lists are built on the device (k_option_lists).
int plan_queue_first_sort(ca_estimate_plan* p);      // (below, with the run's sort helpers)
int plan_prepare(ca_estimate_plan* p, ca_mirror* m, const ca_podset* s, const int32_t* group_off,
                 const int32_t* pod_idx, const OptionSrc* opt, const ca_template* templates, int32_t G) {
    p->m = m; p->s = s; p->G = G;
    {
        PlanStreams ps;                      // (pooled per device: plan_streams_acquire)
        int rc0;
        if ((rc0 = plan_streams_acquire(m->device, ps)) != CA_OK) return rc0;
        for (int i = 0; i < ca_estimate_plan::EV_N; i++) p->ev[i] = ps.ev[i];
        p->ev_go = ps.go; p->ev_pub = ps.pub_ev; p->ev_emitA = ps.emitA; p->ev_emitB = ps.emitB; p->ev_ids = ps.ids;
        p->ev_init = ps.init; p->ev_b = ps.b; p->ev_rb = ps.rb;
        p->pub_stream = ps.pub; p->st2 = ps.st2; p->st3 = ps.st3;
        p->res_device = m->device;
    }
    {
        int rc0;
        if ((rc0 = p->h_out.reserve(sizeof(ChainOut) * (size_t)std::max(G, 1))) != CA_OK) return rc0;
        if ((rc0 = p->h_qc.reserve(sizeof(int32_t) * 5)) != CA_OK) return rc0;
    }
    p->h_off.assign(group_off, group_off + G + 1);
    p->h_tmpl.assign(templates, templates + G);
    p->total = group_off[G] - group_off[0];
    if (group_off[0] != 0) return CA_EINVAL;
    p->h_meta.resize(G);
    p->max_count = 0;
    p->n_masks = 0;
    p->n_tiles = 0;
    p->n_hist = 0;
    p->max_rtiles = 0;
    p->f64_exact = s->req_below_2p53;
    {
        const char* e = knob_env("CASIM_SORT");      // "merge" forces the comparison sort (tests run both)
        p->bucket = s->n_cls <= CLS_MAX && !(e && strcmp(e, "merge") == 0);
    }
    for (int32_t g = 0; g < G; g++) {
        const int32_t c = group_off[g + 1] - group_off[g];
        if (c < 0) return CA_EINVAL;
        GroupMeta& gm = p->h_meta[g];
        const ca_template& t = templates[g];
        gm.tcpu = wsub(t.node.alloc_milli_cpu, t.used_milli_cpu);
        gm.tmem = wsub(t.node.alloc_memory, t.used_memory);
        gm.teph = wsub(t.node.alloc_ephemeral, t.used_ephemeral);
        gm.tpods = clamp_i32(t.node.alloc_pods - t.used_pods);
        if (std::max(gm.tcpu, std::max(gm.tmem, gm.teph)) >= (1ll << 53)) p->f64_exact = false;   // (run_div's bound)
        gm.off = group_off[g];
        gm.count = c;
        gm.tmpl = g;
        gm.tflags = t.node.flags;
        gm.moff = p->n_masks;
        gm.ids_off = gm.off;
        gm.rtiles = (c + RT - 1) / RT;
        gm.hoff = p->n_hist;
        gm.ids_grp = g;
        p->n_hist += 256 * gm.rtiles;
        p->max_rtiles = std::max(p->max_rtiles, gm.rtiles);
        p->n_masks += (c + 63) / 64;
        p->max_count = std::max(p->max_count, c);
        for (int w = 0; w < CA_PORT_WORDS; w++) if (t.used_ports[w]) p->use_ports = true;
        for (int i = 0; i < CA_MAX_SCALAR; i++)
            if (t.node.alloc_scalar[i] || t.used_scalar[i]) p->use_scalar = true;
    }
    hipStream_t st = m->stream;
    int rc;
    const size_t tot = (size_t)std::max(p->total, 1);
    ListFacts lf;
    rc = opt ? lists_from_options(p, s, *opt, templates, G, lf)
             : lists_from_host(p, s, group_off, pod_idx, templates, G, st, lf);
    if (rc != CA_OK) return rc;
    const std::vector<int32_t>& sort_rep = lf.sort_rep;
    const int32_t n_classes = lf.n_classes;
    p->demand.assign(G, 0.0);
    for (int32_t g = 0; g < G; g++) {
        const GroupMeta& gm = p->h_meta[g];
        double d = gm.tpods > 0 ? (double)gm.count / gm.tpods : 0.0;
        if (gm.tcpu > 0) d = std::max(d, lf.c[(size_t)g] / (double)gm.tcpu);
        if (gm.tmem > 0) d = std::max(d, lf.mm[(size_t)g] / (double)gm.tmem);
        p->demand[g] = d;
    }
    p->decouple_ok = lf.tie_free;
    // decoupled: one Go-order sort per sort class; the members read their representative's ids
    // and wait on its ready flag
    p->n_sorts = G;
    std::vector<int32_t> sort_map;                    // (alive until the uploads below are done)
    if (p->decouple_ok && !sort_rep.empty()) {
        p->n_sorts = n_classes;
        {
            for (int32_t g = 0; g < G; g++) {
                p->h_meta[g].ids_grp = sort_rep[g];
                p->h_meta[g].ids_off = p->h_meta[sort_rep[g]].off;
                if (sort_rep[g] == g) sort_map.push_back(g);
            }
        }
    }
    if ((rc = p->d_meta.reserve(sizeof(GroupMeta) * (size_t)std::max(G, 1) + sizeof(int32_t) * sort_map.size())) != CA_OK)
        return rc;
    if (!sort_map.empty())
        CA_HIP_CHECK(hipMemcpyAsync(p->d_meta.as<GroupMeta>() + G, sort_map.data(), sizeof(int32_t) * sort_map.size(),
                                    hipMemcpyHostToDevice, st));
    if ((rc = p->d_tmpl.reserve(sizeof(ca_template) * (size_t)std::max(G, 1))) != CA_OK) return rc;
    if ((rc = p->d_sortA.reserve(sizeof(SortItem) * tot)) != CA_OK) return rc;
    if ((rc = p->d_sortB.reserve(sizeof(SortItem) * tot)) != CA_OK) return rc;
    if ((rc = p->d_stream.reserve(sizeof(StreamPod) * tot)) != CA_OK) return rc;
    if ((rc = p->d_heads.reserve(sizeof(uint64_t) * (size_t)std::max(p->n_masks, 1))) != CA_OK) return rc;
    if ((rc = p->d_spod.reserve(sizeof(int32_t) * tot)) != CA_OK) return rc;
    if ((rc = p->d_seg.reserve(sizeof(Seg) * tot)) != CA_OK) return rc;
    {
        const char* so = knob_env("CASIM_SORT_ORDER");                 // (go_sort_order(), below)
        const bool go_ord = !(so && strcmp(so, "stable") == 0);
        p->pch = (p->decouple_ok && go_ord) ? PCH_DECOUPLED : PCH;
    }
    if (const char* e = knob_env("CASIM_PUB_CHUNK")) p->pch = std::max(1, atoi(e));
    const int32_t pch = p->pch;
    p->n_tickets = 0;
    for (int32_t g = 0; g < G; g++) p->n_tickets += (p->h_meta[g].count + pch - 1) / pch;
    p->nsub = std::max(1, (p->max_count + pch - 1) / pch);
    if ((rc = p->d_tickets.reserve(sizeof(int64_t) * (size_t)std::max(p->n_tickets, 1))) != CA_OK) return rc;
    if ((int64_t)G * p->nsub < INT32_MAX &&
        (rc = p->d_prog.reserve(sizeof(int2) * (size_t)G * (size_t)p->nsub)) != CA_OK) return rc;
    if ((rc = p->d_qctl.reserve(sizeof(int32_t) * 6)) != CA_OK) return rc;
    if ((rc = p->d_unsup.reserve(sizeof(uint32_t) * (size_t)std::max(G, 1))) != CA_OK) return rc;
    if ((rc = p->d_lin.reserve(sizeof(int32_t) * (size_t)std::max(G, 1))) != CA_OK) return rc;
    if ((rc = p->d_need.reserve((size_t)std::max(G, 1))) != CA_OK) return rc;
    if ((rc = p->d_out.reserve(sizeof(ChainOut) * (size_t)std::max(G, 1))) != CA_OK) return rc;
    if ((rc = p->d_sched_pod.reserve(sizeof(int32_t) * tot)) != CA_OK) return rc;
    if ((rc = p->d_sched_node.reserve(sizeof(int32_t) * tot)) != CA_OK) return rc;
    if (p->bucket) {
        if ((rc = p->d_crank.reserve(sizeof(int32_t) * (size_t)std::max(G, 1) * (size_t)std::max(s->n_cls, 1))) != CA_OK)
            return rc;
        if ((rc = p->d_hist.reserve(sizeof(int32_t) * (size_t)std::max(p->n_hist, 1))) != CA_OK) return rc;
    }
    if ((rc = p->d_pdq_e.reserve(sizeof(uint64_t) * tot)) != CA_OK) return rc;
    if ((rc = p->d_pdq_scr.reserve(sizeof(uint64_t) * tot)) != CA_OK) return rc;
    if ((rc = p->d_pdq_stack.reserve(sizeof(pdq::Frame) * (tot / 2 + 2 * (size_t)std::max(G, 1) + 2))) != CA_OK)
        return rc;
    if (!p->bucket && (rc = p->d_item_rank.reserve(sizeof(uint32_t) * tot)) != CA_OK) return rc;
    if (p->decouple_ok) {
        if ((rc = p->d_sortC.reserve(sizeof(uint32_t) * tot)) != CA_OK) return rc;
        if ((rc = p->d_spod_go.reserve(sizeof(int32_t) * tot)) != CA_OK) return rc;
        const size_t fan_words = (size_t)pdq::FAN_STRIDE * (size_t)std::max(G, 1);
        if ((rc = p->d_ids_ready.reserve(sizeof(int32_t) * fan_words)) != CA_OK) return rc;
        CA_HIP_CHECK(hipMemset(p->d_ids_ready.ptr, 0, sizeof(int32_t) * fan_words));   // epoch 0: none
        p->ids_epoch = 0;
        // (test hook: the first sorts' epochs cross the wrap at INT32_MAX)
        if (test_hook_env("CASIM_IDS_EPOCH_NEAR_WRAP")) p->ids_epoch = INT32_MAX - 1;
        // Defaults from profiles/sort_fan_ab.txt; knobs are read here, once
        fan_knobs(&p->fan_parts, &p->fan_min, &p->fan_steps);
        std::vector<int32_t> fan_map;
        for (int32_t g = 0; g < G && p->fan_parts > 0; g++)
            if (p->h_meta[g].ids_grp == g && p->h_meta[g].count > p->fan_min && p->h_meta[g].count <= PDQ_LDS_N)
                fan_map.push_back(g);
        p->n_fan = (int32_t)fan_map.size();
        if (p->n_fan > 0) {
            if ((rc = p->d_fan_map.reserve(sizeof(int32_t) * fan_map.size())) != CA_OK) return rc;
            CA_HIP_CHECK(hipMemcpy(p->d_fan_map.ptr, fan_map.data(), sizeof(int32_t) * fan_map.size(), hipMemcpyHostToDevice));
            if ((rc = p->d_pdq_pstack.reserve(sizeof(pdq::Frame) *
                                              (tot / 2 + 2 * (size_t)pdq::FAN_PARTS_MAX * (size_t)std::max(G, 1) + 4))) != CA_OK)
                return rc;
        }
        if ((rc = p->d_crank2.reserve(sizeof(int32_t) * (size_t)std::max(G, 1) * (size_t)std::max(s->n_cls, 1))) != CA_OK)
            return rc;
        if ((rc = p->d_rstart.reserve(sizeof(int32_t) * (size_t)std::max(G, 1) * (size_t)(s->n_cls + 1))) != CA_OK)
            return rc;
        if ((rc = p->d_rsp.reserve(sizeof(StreamPod) * (size_t)std::max(G, 1) * (size_t)std::max(s->n_cls, 1))) != CA_OK)
            return rc;
        if ((rc = p->d_rdiv.reserve(sizeof(double) * RDIV_N * (size_t)std::max(G, 1) * (size_t)std::max(s->n_cls, 1))) != CA_OK)
            return rc;
    }
    if (G) CA_HIP_CHECK(hipMemcpyAsync(p->d_meta.ptr, p->h_meta.data(), sizeof(GroupMeta) * G, hipMemcpyHostToDevice, st));
    // the lists as (pod, class) pairs: the class of every item next to its pod index, so
    // the sorts and the run table read it in one coalesced load instead of two gathers
    p->has_cls_cnt = p->bucket && s->cls_uniform && p->total > 0;
    if (p->bucket && p->total > 0 &&
        (rc = p->d_item_cls.reserve(sizeof(int32_t) * ((size_t)p->total + (p->has_cls_cnt ? (size_t)G * (size_t)s->n_cls : 0)))) != CA_OK)
        return rc;
    DevBuf d_eg_off, d_eg_pod, d_ok, d_chunk_pre;      // option form: alive until the stream is drained below
    if (opt) {
        // the lists are built in HBM from the equivalence groups and the matrix: 4 B per
        // pending pod and 1 B per pair go up instead of 4 B per item
        if ((rc = p->d_pod_idx.reserve(sizeof(int32_t) * tot)) != CA_OK) return rc;
        if (p->total > 0) {
            const int32_t E = opt->n_eg, nch = (E + OPT_CHUNK - 1) / OPT_CHUNK;
            const size_t n_egp = (size_t)opt->eg_off[E];
            const int32_t* eg_off_d = opt->d_eg_off;
            const int32_t* eg_pod_d = opt->d_eg_pod;
            if (!eg_off_d) {
                if ((rc = d_eg_off.reserve(sizeof(int32_t) * ((size_t)E + 1))) != CA_OK) return rc;
                if ((rc = d_eg_pod.reserve(sizeof(int32_t) * n_egp)) != CA_OK) return rc;
                CA_HIP_CHECK(hipMemcpyAsync(d_eg_off.ptr, opt->eg_off, sizeof(int32_t) * ((size_t)E + 1), hipMemcpyHostToDevice, st));
                CA_HIP_CHECK(hipMemcpyAsync(d_eg_pod.ptr, opt->eg_pod, sizeof(int32_t) * n_egp, hipMemcpyHostToDevice, st));
                eg_off_d = d_eg_off.as<int32_t>();
                eg_pod_d = d_eg_pod.as<int32_t>();
            }
            if ((rc = d_ok.reserve((size_t)G * (size_t)E)) != CA_OK) return rc;
            if ((rc = d_chunk_pre.reserve(sizeof(int32_t) * (size_t)G * (size_t)nch)) != CA_OK) return rc;
            CA_HIP_CHECK(hipMemcpyAsync(d_ok.ptr, opt->ok, (size_t)G * (size_t)E, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_option_chunks, dim3(G), dim3(256), 0, st, eg_off_d, d_ok.as<uint8_t>(), E, nch,
                               d_chunk_pre.as<int32_t>());
            CA_HIP_CHECK(hipGetLastError());
            if (p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_START], st));
            hipLaunchKernelGGL(k_option_lists, dim3((p->max_count + OPT_TILE - 1) / OPT_TILE, G), dim3(256), 0, st,
                               p->d_meta.as<GroupMeta>(), eg_off_d, eg_pod_d, d_ok.as<uint8_t>(),
                               E, nch, d_chunk_pre.as<int32_t>(), s->d_cls.as<int32_t>(), p->d_pod_idx.as<int32_t>(),
                               p->bucket ? p->d_item_cls.as<int32_t>() : nullptr);
            CA_HIP_CHECK(hipGetLastError());
            if (p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_SCORE], st));
        }
    } else if (p->bucket && p->total > 0) {
        const int32_t nb = (int32_t)std::min<int64_t>(4096, (p->total + 255) / 256);
        hipLaunchKernelGGL(k_item_cls, dim3(nb), dim3(256), 0, st, p->d_pod_idx.as<int32_t>(),
                           s->d_cls.as<int32_t>(), p->d_item_cls.as<int32_t>(), p->total);
        CA_HIP_CHECK(hipGetLastError());
    }
    // the class counts of every list, behind whichever kernel wrote the classes: plans that
    // can take the run-table path (k_run_table reads them in every run)
    if (p->has_cls_cnt) {
        CA_HIP_CHECK(hipMemsetAsync(p->cls_cnt(), 0, sizeof(int32_t) * (size_t)G * (size_t)s->n_cls, st));
        hipLaunchKernelGGL(k_cls_hist, dim3((p->max_count + CLS_HIST_TILE - 1) / CLS_HIST_TILE, G), dim3(256), 0, st,
                           p->d_meta.as<GroupMeta>(), p->d_item_cls.as<int32_t>(), s->n_cls, p->cls_cnt());
        CA_HIP_CHECK(hipGetLastError());
    }
    if (G) CA_HIP_CHECK(hipMemcpyAsync(p->d_tmpl.ptr, templates, sizeof(ca_template) * G, hipMemcpyHostToDevice, st));
    CA_HIP_CHECK(hipStreamSynchronize(st));
    if (opt && p->total > 0 && p->phase_events)
        CA_HIP_CHECK(hipEventElapsedTime(&p->opt_lists_ms, p->ev[ca_estimate_plan::EV_START], p->ev[ca_estimate_plan::EV_SCORE]));
    // (the option form's inputs go back to the allocation cache before the sort is queued: a
    // release synchronises the device and would wait for it)
    for (DevBuf* b : {&d_eg_off, &d_eg_pod, &d_ok, &d_chunk_pre}) b->release();
    // the Go-order ids are plan state: sorted here once, behind the lists (host lists or
    // k_option_lists), and again only by a run whose settings differ
    return plan_queue_first_sort(p);
}

// how long a publisher waits for the first chain of its batch to start (100 MHz ticks):
// the chains are launched just before it, so a chain not running by then means the two
// kernels were serialised (CASIM_PUB_START_US overrides; default 2 ms)
uint64_t pub_start_ticks() {
    const char* e = knob_env("CASIM_PUB_START_US");
    const long us = e ? std::max(1L, atol(e)) : 2000L;
    return (uint64_t)us * 100ull;
}

__global__ void k_narrow16(const int32_t* __restrict__ src, uint16_t* __restrict__ dst, int32_t n) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (uint16_t)src[i];
}

// the plan's device results (sched_pod layout) into the caller's buffer: int32 ids, or
// 16-bit ids narrowed on the device first (stream-ordered copies)
int results_to_host(ca_estimate_plan* p, hipStream_t st, int32_t* sched_pod, uint16_t* sched16) {
    const int32_t n = std::max(p->total, 0);
    if (!sched16) {
        CA_HIP_CHECK(hipMemcpyAsync(sched_pod, p->d_sched_pod.ptr, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        return CA_OK;
    }
    int rc;
    if ((rc = p->d_sched16.reserve(sizeof(uint16_t) * (size_t)std::max(n, 1))) != CA_OK) return rc;
    if (n > 0) {
        hipLaunchKernelGGL(k_narrow16, dim3((n + 255) / 256), dim3(256), 0, st, p->d_sched_pod.as<int32_t>(),
                           p->d_sched16.as<uint16_t>(), n);
        CA_HIP_CHECK(hipGetLastError());
        CA_HIP_CHECK(hipMemcpyAsync(sched16, p->d_sched16.ptr, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, st));
    }
    return CA_OK;
}

// Estimate's tie order: Go 1.19 sort.Slice (the reference, default) or, with
// CASIM_SORT_ORDER=stable, ties by list position (the radix / merge paths alone)
bool go_sort_order() {
    const char* e = knob_env("CASIM_SORT_ORDER");
    return !(e && strcmp(e, "stable") == 0);
}

// k_pdq_sort for `ng` groups (map gm) into d_sortA: ranks from the class ranks (crank, U)
// or from item_rank
int launch_pdq_sort(ca_estimate_plan* p, hipStream_t ss, const int32_t* gm, int32_t ng, const int32_t* crank,
                    int32_t U, const uint32_t* item_rank, int32_t force = 0, uint32_t* out = nullptr,
                    int32_t* ids_out = nullptr, int32_t* ids_ready = nullptr, int32_t ids_epoch = 0,
                    int32_t fold_np = 0) {
    const int32_t lds_n = std::min(p->max_count, PDQ_LDS_N);
    const size_t lds = pdq_lds_bytes(lds_n);
    int rc;
    if ((rc = ensure_dyn_lds((const void*)k_pdq_sort, lds)) != CA_OK) return rc;
    // the decoupled path's sorts (ids_ready: the fan table) fan out over part workgroups
    const bool fan = ids_out && ids_ready && p->fan_parts > 0 && p->n_fan > 0;
    hipLaunchKernelGGL(k_pdq_sort, dim3(ng), dim3(pdq::NT), lds, ss, p->d_meta.as<GroupMeta>(),
                       p->d_pod_idx.as<int32_t>(), p->s ? p->s->d_cls.as<int32_t>() : nullptr, crank, U, item_rank,
                       out ? out : p->d_sortA.as<uint32_t>(), p->d_pdq_e.as<uint64_t>(), p->d_pdq_scr.as<uint64_t>(),
                       p->d_pdq_stack.as<pdq::Frame>(), lds_n, force, 0, gm, ids_out, ids_ready, ids_epoch,
                       (p->bucket && crank && !item_rank) ? p->d_item_cls.as<int32_t>() : nullptr,
                       p->d_tmpl.as<ca_template>(), fold_np > 0 ? p->s->d_cls_sc.as<int64_t>() : nullptr, fold_np,
                       fan ? p->fan_parts : 0, p->fan_min, p->fan_steps);
    CA_HIP_CHECK(hipGetLastError());
    if (fan) {
        if ((rc = ensure_dyn_lds((const void*)k_pdq_sort_parts, lds)) != CA_OK) return rc;
        hipLaunchKernelGGL(k_pdq_sort_parts, dim3(p->fan_parts, p->n_fan), dim3(pdq::NT), lds, ss,
                           p->d_meta.as<GroupMeta>(), p->d_pod_idx.as<int32_t>(), (uint32_t*)nullptr,
                           p->d_pdq_e.as<uint64_t>(), p->d_pdq_stack.as<pdq::Frame>(), p->d_pdq_pstack.as<pdq::Frame>(),
                           lds_n, p->d_fan_map.as<int32_t>(), ids_out, ids_ready, ids_epoch);
        CA_HIP_CHECK(hipGetLastError());
    }
    if (fan) p->ran_fan = 1;
    return CA_OK;
}

// The decoupled path's Go-order sort: the class ranks inside the sort kernel when its LDS has
// room for the scratch (*NP: the padded class count), else k_class_rank ahead of it
bool go_sort_fold(const ca_estimate_plan* p, int32_t* NP) {
    const int32_t U = p->s->n_cls;
    int32_t np2 = 1;
    while (np2 < U) np2 <<= 1;
    *NP = np2;
    const size_t npad = ((size_t)std::min(p->max_count, PDQ_LDS_N) + 63) & ~(size_t)63;
    return 16 * (size_t)np2 <= 3 * npad && 2 * (size_t)U <= npad / 8 && !knob_env("CASIM_NO_RANK_FOLD");
}

// the settings a decoupled run sorts under (sort_reuse_host.h); the fan settings and the sort
// classes are fixed at creation, the rank fold and the tie order are read per run
GoSortKey go_sort_key(const ca_estimate_plan* p, bool decoupled, bool fold) {
    GoSortKey k;
    k.fan_parts = p->fan_parts; k.fan_min = p->fan_min; k.fan_steps = p->fan_steps;
    k.n_sorts = p->n_sorts;
    k.decoupled = decoupled ? 1 : 0;
    k.fold = fold ? 1 : 0;
    k.fanned = p->fan_parts > 0 && p->n_fan > 0 ? 1 : 0;
    k.go_order = go_sort_order() ? 1 : 0;
    return k;
}

// a new epoch for the sort about to be queued on st3 (wrapped: start over from a clean table)
int go_sort_new_epoch(ca_estimate_plan* p) {
    bool wrapped = false;
    const int32_t next = go_sort_next_epoch(p->ids_epoch, &wrapped);
    if (wrapped)
        CA_HIP_CHECK(hipMemsetAsync(p->d_ids_ready.ptr, 0, sizeof(int32_t) * (size_t)pdq::FAN_STRIDE * (size_t)p->G, p->st3));
    p->ids_epoch = next;
    p->ids_done = false;
    return CA_OK;
}

// Go's sort.Slice permutation of every sort class and its pod ids, on st3 under p->ids_epoch:
// one workgroup per sort class (its representative group); the other members' consumers read
// the representative's slice of d_spod_go and its ready flag (GroupMeta::ids_off / ids_grp)
int queue_go_sort(ca_estimate_plan* p, bool fold, int32_t NP) {
    const int32_t G = p->G, U = p->s->n_cls;
    const int32_t ns = p->n_sorts;
    const int32_t* smap = ns < G ? reinterpret_cast<const int32_t*>(p->d_meta.as<GroupMeta>() + G) : nullptr;
    p->ran_sorts = ns;
    if (!fold) {
        hipLaunchKernelGGL(k_class_rank, dim3(ns), dim3(1024), 0, p->st3, p->d_meta.as<GroupMeta>(),
                           p->d_tmpl.as<ca_template>(), p->s->d_cls_sc.as<int64_t>(), U, NP,
                           p->d_crank2.as<int32_t>(), smap);
        CA_HIP_CHECK(hipGetLastError());
    }
    return launch_pdq_sort(p, p->st3, smap, ns, p->d_crank2.as<int32_t>(), U, nullptr, 0,
                           p->d_sortC.as<uint32_t>(), p->d_spod_go.as<int32_t>(),
                           p->d_ids_ready.as<int32_t>(), p->ids_epoch, fold ? NP : 0);
}

// CASIM_SORT_REUSE=0 (read per run): every decoupled run sorts again (tests, A/B)
bool sort_reuse_on() {
    const char* e = knob_env("CASIM_SORT_REUSE");
    return !(e && atoi(e) == 0);
}

// Plan creation (after the lists, classes and templates are on the device and m->stream is
// drained): the sort a default run would launch, queued on st3 so that the first run behaves
// like every later one.  Nothing waits for it here; a run that finds it still in flight has
// its publisher wait part by part, and the other consumers wait for ev_ids.  An asynchronous
// error surfaces at that run's hipEventQuery(ev_ids).
int plan_queue_first_sort(ca_estimate_plan* p) {
    const bool decoupled = go_sort_order() && p->decouple_ok && p->total > 0 &&
                           !(knob_env("CASIM_GO_DECOUPLE") && atoi(knob_env("CASIM_GO_DECOUPLE")) == 0);
    if (!decoupled || !sort_reuse_on()) return CA_OK;
    int32_t NP = 1;
    const bool fold = go_sort_fold(p, &NP);
    int rc;
    if ((rc = go_sort_new_epoch(p)) != CA_OK) return rc;
    p->ran_fan = 0;
    if ((rc = queue_go_sort(p, fold, NP)) != CA_OK) return rc;
    CA_HIP_CHECK(hipEventRecord(p->ev_ids, p->st3));
    p->ids.valid = true;
    p->ids.epoch = p->ids_epoch;
    p->ids.key = go_sort_key(p, true, fold);
    p->ids_sorts = p->ran_sorts;
    p->ids_fan = p->ran_fan;
    return CA_OK;
}

int32_t pub_blocks(bool decoupled, bool table_chain) {
    const char* e = knob_env("CASIM_PUB_BLOCKS");
    // scripts/pub_sweep.sh on C2: stable order 32 x 4096-output chunks; decoupled Go order
    // 128 x 8192 in round 4 (each group's ids are ready when its own sort ends, from ~0.17 ms
    // on; more blocks in flight keep a block waiting on a late group from holding up the
    // ready ones — 0.474 against 0.478 ms for 64 x 16384, interleaved repeats,
    // scripts/gpu_pubsweep2.sh); with round 6's chains and sort, 64 x 16384 (A/Bs of variant
    // builds: profiles/r06_pub_chunk_ab.txt, r06_pub_blocks_ab.txt); with the run-table chain
    // the publisher's tail behind the sort ends the step, not the chains: 128 blocks
    // (profiles/table_chain_ab.txt: 0.4396 against 0.4423 ms for 64, 0.4411 for 256); with the
    // sort out of the step (the plan's stored ids) 32 blocks read 0.008-0.011 ms less in every
    // round of three comparisons, under three times the 128-block rounds' own range: 128 stays
    // (profiles/sort_reuse_ab.txt)
#ifndef CASIM_PUB_BLOCKS_DECOUPLED
#define CASIM_PUB_BLOCKS_DECOUPLED 64
#endif
    return e ? std::max(1, atoi(e)) : (table_chain ? 128 : decoupled ? CASIM_PUB_BLOCKS_DECOUPLED : 32);
}

// The run-table chain's table of a podset with U score classes (k_ffd_chain<.., TB>): a
// 32-B record and a first position per rank, and the list of (rank, first position) of
// the ranks that start a run.
// lean: and the rank's float64 requests and reciprocals (48 B) behind its record, and its copy
// count on a fresh template copy (4 B).
size_t chain_table_bytes(int32_t U, bool lean = false) {
    return ((sizeof(StreamPod) + (lean ? 6 * sizeof(double) + sizeof(int32_t) : 0)) * (size_t)U +
            (sizeof(int2) + sizeof(int32_t)) * ((size_t)U + 1) + 15) & ~(size_t)15;
}
// table_ranks >= 0: with the run table of that many classes behind the rows (which start
// 16-byte aligned: the table's offset is the size without it)
size_t chain_lds_bytes(int32_t kcap, bool use_ports, bool use_scalar, int32_t table_ranks = -1, bool lean = false) {
    const size_t nb = (size_t)((kcap + 63) >> 6);
    size_t b = 32 * ((size_t)kcap + nb) + 8 * (size_t)kcap;   // rows, summaries, CAPA + ALIVE
    if (use_ports) b += 8 * CA_PORT_WORDS * (size_t)kcap;
    if (use_scalar) b += 8 * CA_MAX_SCALAR * (size_t)kcap;
    b = (b + 15) & ~(size_t)15;
    if (table_ranks >= 0) b += chain_table_bytes(table_ranks, lean);
    return b;
}

int plan_run(ca_estimate_plan* p, const ca_limiter* lim, int32_t* last_index, ca_estimate_result* results,
             int32_t* sched_pod, int32_t* sched_node, uint16_t* sched16 = nullptr) {
    ca_mirror* m = p->m;
    hipStream_t st = m->stream;
    const int32_t G = p->G;
    if (!lim || !last_index || !results) return CA_EINVAL;
    // sched_pod == NULL: the scheduled pods stay in device memory (ca_estimate_plan_fetch /
    // ca_estimate_plan_device_results); no node ordinals then
    const bool to_host = sched_pod != nullptr || sched16 != nullptr;
    if (!to_host && sched_node) return CA_EINVAL;
    // 16-bit results: pod ids of a podset of at most 65535 pods (0xFFFF: not scheduled)
    if (sched16 && (sched_pod || sched_node || p->s->n_host > 65535)) return CA_EINVAL;
    p->pub_state = 0;
    p->lists_final = false;
    const auto t_start = std::chrono::steady_clock::now();
    // CASIM_STEP_TIMING (read once per process): host-side split of the steps, averaged over
    // 20 calls — entry to the first launch, to the last launch, to the join, to the return,
    // and the caller's time between a return and the next entry
    static const bool step_timing = knob_env("CASIM_STEP_TIMING") != nullptr;
    static double st_acc[6] = {0, 0, 0, 0, 0, 0};
    static int st_n = 0;
    static std::chrono::steady_clock::time_point st_last_exit;
    std::chrono::steady_clock::time_point st_t[4];
    auto st_mark = [&](int k) { if (step_timing) st_t[k] = std::chrono::steady_clock::now(); };
    CA_HIP_CHECK(hipSetDevice(m->device));
    const int32_t n_base = (int32_t)m->nodes.size();
    if (G == 0) return CA_OK;
    if (m->n_scope_blockers > 0) return CA_EUNSUPPORTED;    // casim.h scope: required anti-affinity in the snapshot
    // kcap: new nodes a group can add (limiter cap, or one per pod when unlimited: a group
    // never opens more nodes than it has pods)
    int32_t kcap = lim->max_nodes > 0 ? std::min(lim->max_nodes, std::max(p->max_count, 1)) : std::max(p->max_count, 1);
    kcap = ((kcap + 63) / 64) * 64;
    size_t lds = chain_lds_bytes(kcap, p->use_ports, p->use_scalar);
    // rows that do not fit the CU's LDS (an unlimited estimate of a large group) live in a
    // per-group HBM slab sized by the group's own pod count
    const bool grows = lds + sizeof(ChainRed) > 160 * 1024 || (knob_env("CASIM_CHAIN_GLOBAL") != nullptr);
    if (grows) {
        lds = 0;
        if (p->slab_max_nodes != lim->max_nodes) {
            std::vector<int64_t> off(G);
            std::vector<int32_t> kc(G);
            int64_t tot = 0;
            for (int32_t g = 0; g < G; g++) {
                const int32_t c = std::max(p->h_meta[g].count, 1);
                int32_t kg = lim->max_nodes > 0 ? std::min(lim->max_nodes, c) : c;
                kg = ((kg + 63) / 64) * 64;
                kc[g] = kg;
                off[g] = tot;
                tot += (int64_t)((chain_lds_bytes(kg, p->use_ports, p->use_scalar) + 255) & ~(size_t)255);
            }
            int rc;
            if ((rc = p->d_slab.reserve((size_t)std::max<int64_t>(tot, 256))) != CA_OK) return rc;
            if ((rc = p->d_slab_off.reserve(sizeof(int64_t) * (size_t)G)) != CA_OK) return rc;
            if ((rc = p->d_gkcap.reserve(sizeof(int32_t) * (size_t)G)) != CA_OK) return rc;
            CA_HIP_CHECK(hipMemcpy(p->d_slab_off.ptr, off.data(), sizeof(int64_t) * G, hipMemcpyHostToDevice));
            CA_HIP_CHECK(hipMemcpy(p->d_gkcap.ptr, kc.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice));
            p->slab_max_nodes = lim->max_nodes;
        }
    }
    // Zero-copy results: when the caller's sched_pod is page-locked (ca_host_alloc) and no
    // node ordinals are wanted, the chains publish straight into it (k_ffd_chain epilogue).
    // (Device-resident results could use the same publisher into the plan's own buffer;
    // measured on C2 it slows the chains more than k_copy_segments after them costs.)
    int32_t* publish = nullptr;
    if (to_host && !sched_node && p->total > 0 && (int64_t)G * p->nsub < INT32_MAX && !knob_env("CASIM_NO_PUBLISH")) {
        {
            hipPointerAttribute_t attr;
            const void* hp = sched16 ? (const void*)sched16 : (const void*)sched_pod;
            if (hipPointerGetAttributes(&attr, hp) == hipSuccess && attr.type == hipMemoryTypeHost &&
                attr.devicePointer != nullptr)
                publish = static_cast<int32_t*>(attr.devicePointer);
            else
                (void)hipGetLastError();
        }
    }
    // (no fill of the result buffers: k_copy_segments writes every output the chains do
    // not — run placements, and -1 past n_scheduled or for a failed group)
    const char* rb_env = knob_env("CASIM_RUN_BATCH");
    const int32_t batch_runs = (rb_env && rb_env[0] == '0') ? 0 : 1;
    const bool serial_pub = knob_env("CASIM_PUB_SERIAL") != nullptr;
    // (test hook: the publisher serialised in round 1 only — it gives up there, a later
    // lastIndex round publishes cleanly, and the fallback must still cover round 1's groups)
    const bool serial_pub_r1 = test_hook_env("CASIM_PUB_SERIAL_R1") != nullptr;
    int32_t tickets1 = 0;                               // publisher tickets of round 1 (every group)
    if (publish)
        for (int32_t g = 0; g < G; g++) tickets1 += (p->h_meta[g].count + p->pch - 1) / p->pch;
    // decoupled Go order (uniform classes, bucket path): chains on the stable order, Go's ids
    // beside them (CASIM_GO_DECOUPLE=0: the Go sort ahead of the stream, for tests)
    const bool go_order = go_sort_order();
    const bool decoupled = go_order && p->decouple_ok && p->total > 0 &&
                           !(knob_env("CASIM_GO_DECOUPLE") && atoi(knob_env("CASIM_GO_DECOUPLE")) == 0);
    p->ran_decoupled = decoupled ? 1 : 0;
    p->ran_fan = 0;
    p->ran_sorts = G;                                   // (decoupled: the sort classes, launch_go_sort)
    // Go's sort.Slice permutation of every group and its pod ids, on st3: its own class
    // ranks, k_pdq_sort, ids into d_spod_go and per-group ready flags holding this run's
    // epoch (no reset between runs; every run is synchronised before it returns).  The
    // chains meanwhile run on the stable class order (same class at every position).  It
    // is queued right after the heavy chains when the groups split and the chains read the
    // emitted stream (the heavy chains are then the step's critical path; the sort only
    // bounds when the publisher can start and ends well before them), else before anything
    // else (sort_first, below).
    // (the run's epoch is set before anything is queued: every consumer launched below reads it)
    //
    // The ids are plan state: a decoupled run whose settings match the record of the stored
    // ids (ca_estimate_plan::ids) keeps their epoch and launches no sort — its consumers find
    // every flag up, or wait as usual if the sort queued at creation is still in flight.
    // Every other decoupled run sorts under a new epoch.  The record is cleared here and set
    // again where the run returns CA_OK, so a run that fails, and every run that is not
    // decoupled (the coupled Go sort and the merge path write d_pdq_e / d_pdq_scr /
    // d_pdq_stack), leaves it invalid.
    int32_t sort_NP = 1;
    const bool sort_fold = decoupled && go_sort_fold(p, &sort_NP);
    const GoSortKey sort_key = go_sort_key(p, decoupled, sort_fold);
    const bool reuse_ids = go_sort_reusable(p->ids, sort_key, sort_reuse_on());
    p->ids.valid = false;
    p->ran_reused = reuse_ids ? 1 : 0;
    // ids_final: the stored ids' sort is known finished — nothing waits for ids in this run
    bool ids_final = false;
    if (reuse_ids || (p->decouple_ok && !decoupled)) {
        if (!p->ids_done) {
            if (reuse_ids) {
                const hipError_t q = hipEventQuery(p->ev_ids);
                if (q == hipSuccess) p->ids_done = true;
                else if (q == hipErrorNotReady) (void)hipGetLastError();
                else CA_HIP_CHECK(q);                     // (an error of the sort queued at creation)
            } else {
                // a sort may still be running on st3 with the scratch this run's own sort uses
                CA_HIP_CHECK(hipStreamSynchronize(p->st3));
                p->ids_done = true;
            }
        }
        ids_final = reuse_ids && p->ids_done;
    }
    if (reuse_ids) {
        p->ran_sorts = p->ids_sorts;
        p->ran_fan = p->ids_fan;
        st_mark(0);
    } else if (decoupled) {
        int rce;
        if ((rce = go_sort_new_epoch(p)) != CA_OK) return rce;
    }
    auto launch_go_sort = [&]() -> int {
        int rc0;
        if ((rc0 = queue_go_sort(p, sort_fold, sort_NP)) != CA_OK) return rc0;
        st_mark(0);
        return CA_OK;
    };
    bool go_sort_queued = !decoupled || reuse_ids;
    // (ev_ids is recorded on st3 once the heavy chains are queued: the host's launches ahead
    // of them pace the step's start; a run that reuses the ids keeps the sort's own record)
    bool ids_recorded = !decoupled || reuse_ids;
    auto record_ids = [&]() -> int {
        if (!ids_recorded) { CA_HIP_CHECK(hipEventRecord(p->ev_ids, p->st3)); ids_recorded = true; }
        return CA_OK;
    };
    if (p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_START], st));
    // decoupled: the stream from per-class counts (k_run_table) instead of the radix passes
    // and k_emit_bucket (CASIM_RUNS_STREAM=0: the radix path, for tests)
    const bool runs_stream = !(knob_env("CASIM_RUNS_STREAM") && atoi(knob_env("CASIM_RUNS_STREAM")) == 0);
    // round 1 without k_round_init: k_run_table sets each group's lastIndex / need /
    // unsupported flags, and the publisher's tickets and control words are clean from the
    // last run (ca_estimate_plan::pub_clean) — no launch and no cross-stream event ahead of
    // the chains
    const bool fast_init = decoupled && runs_stream && (!publish || p->pub_clean) && !serial_pub && !serial_pub_r1 &&
                           !knob_env("CASIM_NO_FAST_INIT");
    // The run-table chain (k_ffd_chain<.., TB>): the chains read the run table itself, so
    // k_emit_runs is not launched and d_stream / d_heads are not read; the table of round 1
    // serves the later speculation rounds.  Bound: the table — 44 B per score class of the
    // podset + 12 B (chain_table_bytes) — must fit the CU's 160 KB of LDS beside the rows
    // (or alone, with the rows in HBM slabs) and the reduction scratch; a podset with more
    // classes than that keeps the stream.  CASIM_TABLE_CHAIN=0: the stream path (tests, A/B).
    size_t tab_off = 0;
    bool table_chain = decoupled && runs_stream && batch_runs && p->bucket &&
                       !(knob_env("CASIM_TABLE_CHAIN") && atoi(knob_env("CASIM_TABLE_CHAIN")) == 0);
    if (table_chain) {
        tab_off = grows ? 0 : lds;
        const size_t with_table = grows ? chain_table_bytes(p->s->n_cls)
                                        : chain_lds_bytes(kcap, p->use_ports, p->use_scalar, p->s->n_cls);
        if (with_table + sizeof(ChainRed) > 160 * 1024) { table_chain = false; tab_off = 0; }
        else lds = with_table;
    }
    // The lean chain (k_ffd_chain<.., TB, LEAN>): the run-table chain with rows in LDS, no
    // ports or scalars, no node ordinals wanted, groups of at most 2^20 pods and float64-exact
    // quantities (a plan fact); its table carries 48 B more per class, and one that no
    // longer fits keeps the generic kernel.  CASIM_LEAN_CHAIN=0: the generic kernel (tests, A/B).
    bool lean_chain = table_chain && !grows && !p->use_ports && !p->use_scalar && !sched_node &&
                      p->max_count <= (1 << 20) && p->f64_exact && (kcap + 63) / 64 <= 64 &&
                      !(knob_env("CASIM_LEAN_CHAIN") && atoi(knob_env("CASIM_LEAN_CHAIN")) == 0);
    if (lean_chain) {
        const size_t with_lean = chain_lds_bytes(kcap, false, false, p->s->n_cls, true);
        if (with_lean + sizeof(ChainRed) + sizeof(LeanX) > 160 * 1024) lean_chain = false;
        else lds = with_lean;
    }
    p->ran_table_chain = table_chain ? 1 : 0;
    p->ran_lean_chain = lean_chain ? 1 : 0;
    const int32_t lin0 = *last_index;
    if (publish) p->pub_clean = false;        // set again once this run's publishers all finished clean
    bool pub_gave_up = false;
    if (!fast_init) {
        const int32_t n = std::max(G, tickets1);
        hipLaunchKernelGGL(k_round_init, dim3(std::min((n + 255) / 256, 64)), dim3(256), 0, st, G, *last_index,
                           p->d_lin.as<int32_t>(), p->d_need.as<uint8_t>(), p->d_unsup.as<uint32_t>(),
                           publish ? p->d_tickets.as<int64_t>() : nullptr, tickets1,
                           publish ? p->d_qctl.as<int32_t>() : nullptr);
        CA_HIP_CHECK(hipGetLastError());
    }
    // heavy groups first (bucket path): see ca_estimate_plan::demand
    bool split = false;
    const int32_t* gmapA = nullptr;
    const int32_t* gmapB = nullptr;
    if (p->total > 0 && p->bucket && G >= 8 && !knob_env("CASIM_NO_SPLIT")) {
        // The heavy set: groups whose chain cost is within 60% of the largest, if that is
        // at most half the batch (a flat distribution gains nothing from the split).
        // First from the demand model, then once from the chain times the previous run
        // measured (ChainOut ticks) with the same max_nodes — a scheduling choice only:
        // every run computes everything.
        auto build_map = [&](const std::vector<double>& cost) -> int {
            double cmax = 0;
            for (int32_t g = 0; g < G; g++) cmax = std::max(cmax, cost[g]);
            std::vector<int32_t> map;
            map.reserve(G);
            for (int32_t g = 0; g < G; g++) if (cmax > 0 && cost[g] >= 0.6 * cmax) map.push_back(g);
            p->n_heavy = (int32_t)map.size() * 2 <= G ? (int32_t)map.size() : 0;
            for (int32_t g = 0; g < G; g++) if (!(cmax > 0 && cost[g] >= 0.6 * cmax)) map.push_back(g);
            int rc;
            if ((rc = p->d_gmap.reserve(sizeof(int32_t) * (size_t)G)) != CA_OK) return rc;
            CA_HIP_CHECK(hipMemcpy(p->d_gmap.ptr, map.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice));
            return CA_OK;
        };
        int rc;
        if (p->map_max_nodes != lim->max_nodes) {
            // chain length ~ the template copies a group opens over the runs it gets
            // through: `demand` below the limiter's cap, cap^2/demand above it (the
            // limiter stops the group after ~cap/demand of its pods)
            const double M = lim->max_nodes > 0 ? (double)lim->max_nodes : 0.0;
            std::vector<double> cost(G);
            for (int32_t g = 0; g < G; g++) {
                const double d = p->demand[g];
                cost[g] = (M > 0 && d > M) ? M * M / d : d;
            }
            if ((rc = build_map(cost)) != CA_OK) return rc;
            p->map_max_nodes = lim->max_nodes;
            p->map_source = 1;
        } else if (p->map_source == 1 && (int32_t)p->diag.size() == G) {
            std::vector<double> cost(G);
            for (int32_t g = 0; g < G; g++) cost[g] = (double)(uint32_t)(p->diag[g] & 0xFFFFFFFFull);
            if ((rc = build_map(cost)) != CA_OK) return rc;
            p->map_source = 2;
        }
        split = p->n_heavy > 0 && p->n_heavy < G;
        gmapA = p->d_gmap.as<int32_t>();
        gmapB = gmapA + p->n_heavy;
    }
    const int32_t nA = split ? p->n_heavy : G, nB = split ? G - p->n_heavy : 0;
    // The usual decoupled run uses the plan's stored ids and has no sort to queue: the heavy
    // run table and chains are the first launches of the step, nothing is queued on st3 and
    // no consumer waits for ev_ids.  What follows orders a run that does sort.
    // With the run-table chain the sort is launched first and the heavy run table right behind
    // it.  Since a segment ticket waits only for the sort parts it reads and k_run_table takes
    // its counts from the plan, the publisher ends ~5 us after the heavy chain and the step
    // ends with that chain (C2: profiles/publish_hold_timeline.txt); launching the heavy
    // chains first measured 0.007-0.011 ms faster in every round but cleared the A/B rule in
    // one record of three (profiles/publish_hold_ab.txt), so the order stays.  On the stream
    // path the heavy chains bound the step and go first.  (CASIM_SORT_FIRST=1 / 0 forces either.)
    const char* sf_env = knob_env("CASIM_SORT_FIRST");
    const bool sort_first = sf_env ? atoi(sf_env) != 0 : table_chain;
    const bool sort_after_heavy = split && p->total > 0 && p->bucket && !sort_first;
    if (!go_sort_queued && !sort_after_heavy) {
        int rcs;
        if ((rcs = launch_go_sort()) != CA_OK) return rcs;
        go_sort_queued = true;
    }
    // where the consumers (publisher, segment copies) read the stream's pod ids
    const int32_t* const ids_src = decoupled ? p->d_spod_go.as<int32_t>() : p->d_spod.as<int32_t>();
    std::function<int()> sort_light;        // split: the light groups' sort, queued after the heavy chains
    // 1-3: score, sort, stream
    if (p->total > 0 && p->bucket) {
        const int32_t U = p->s->n_cls;
        int32_t NP = 1;
        while (NP < U) NP <<= 1;
        int32_t* crank = p->d_crank.as<int32_t>();
        const int32_t* pcls = p->s->d_cls.as<int32_t>();
        int32_t nb = 1, passes = 0;                       // buckets <= U: 8-bit digits
        while (nb < U) { nb <<= 8; passes++; }
        passes = std::max(passes, 1);
        const int32_t passes_run = (go_order && !decoupled) ? 0 : passes;
        const int32_t blocks = (p->max_count + 255) / 256;
        // class ranks, then Go's pdqsort (default) or the stable LSD radix passes, stream
        // emission for `ng` groups (map `gm`)
        // (by value: the light groups' call runs after this block's locals are gone)
        auto sort_groups = [=](hipStream_t ss, const int32_t* gm, int32_t ng, bool events) -> int {
            if (decoupled && runs_stream) {
                // the stream from per-class counts (no sort of the pod lists; the class ranks
                // are computed inside k_run_table)
                if (events && p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_SCORE], ss));
                hipLaunchKernelGGL(k_run_table, dim3(ng), dim3(1024), 0, ss, p->d_meta.as<GroupMeta>(),
                                   p->cls_cnt(), p->s->d_cls_sc.as<int64_t>(), NP,
                                   p->s->d_cls_rep.as<int32_t>(), U,
                                   p->d_tmpl.as<ca_template>(), p->s->t.hot.as<PodHot>(), p->s->t.spec.as<ca_pod_spec>(),
                                   p->s->t.terms.as<ca_selector_term>(), p->s->t.reqs.as<ca_selector_req>(),
                                   p->d_rstart.as<int32_t>(), p->d_rsp.as<StreamPod>(), p->d_unsup.as<uint32_t>(), gm,
                                   fast_init ? p->d_lin.as<int32_t>() : nullptr, p->d_need.as<uint8_t>(), lin0,
                                   p->d_rdiv.as<double>());
                CA_HIP_CHECK(hipGetLastError());
                if (!table_chain) {     // (the run-table chain reads the table, not the stream)
                    hipLaunchKernelGGL(k_emit_runs, dim3(blocks, ng), dim3(256), 0, ss, p->d_meta.as<GroupMeta>(),
                                       p->d_rstart.as<int32_t>(), p->d_rsp.as<StreamPod>(), U,
                                       p->d_stream.as<StreamPod>(), p->d_heads.as<uint64_t>(), gm, batch_runs ? 0 : 1);
                    CA_HIP_CHECK(hipGetLastError());
                }
                if (events && p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_MERGE], ss));
                return CA_OK;
            }
            hipLaunchKernelGGL(k_class_rank, dim3(ng), dim3(1024), 0, ss, p->d_meta.as<GroupMeta>(),
                               p->d_tmpl.as<ca_template>(), p->s->d_cls_sc.as<int64_t>(), U, NP, crank, gm);
            CA_HIP_CHECK(hipGetLastError());
            if (events && p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_SCORE], ss));
            uint32_t* a = nullptr;                        // identity (position order)
            uint32_t* bufs[2] = {p->d_sortA.as<uint32_t>(), p->d_sortB.as<uint32_t>()};
            if (go_order && !decoupled) {
                int rc0;
                if ((rc0 = launch_pdq_sort(p, ss, gm, ng, crank, U, nullptr)) != CA_OK) return rc0;
                a = bufs[0];
            }
            for (int ps = 0; ps < passes_run; ps++) {
                uint32_t* b = bufs[ps & 1];
                hipLaunchKernelGGL(k_radix_hist, dim3(p->max_rtiles, ng), dim3(RTHREADS), 0, ss, p->d_meta.as<GroupMeta>(),
                                   a, p->d_pod_idx.as<int32_t>(), pcls, crank, U, 8 * ps, p->d_hist.as<int32_t>(), gm);
                CA_HIP_CHECK(hipGetLastError());
                hipLaunchKernelGGL(k_radix_scan, dim3(ng), dim3(256), 0, ss, p->d_meta.as<GroupMeta>(),
                                   p->d_hist.as<int32_t>(), gm);
                CA_HIP_CHECK(hipGetLastError());
                hipLaunchKernelGGL(k_radix_scatter, dim3(p->max_rtiles, ng), dim3(RTHREADS), 0, ss,
                                   p->d_meta.as<GroupMeta>(), a, p->d_pod_idx.as<int32_t>(), pcls, crank, U, 8 * ps,
                                   p->d_hist.as<int32_t>(), b, gm);
                CA_HIP_CHECK(hipGetLastError());
                a = b;
            }
            if (events && p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_MERGE], ss));
            hipLaunchKernelGGL(k_emit_bucket, dim3(blocks, ng), dim3(256), 0, ss, p->d_meta.as<GroupMeta>(), a,
                               p->d_pod_idx.as<int32_t>(), p->d_tmpl.as<ca_template>(), p->s->t.hot.as<PodHot>(),
                               p->s->t.spec.as<ca_pod_spec>(), p->s->t.terms.as<ca_selector_term>(),
                               p->s->t.reqs.as<ca_selector_req>(), p->d_stream.as<StreamPod>(), p->d_spod.as<int32_t>(),
                               p->d_heads.as<uint64_t>(), p->d_unsup.as<uint32_t>(), gm);
            CA_HIP_CHECK(hipGetLastError());
            return CA_OK;
        };
        int rc;
        if (split) {     // the light groups are sorted right after the heavy chains are queued
            // (fast_init: nothing of k_round_init to wait for)
            if (!fast_init) CA_HIP_CHECK(hipEventRecord(p->ev_init, st));
            if ((rc = sort_groups(st, gmapA, nA, true)) != CA_OK) return rc;
            sort_light = [=]() -> int {
                if (!fast_init) CA_HIP_CHECK(hipStreamWaitEvent(p->st2, p->ev_init, 0));
                return sort_groups(p->st2, gmapB, nB, false);
            };
        } else if ((rc = sort_groups(st, nullptr, G, true)) != CA_OK) {
            return rc;
        }
    } else if (p->total > 0) {
        const int32_t tiles = (p->max_count + TILE - 1) / TILE;
        hipLaunchKernelGGL(k_score_tiles, dim3(tiles, G), dim3(256), 0, st, p->d_meta.as<GroupMeta>(),
                           p->d_pod_idx.as<int32_t>(), p->d_tmpl.as<ca_template>(), p->s->t.hot.as<PodHot>(),
                           p->s->t.spec.as<ca_pod_spec>(), p->s->t.terms.as<ca_selector_term>(),
                           p->s->t.reqs.as<ca_selector_req>(), p->d_sortA.as<SortItem>(), p->d_unsup.as<uint32_t>());
        CA_HIP_CHECK(hipGetLastError());
        if (p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_SCORE], st));
        SortItem* a = p->d_sortA.as<SortItem>();
        SortItem* b = p->d_sortB.as<SortItem>();
        const int32_t blocks = (p->max_count + 255) / 256;
        for (int32_t w = TILE; w < p->max_count; w *= 2) {
            hipLaunchKernelGGL(k_merge_runs, dim3(blocks, G), dim3(256), 0, st, p->d_meta.as<GroupMeta>(), a, b, w);
            CA_HIP_CHECK(hipGetLastError());
            std::swap(a, b);
        }
        if (go_order) {
            // dense ranks from the comparison sort, then sort.Slice's permutation of them
            hipLaunchKernelGGL(k_item_rank, dim3(G), dim3(1024), 0, st, p->d_meta.as<GroupMeta>(), a,
                               p->d_item_rank.as<uint32_t>());
            CA_HIP_CHECK(hipGetLastError());
            int rc0;
            if ((rc0 = launch_pdq_sort(p, st, nullptr, G, nullptr, 0, p->d_item_rank.as<uint32_t>())) != CA_OK)
                return rc0;
        }
        if (p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_MERGE], st));
        if (go_order) {
            hipLaunchKernelGGL(k_emit_bucket, dim3(blocks, G), dim3(256), 0, st, p->d_meta.as<GroupMeta>(),
                               p->d_sortA.as<uint32_t>(), p->d_pod_idx.as<int32_t>(), p->d_tmpl.as<ca_template>(),
                               p->s->t.hot.as<PodHot>(), p->s->t.spec.as<ca_pod_spec>(),
                               p->s->t.terms.as<ca_selector_term>(), p->s->t.reqs.as<ca_selector_req>(),
                               p->d_stream.as<StreamPod>(), p->d_spod.as<int32_t>(), p->d_heads.as<uint64_t>(),
                               p->d_unsup.as<uint32_t>(), nullptr);
        } else {
            hipLaunchKernelGGL(k_emit_stream, dim3(blocks, G), dim3(256), 0, st, p->d_meta.as<GroupMeta>(), a,
                               p->d_pod_idx.as<int32_t>(), p->s->t.hot.as<PodHot>(), p->d_stream.as<StreamPod>(),
                               p->d_spod.as<int32_t>(), p->d_heads.as<uint64_t>());
        }
        CA_HIP_CHECK(hipGetLastError());
    }
    if (p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_EMIT], st));
    // 4-5: chains with lastIndex speculation
    std::vector<int32_t> lin(G, *last_index);
    std::vector<uint8_t> need(G, 1);
    std::vector<ChainOut> outs(G);
    std::vector<uint8_t> accepted(G, 0);
    std::vector<int32_t> true_lin(G, *last_index);
    int32_t cut = -1;                   // first unsupported group when later groups exist (prefix protocol)
    // the host joins the streams itself (publisher, heavy and light chains) instead of
    // queueing cross-stream waits ahead of the readback event on st
    const bool host_joins = publish && !p->phase_events;
    bool light_pending = false;
    int32_t rounds = 0;
    float chain_ms = 0;
    {
        int32_t* hq = p->h_qc.as<int32_t>();     // host-side failure flags ([2] per round, [3] sticky)
        hq[2] = hq[3] = 0;
    }
    for (;;) {
        rounds++;
        if (rounds > 1) p->h_qc.as<int32_t>()[2] = 0;
        const bool serial_now = serial_pub || (serial_pub_r1 && rounds == 1);
        if (rounds > 1) {      // round 1's state came from k_round_init
            CA_HIP_CHECK(hipMemcpyAsync(p->d_lin.ptr, lin.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, st));
            CA_HIP_CHECK(hipMemcpyAsync(p->d_need.ptr, need.data(), G, hipMemcpyHostToDevice, st));
        }
        int32_t round_tickets = 0;
        // the publisher's start: after the ticket reset (k_round_init, or the memsets of a
        // later round); round 1 of a split run reuses ev_init (recorded right after
        // k_round_init), so no marker sits between the heavy stream and its chains
        hipEvent_t pub_go = p->ev_go;
        if (publish) {
            for (int32_t g = 0; g < G; g++) if (need[g]) round_tickets += (p->h_meta[g].count + p->pch - 1) / p->pch;
            if (rounds > 1) {
                CA_HIP_CHECK(hipStreamWaitEvent(st, p->ev_pub, 0));   // previous publisher done
                CA_HIP_CHECK(hipMemsetAsync(p->d_tickets.ptr, 0xFF, sizeof(int64_t) * (size_t)std::max(round_tickets, 1), st));
                CA_HIP_CHECK(hipMemsetAsync(p->d_qctl.ptr, 0, sizeof(int32_t) * 3, st));   // [3] stays: sticky
                CA_HIP_CHECK(hipMemsetAsync(p->d_qctl.as<int32_t>() + 4, 0, sizeof(int32_t) * 2, st));
            }
            if (rounds == 1 && fast_init) pub_go = nullptr;       // the tickets are clean already
            else if (rounds == 1 && split) pub_go = p->ev_init;
            else CA_HIP_CHECK(hipEventRecord(p->ev_go, st));
        }
        // CASIM_PUB_SERIAL (tests): the publisher goes first on the chains' own stream, i.e.
        // the two kernels are serialised — it must give up at its start deadline
        auto launch_pub = [&](hipStream_t ps) -> int {
            if (sched16)
                hipLaunchKernelGGL(k_publish<uint16_t>, dim3(std::min(round_tickets, pub_blocks(decoupled, table_chain))), dim3(256), 0, ps,
                                   p->d_meta.as<GroupMeta>(), p->d_out.as<ChainOut>(), p->d_seg.as<Seg>(),
                                   ids_src, p->d_sched_pod.as<int32_t>(), p->d_tickets.as<int64_t>(),
                                   p->d_qctl.as<int32_t>(), round_tickets, p->nsub, p->d_prog.as<int2>(), p->pch,
                                   reinterpret_cast<uint16_t*>(publish), pub_start_ticks(),
                                   decoupled ? p->d_ids_ready.as<int32_t>() : nullptr, p->ids_epoch, p->h_qc.as<int32_t>(),
                                   ids_final ? 1 : 0);
            else
                hipLaunchKernelGGL(k_publish<int32_t>, dim3(std::min(round_tickets, pub_blocks(decoupled, table_chain))), dim3(256), 0, ps,
                                   p->d_meta.as<GroupMeta>(), p->d_out.as<ChainOut>(), p->d_seg.as<Seg>(),
                                   ids_src, p->d_sched_pod.as<int32_t>(), p->d_tickets.as<int64_t>(),
                                   p->d_qctl.as<int32_t>(), round_tickets, p->nsub, p->d_prog.as<int2>(), p->pch,
                                   publish, pub_start_ticks(), decoupled ? p->d_ids_ready.as<int32_t>() : nullptr, p->ids_epoch,
                                   p->h_qc.as<int32_t>(), ids_final ? 1 : 0);
            CA_HIP_CHECK(hipGetLastError());
            return CA_OK;
        };
        if (publish && round_tickets > 0 && serial_now) {
            int rc0;
            if ((rc0 = launch_pub(st)) != CA_OK) return rc0;
            CA_HIP_CHECK(hipEventRecord(p->ev_pub, st));
        }
        if (p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_CHAIN0], st));
        const bool ps = p->use_ports || p->use_scalar;
        auto chain_kernel =
            lean_chain  ? k_ffd_chain<false, false, true, true> :
            table_chain ? (grows ? (ps ? k_ffd_chain<true, true, true> : k_ffd_chain<true, false, true>)
                                 : (ps ? k_ffd_chain<false, true, true> : k_ffd_chain<false, false, true>))
                        : (grows ? (ps ? k_ffd_chain<true, true, false> : k_ffd_chain<true, false, false>)
                                 : (ps ? k_ffd_chain<false, true, false> : k_ffd_chain<false, false, false>));
        if (lds > 0) {
            int rcl;
            if ((rcl = ensure_dyn_lds((const void*)chain_kernel, lds)) != CA_OK) return rcl;
        }
        auto chain = [&](hipStream_t ss, const int32_t* gm, int32_t ng) -> int {
            hipLaunchKernelGGL(chain_kernel, dim3(ng), dim3(CT), lds, ss,
                               p->d_meta.as<GroupMeta>(),
                               p->d_stream.as<StreamPod>(), p->d_heads.as<uint64_t>(), p->d_tmpl.as<ca_template>(),
                               p->s->t.spec.as<ca_pod_spec>(), p->s->t.hot.as<PodHot>(), p->d_lin.as<int32_t>(),
                               p->d_need.as<uint8_t>(), p->d_unsup.as<uint32_t>(), n_base, lim->max_nodes, kcap,
                               p->use_ports ? 1 : 0, p->use_scalar ? 1 : 0, batch_runs,
                               p->d_sched_pod.as<int32_t>(), sched_node ? p->d_sched_node.as<int32_t>() : nullptr,
                               p->d_seg.as<Seg>(), publish ? p->d_tickets.as<int64_t>() : nullptr,
                               p->d_qctl.as<int32_t>(), p->nsub, p->d_prog.as<int2>(), p->pch, p->d_out.as<ChainOut>(),
                               gm, grows ? p->d_slab.as<unsigned char>() : nullptr,
                               grows ? p->d_slab_off.as<int64_t>() : nullptr, grows ? p->d_gkcap.as<int32_t>() : nullptr,
                               decoupled ? 1 : 0, p->h_out.as<ChainOut>(), p->h_qc.as<int32_t>(),
                               p->d_rstart.as<int32_t>(), p->d_rsp.as<StreamPod>(), p->s->n_cls, (int32_t)tab_off,
                               p->d_rdiv.as<double>());
            CA_HIP_CHECK(hipGetLastError());
            return CA_OK;
        };
        int rc;
        if (rounds == 1 && split) {         // heavy groups on st as soon as their sort is done
            if ((rc = chain(st, gmapA, nA)) != CA_OK) return rc;
            if (!go_sort_queued) {
                if ((rc = launch_go_sort()) != CA_OK) return rc;
                go_sort_queued = true;
            }
            if ((rc = record_ids()) != CA_OK) return rc;
            if ((rc = sort_light()) != CA_OK) return rc;
            if ((rc = chain(p->st2, gmapB, nB)) != CA_OK) return rc;
            CA_HIP_CHECK(hipEventRecord(p->ev_b, p->st2));
            // (publishing without phase events the host waits for ev_b itself: one
            // cross-stream hop less between the last chain and the host)
            if (!host_joins) CA_HIP_CHECK(hipStreamWaitEvent(st, p->ev_b, 0));
            light_pending = host_joins;
        } else if ((rc = chain(st, nullptr, G)) != CA_OK) {
            return rc;
        }
        if (!go_sort_queued) {             // (a later round of a split run: queued in round 1)
            if ((rc = launch_go_sort()) != CA_OK) return rc;
            go_sort_queued = true;
        }
        if ((rc = record_ids()) != CA_OK) return rc;
        if (publish && round_tickets > 0 && !serial_now) {
            if (pub_go) CA_HIP_CHECK(hipStreamWaitEvent(p->pub_stream, pub_go, 0));
            if ((rc = launch_pub(p->pub_stream)) != CA_OK) return rc;
            CA_HIP_CHECK(hipEventRecord(p->ev_pub, p->pub_stream));
        }
        if (p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_CHAIN1], st));
        // one readback per round: the chain outputs, and (publishing) the publisher's
        // counters once it is done — the results are then already in the caller's buffer
        // (the chains write their ChainOut records, and the chains / publisher their failure
        // flags, straight into page-locked h_out / h_qc: no copy kernels at the step's end)
        const ChainOut* fresh = p->h_out.as<ChainOut>();
        const bool pub_ran = publish && round_tickets > 0 && !serial_now;
        if (publish && !(host_joins && pub_ran)) CA_HIP_CHECK(hipStreamWaitEvent(st, p->ev_pub, 0));
        CA_HIP_CHECK(hipEventRecord(p->ev_rb, st));
        // results of this round, queued behind the readback: the device fills them while
        // the host walks the lastIndex chain (a later round queues them again)
        if (p->total > 0 && !publish && !decoupled) {
            hipLaunchKernelGGL(k_copy_segments, dim3((p->max_count + CPY_PER_BLOCK - 1) / CPY_PER_BLOCK, G), dim3(256), 0,
                               st, p->d_meta.as<GroupMeta>(), p->d_out.as<ChainOut>(), p->d_seg.as<Seg>(),
                               p->d_spod.as<int32_t>(), p->d_sched_pod.as<int32_t>(),
                               sched_node ? p->d_sched_node.as<int32_t>() : nullptr, 0);
            CA_HIP_CHECK(hipGetLastError());
        }
        if (p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_COMPACT], st));
        // (polling the events with hipEventQuery instead measured the same: 0.486 ms)
        if (rounds == 1) st_mark(1);
        if (host_joins && pub_ran) CA_HIP_CHECK(hipEventSynchronize(p->ev_pub));   // (finishes last)
        CA_HIP_CHECK(hipEventSynchronize(p->ev_rb));
        if (light_pending) { CA_HIP_CHECK(hipEventSynchronize(p->ev_b)); light_pending = false; }
        if (rounds == 1) st_mark(2);
        if (publish && p->h_qc.as<int32_t>()[2] != 0) pub_gave_up = true;
        float ms = 0;
        if (p->phase_events)
            (void)hipEventElapsedTime(&ms, p->ev[ca_estimate_plan::EV_CHAIN0], p->ev[ca_estimate_plan::EV_CHAIN1]);
        chain_ms += ms;
        for (int32_t g = 0; g < G; g++) if (need[g]) outs[g] = fresh[g];
        if (rounds == 1) {
            p->diag.resize(G);
            for (int32_t g = 0; g < G; g++) p->diag[g] = fresh[g].pad;
        }
        // walk the lastIndex chain
        int64_t cur = *last_index;
        cut = -1;
        bool known = true;
        bool all_ok = true;
        std::fill(need.begin(), need.end(), 0);
        for (int32_t g = 0; g < G; g++) {
            const ChainOut& o = outs[g];
            true_lin[g] = (int32_t)cur;     // exact once the walk converged (known stays true)
            if (o.status == CA_EUNSUPPORTED && known) {
                // prefix protocol (casim.h scope): groups after it are CA_ENOTRUN, the batch's
                // lastIndex is the one this group starts from
                for (int32_t h = g; h < G; h++) { accepted[h] = 1; need[h] = 0; }
                if (g + 1 < G) cut = g;
                break;
            }
            const bool insensitive = o.status != CA_OK || !o.sensitive;
            if (known && (o.lin == cur || insensitive)) {
                accepted[g] = 1;
                if (o.status == CA_OK && o.had_success) cur = o.lout;
                continue;
            }
            if (!known && insensitive) {
                accepted[g] = 1;                         // result independent of lastIndex
                if (o.status == CA_OK && o.had_success) { cur = o.lout; known = true; }
                continue;
            }
            // sensitive group run from a wrong lastIndex: re-run from the best guess
            accepted[g] = 0;
            all_ok = false;
            need[g] = 1;
            lin[g] = (int32_t)cur;
            if (known) {
                known = false;   // this group's output is unknown until it re-runs
            }
            // speculate: the stale output is the guess for the successors
            cur = o.had_success ? o.lout : cur;
        }
        if (all_ok) {
            *last_index = (int32_t)cur;
            break;
        }
        if (rounds > G + 2) { set_last_error("estimate speculation did not converge"); return CA_EDEVICE; }
    }
    // results: the chains wrote single placements directly, the last round's
    // k_copy_segments the run placements (or the publisher, into the caller's buffer)
    if (decoupled && !publish && p->total > 0) {
        // once, after the last round: stream positions -> Go-order ids
        if (!ids_final) CA_HIP_CHECK(hipStreamWaitEvent(st, p->ev_ids, 0));
        hipLaunchKernelGGL(k_copy_segments, dim3((p->max_count + CPY_PER_BLOCK - 1) / CPY_PER_BLOCK, G), dim3(256), 0,
                           st, p->d_meta.as<GroupMeta>(), p->d_out.as<ChainOut>(), p->d_seg.as<Seg>(),
                           ids_src, p->d_sched_pod.as<int32_t>(),
                           sched_node ? p->d_sched_node.as<int32_t>() : nullptr, 1);
        CA_HIP_CHECK(hipGetLastError());
    }
    if (publish) {
        p->pub_clean = !pub_gave_up;
        // the publisher of the last round wrote the results; a deadline hit (a chain that
        // died) falls back to the device copy + D2H
        const int32_t* qc = p->h_qc.as<int32_t>();      // read back with the last round's outputs
        p->pub_state = 1;
        // (a give-up in ANY round: qc[2] is reset per round and a later round publishes only
        // the groups it re-ran, so round 1's accepted groups would otherwise stay unwritten)
        if (pub_gave_up || qc[2] != 0 || qc[3] != 0) {
            p->pub_state = 2;
            set_last_error("estimate publisher missed a ticket; results copied instead");
            if (decoupled && !ids_final) CA_HIP_CHECK(hipStreamWaitEvent(st, p->ev_ids, 0));
            hipLaunchKernelGGL(k_copy_segments, dim3((p->max_count + CPY_PER_BLOCK - 1) / CPY_PER_BLOCK, G), dim3(256), 0,
                               st, p->d_meta.as<GroupMeta>(), p->d_out.as<ChainOut>(), p->d_seg.as<Seg>(),
                               ids_src, p->d_sched_pod.as<int32_t>(), nullptr, decoupled ? 1 : 0);
            CA_HIP_CHECK(hipGetLastError());
            int rc;
            if (to_host && (rc = results_to_host(p, st, sched_pod, sched16)) != CA_OK) return rc;
        }
    } else if (to_host) {
        int rc;
        if ((rc = results_to_host(p, st, sched_pod, sched16)) != CA_OK) return rc;
    }
    if (sched_node)
        CA_HIP_CHECK(hipMemcpyAsync(sched_node, p->d_sched_node.ptr, sizeof(int32_t) * std::max(p->total, 0),
                                    hipMemcpyDeviceToHost, st));
    if (p->phase_events) CA_HIP_CHECK(hipEventRecord(p->ev[ca_estimate_plan::EV_D2H], st));
    // (published with the host joining the streams: the round's event already covered
    // everything queued on st, nothing was queued since)
    if (!(host_joins && p->pub_state == 1)) CA_HIP_CHECK(hipStreamSynchronize(st));
    for (int32_t g = 0; g < G; g++) {
        const ChainOut& o = outs[g];
        ca_estimate_result& r = results[g];
        r.node_count = o.node_count;
        r.n_scheduled = o.n_sched;
        r.nodes_added = o.nodes_added;
        r.last_index_in = true_lin[g];
        r.last_index_out = o.status == CA_OK && o.had_success ? o.lout : true_lin[g];
        r.status = o.status;
        r.evals = o.evals;
        if (cut >= 0 && g > cut) {        // CA_ENOTRUN: nothing of it is reported
            r.node_count = r.n_scheduled = r.nodes_added = 0;
            r.last_index_in = r.last_index_out = true_lin[cut];
            r.status = CA_ENOTRUN;
            r.evals = 0;
        }
    }
    float sort_ms = 0;
    {
        using P = ca_estimate_plan;
        auto el = [&](int a, int b) {
            float v = 0;
            if (p->phase_events) (void)hipEventElapsedTime(&v, p->ev[a], p->ev[b]);
            return v;
        };
        const bool any = p->total > 0;
        p->t_ms[0] = any ? el(P::EV_START, P::EV_SCORE) : 0;
        p->t_ms[1] = any ? el(P::EV_SCORE, P::EV_MERGE) : 0;
        p->t_ms[2] = any ? el(P::EV_MERGE, P::EV_EMIT) : 0;
        p->t_ms[3] = chain_ms;
        p->t_ms[4] = el(P::EV_CHAIN1, P::EV_COMPACT);
        p->t_ms[5] = el(P::EV_COMPACT, P::EV_D2H);
        sort_ms = el(P::EV_START, P::EV_EMIT);
    }
    p->grp_succ.assign((size_t)G, 0);
    for (int32_t g = 0; g < G; g++)
        p->grp_succ[g] = outs[g].status == CA_OK && outs[g].had_success && !(cut >= 0 && g > cut) ? 1 : 0;
    // batch-level lastIndex dependence: the first group with a FitsAnyNode success decides
    p->stats.lin_sensitive = 0;
    p->stats.had_success = 0;
    for (int32_t g = 0; g < G; g++) {
        const ChainOut& o = outs[g];
        if (o.status != CA_OK || !o.had_success) continue;
        p->stats.lin_sensitive = o.sensitive;
        p->stats.had_success = 1;
        break;
    }
    p->stats.rounds = rounds;
    p->stats.kernel_ms = chain_ms;
    p->stats.sort_ms = reuse_ids ? 0.f : sort_ms;      // (a run that launched no Go-order sort)
    p->stats.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    p->t_ms[6] = p->stats.total_ms;
    if (step_timing) {
        const auto t_exit = std::chrono::steady_clock::now();
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double, std::micro>(b - a).count();
        };
        st_acc[0] += us(t_start, st_t[0]);
        st_acc[1] += us(st_t[0], st_t[1]);
        st_acc[2] += us(st_t[1], st_t[2]);
        st_acc[3] += us(st_t[2], t_exit);
        if (st_n > 0) st_acc[4] += us(st_last_exit, t_start);
        st_acc[5] += us(t_start, t_exit);
        st_last_exit = t_exit;
        if (++st_n == 20) {
            fprintf(stderr, "[step] us per call: to the sort launch %.1f, to the last launch %.1f, join wait %.1f, "
                    "to the return %.1f, caller between calls %.1f, call %.1f\n", st_acc[0] / 20, st_acc[1] / 20,
                    st_acc[2] / 20, st_acc[3] / 20, st_acc[4] / 19, st_acc[5] / 20);
            for (double& v : st_acc) v = 0;
            st_n = 0;
        }
    }
    p->last_nsched.resize((size_t)G);
    for (int32_t g = 0; g < G; g++) p->last_nsched[g] = results[g].status == CA_OK ? results[g].n_scheduled : 0;
    // (a publisher that ran to its end wrote the caller's buffer only: d_sched_pod then holds
    // stream positions or single placements alone)
    p->lists_final = !publish || p->pub_state == 2;
    if (decoupled) {
        // the ids in d_spod_go / d_ids_ready are this run's (sorted or kept): the next run
        // with the same settings uses them
        p->ids.valid = true;
        p->ids.epoch = p->ids_epoch;
        p->ids.key = sort_key;
        p->ids_sorts = p->ran_sorts;
        p->ids_fan = p->ran_fan;
    }
    return CA_OK;
}

}  // namespace

// Results of the plan's last run re-based to another input lastIndex, for a batch that is
// not lastIndex-sensitive (its outputs are the same from any input: multi.hip).  Returns
// the batch's output lastIndex from `lin`.
namespace casim {
int32_t estimate_plan_rebase(const ca_estimate_plan* p, ca_estimate_result* results, int32_t lin) {
    int32_t cur = lin;
    for (int32_t g = 0; g < p->G; g++) {
        ca_estimate_result& r = results[g];
        r.last_index_in = cur;
        if (r.status == CA_OK && g < (int32_t)p->grp_succ.size() && p->grp_succ[g]) cur = r.last_index_out;
        else r.last_index_out = cur;
    }
    return cur;
}
}  // namespace casim

namespace casim {
void estimate_plan_lists(const ca_estimate_plan* p, PlanLists* out) {
    out->m = p->m;
    out->s = p->s;
    out->G = p->G;
    out->total = p->total;
    out->h_off = p->h_off.data();
    out->h_nsched = p->last_nsched.data();
    out->d_sched_pod = p->d_sched_pod.as<int32_t>();
    out->final_lists = p->lists_final && (int32_t)p->last_nsched.size() == p->G;
    out->scratch = &p->opt_scratch;
    out->missing = &p->missing_scratch;
    out->price = &p->price_scratch;
}
}  // namespace casim

extern "C" {

int ca_estimate_plan_rebase(const ca_estimate_plan* p, ca_estimate_result* results, int32_t last_index_in,
                            int32_t* last_index_out) {
    if (!p || (p->G > 0 && !results)) return CA_EINVAL;
    const int32_t lout = casim::estimate_plan_rebase(p, results, last_index_in);
    if (last_index_out) *last_index_out = lout;
    return CA_OK;
}

int ca_estimate_plan_create(ca_mirror* m, const ca_podset* s, const int32_t* group_off, const int32_t* pod_idx,
                            const ca_template* templates, int32_t n_groups, ca_estimate_plan** out) {
    if (!m || !s || !group_off || !out || n_groups < 0 || (n_groups > 0 && !templates)) return CA_EINVAL;
    CA_HIP_CHECK(hipSetDevice(m->device));
    ca_estimate_plan* p = new ca_estimate_plan();
    int rc = plan_prepare(p, m, s, group_off, pod_idx, nullptr, templates, n_groups);
    if (rc != CA_OK) { delete p; return rc; }
    *out = p;
    return CA_OK;
}

int ca_estimate_plan_create_options(ca_mirror* m, const ca_podset* s, const int32_t* eg_off, const int32_t* eg_pod,
                                    int32_t n_eg, const uint8_t* ok, const ca_template* templates, int32_t n_groups,
                                    int32_t* group_off_out, ca_estimate_plan** out) {
    if (!m || !s || !eg_off || !out || !group_off_out || n_eg < 0 || n_groups < 0 || (n_groups > 0 && !templates) ||
        (n_groups > 0 && n_eg > 0 && !ok))
        return CA_EINVAL;
    // every check before any launch or allocation
    if (eg_off[0] != 0) return CA_EINVAL;
    for (int32_t e = 0; e < n_eg; e++)
        if (eg_off[e + 1] < eg_off[e]) return CA_EINVAL;
    if (eg_off[n_eg] > 0 && !eg_pod) return CA_EINVAL;
    const int32_t np_ = s->t.n_pods;
    for (int32_t i = 0; i < eg_off[n_eg]; i++)
        if ((uint32_t)eg_pod[i] >= (uint32_t)np_) return CA_EINVAL;
    std::vector<int32_t> group_off((size_t)n_groups + 1, 0);
    int64_t total = 0;
    for (int32_t g = 0; g < n_groups; g++) {
        const uint8_t* row = ok + (size_t)g * (size_t)n_eg;
        int64_t c = 0;
        for (int32_t e = 0; e < n_eg; e++) c += row[e] ? (int64_t)(eg_off[e + 1] - eg_off[e]) : 0;
        total += c;
        if (total > INT32_MAX) return CA_EINVAL;
        group_off[(size_t)g + 1] = (int32_t)total;
    }
    CA_HIP_CHECK(hipSetDevice(m->device));
    ca_estimate_plan* p = new ca_estimate_plan();
    const OptionSrc opt{eg_off, eg_pod, n_eg, ok};
    int rc = plan_prepare(p, m, s, group_off.data(), nullptr, &opt, templates, n_groups);
    if (rc != CA_OK) { delete p; return rc; }
    std::memcpy(group_off_out, group_off.data(), sizeof(int32_t) * group_off.size());
    *out = p;
    return CA_OK;
}

int ca_estimate_plan_create_groups(ca_mirror* m, const ca_podset* s, const ca_pod_groups* g, const uint8_t* ok,
                                   const ca_template* templates, int32_t n_groups, int32_t* group_off_out,
                                   ca_estimate_plan** out) {
    if (!m || !s || !g || g->m != m || g->s != s || !out || !group_off_out || n_groups < 0 ||
        (n_groups > 0 && !templates) || (n_groups > 0 && g->n_eg > 0 && !ok))
        return CA_EINVAL;
    // the handle's CSR was built from checked indices: only the rows' totals are taken here
    const int32_t n_eg = g->n_eg;
    const int32_t* eg_off = g->h_eg_off.data();
    std::vector<int32_t> group_off((size_t)n_groups + 1, 0);
    int64_t total = 0;
    for (int32_t q = 0; q < n_groups; q++) {
        const uint8_t* row = ok + (size_t)q * (size_t)n_eg;
        int64_t c = 0;
        for (int32_t e = 0; e < n_eg; e++) c += row[e] ? (int64_t)(eg_off[e + 1] - eg_off[e]) : 0;
        total += c;
        if (total > INT32_MAX) return CA_EINVAL;
        group_off[(size_t)q + 1] = (int32_t)total;
    }
    CA_HIP_CHECK(hipSetDevice(m->device));
    ca_estimate_plan* p = new ca_estimate_plan();
    OptionSrc opt{eg_off, g->h_eg_pod.data(), n_eg, ok};
    opt.d_eg_off = g->d_eg_off;
    opt.d_eg_pod = g->d_eg_pod;
    int rc = plan_prepare(p, m, s, group_off.data(), nullptr, &opt, templates, n_groups);
    if (rc != CA_OK) { delete p; return rc; }
    std::memcpy(group_off_out, group_off.data(), sizeof(int32_t) * group_off.size());
    *out = p;
    return CA_OK;
}

int ca_estimate_plan_fetch_lists(const ca_estimate_plan* p, int32_t* pod_idx, int32_t* item_cls) {
    if (!p) return CA_EINVAL;
    CA_HIP_CHECK(hipSetDevice(p->m->device));
    if (p->total > 0 && pod_idx)
        CA_HIP_CHECK(hipMemcpy(pod_idx, p->d_pod_idx.ptr, sizeof(int32_t) * (size_t)p->total, hipMemcpyDeviceToHost));
    if (p->total > 0 && item_cls && p->bucket)
        CA_HIP_CHECK(hipMemcpy(item_cls, p->d_item_cls.ptr, sizeof(int32_t) * (size_t)p->total, hipMemcpyDeviceToHost));
    return CA_OK;
}

int ca_estimate_plan_fetch_class_counts(const ca_estimate_plan* p, int32_t* out, int32_t* n_classes) {
    if (!p || (!out && !n_classes)) return CA_EINVAL;
    if (n_classes) *n_classes = p->s->n_cls;
    if (!out) return CA_OK;
    CA_HIP_CHECK(hipSetDevice(p->m->device));
    const size_t n = (size_t)p->G * (size_t)p->s->n_cls;
    if (!p->has_cls_cnt) {                 // (no items, or a plan that never takes the run-table path)
        if (p->total > 0) return CA_EINVAL;
        std::fill(out, out + n, 0);
        return CA_OK;
    }
    CA_HIP_CHECK(hipMemcpy(out, p->cls_cnt(), sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return CA_OK;
}

int ca_estimate_plan_fetch(const ca_estimate_plan* p, int32_t* sched_pod) {
    if (!p || !sched_pod) return CA_EINVAL;
    CA_HIP_CHECK(hipSetDevice(p->m->device));
    if (p->total > 0)
        CA_HIP_CHECK(hipMemcpy(sched_pod, p->d_sched_pod.ptr, sizeof(int32_t) * (size_t)p->total, hipMemcpyDeviceToHost));
    return CA_OK;
}

int ca_estimate_plan_device_results(const ca_estimate_plan* p, const int32_t** sched_pod_dev) {
    if (!p || !sched_pod_dev) return CA_EINVAL;
    *sched_pod_dev = p->d_sched_pod.as<int32_t>();
    return CA_OK;
}

int ca_estimate_plan_run(ca_estimate_plan* p, const ca_limiter* limiter, int32_t* last_index,
                         ca_estimate_result* results, int32_t* sched_pod, int32_t* sched_node) {
    if (!p) return CA_EINVAL;
    return plan_run(p, limiter, last_index, results, sched_pod, sched_node);
}

int ca_estimate_plan_run_u16(ca_estimate_plan* p, const ca_limiter* limiter, int32_t* last_index,
                             ca_estimate_result* results, uint16_t* sched_pod16) {
    if (!p || !sched_pod16) return CA_EINVAL;
    return plan_run(p, limiter, last_index, results, nullptr, nullptr, sched_pod16);
}

int ca_estimate_plan_destroy(ca_estimate_plan* p) {
    if (!p) return CA_EINVAL;
    delete p;
    return CA_OK;
}

int ca_estimate_plan_stats(const ca_estimate_plan* p, int32_t* rounds, float* chain_ms, float* sort_ms, float* total_ms) {
    if (!p) return CA_EINVAL;
    if (rounds) *rounds = p->stats.rounds;
    if (chain_ms) *chain_ms = p->stats.kernel_ms;
    if (sort_ms) *sort_ms = p->stats.sort_ms;
    if (total_ms) *total_ms = p->stats.total_ms;
    return CA_OK;
}

int ca_estimate_plan_timings(const ca_estimate_plan* p, float* out, int32_t cap) {
    if (!p || (cap > 0 && !out)) return CA_EINVAL;
    const int32_t n = 15;
    for (int32_t i = 0; i < 7 && i < cap; i++) out[i] = p->t_ms[i];
    if (cap > 14) out[14] = (float)p->ran_reused;
    if (cap > 12) out[12] = p->opt_lists_ms;
    if (cap > 13) out[13] = (float)p->ran_lean_chain;
    if (cap > 7) out[7] = (float)p->pub_state;
    if (cap > 8) out[8] = (float)p->ran_decoupled;
    if (cap > 9) out[9] = (float)p->ran_table_chain;
    if (cap > 10) out[10] = (float)p->ran_sorts;
    if (cap > 11) {
        // the parts are decided on the device: read the fan records of the sort whose ids the
        // run used (a sort queued at creation, or one whose last parts no ticket read, may
        // still be running: st3 is drained first)
        int32_t parts = p->ran_sorts;
        if (p->ran_decoupled && p->ran_fan) {
            const int32_t G = p->G;
            CA_HIP_CHECK(hipSetDevice(p->m->device));
            CA_HIP_CHECK(hipStreamSynchronize(p->st3));
            std::vector<int32_t> rec((size_t)pdq::FAN_STRIDE * (size_t)std::max(G, 1));
            CA_HIP_CHECK(hipMemcpy(rec.data(), p->d_ids_ready.ptr, sizeof(int32_t) * rec.size(), hipMemcpyDeviceToHost));
            parts = 0;
            for (int32_t g = 0; g < G; g++)
                if (p->h_meta[g].ids_grp == g) parts += rec[(size_t)g * pdq::FAN_STRIDE + pdq::FAN_NPARTS];
        }
        out[11] = (float)parts;
    }
    return n;
}

int ca_estimate_plan_set_phase_timing(ca_estimate_plan* p, int32_t on) {
    if (!p) return CA_EINVAL;
    p->phase_events = on != 0;
    return CA_OK;
}

int ca_estimate_plan_group_ticks(const ca_estimate_plan* p, uint64_t* out, int32_t cap) {
    if (!p || (cap > 0 && !out)) return CA_EINVAL;
    const int32_t n = (int32_t)p->diag.size();
    for (int32_t i = 0; i < n && i < cap; i++) out[i] = p->diag[i];
    return n;
}

int ca_estimate_plan_chain_info(const ca_estimate_plan* p, int32_t* lin_sensitive, int32_t* had_success) {
    if (!p) return CA_EINVAL;
    if (lin_sensitive) *lin_sensitive = p->stats.lin_sensitive;
    if (had_success) *had_success = p->stats.had_success;
    return CA_OK;
}

int ca_estimate_batch(ca_mirror* m, const ca_podset* s, const int32_t* group_off, const int32_t* pod_idx,
                      const ca_template* templates, int32_t n_groups, const ca_limiter* limiter, int32_t* last_index,
                      ca_estimate_result* results, int32_t* sched_pod, int32_t* sched_node) {
    ca_estimate_plan* p = nullptr;
    int rc = ca_estimate_plan_create(m, s, group_off, pod_idx, templates, n_groups, &p);
    if (rc != CA_OK) return rc;
    rc = ca_estimate_plan_run(p, limiter, last_index, results, sched_pod, sched_node);
    ca_estimate_plan_destroy(p);
    return rc;
}

int ca_go_sort_ranks(int32_t device, const uint32_t* ranks, int32_t n, int32_t store, int32_t limit, int32_t* perm) {
    if (n < 0 || (n > 0 && (!ranks || !perm)) || store < 0 || store > 3) return CA_EINVAL;
    if (n == 0) return CA_OK;
    CA_HIP_CHECK(hipSetDevice(device));
    DevBuf meta, rk, sorted, e, scr, stack;
    int rc;
    if ((rc = meta.reserve(sizeof(GroupMeta))) != CA_OK || (rc = rk.reserve(sizeof(uint32_t) * (size_t)n)) != CA_OK ||
        (rc = sorted.reserve(sizeof(uint32_t) * (size_t)n)) != CA_OK ||
        (rc = e.reserve(sizeof(uint64_t) * (size_t)n)) != CA_OK || (rc = scr.reserve(sizeof(uint64_t) * (size_t)n)) != CA_OK ||
        (rc = stack.reserve(sizeof(pdq::Frame) * ((size_t)n / 2 + 4))) != CA_OK)
        return rc;
    GroupMeta gm = {};
    gm.off = 0;
    gm.count = n;
    CA_HIP_CHECK(hipMemcpy(meta.ptr, &gm, sizeof(gm), hipMemcpyHostToDevice));
    CA_HIP_CHECK(hipMemcpy(rk.ptr, ranks, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice));
    const int32_t lds_n = std::min(n, PDQ_LDS_N);
    const size_t lds = pdq_lds_bytes(lds_n);
    if ((rc = ensure_dyn_lds((const void*)k_pdq_sort, lds)) != CA_OK) return rc;
    hipLaunchKernelGGL(k_pdq_sort, dim3(1), dim3(pdq::NT), lds, 0, meta.as<GroupMeta>(), nullptr, nullptr, nullptr, 0,
                       rk.as<uint32_t>(), sorted.as<uint32_t>(), e.as<uint64_t>(), scr.as<uint64_t>(),
                       stack.as<pdq::Frame>(), lds_n, store, std::max(limit, 0), nullptr, nullptr, nullptr, 0,
                       (const int32_t*)nullptr, (const ca_template*)nullptr, (const int64_t*)nullptr, 0, 0, 0, 0);
    CA_HIP_CHECK(hipGetLastError());
    CA_HIP_CHECK(hipMemcpy(perm, sorted.ptr, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return CA_OK;
}

int ca_go_sort_ranks_fan(int32_t device, const uint32_t* ranks, int32_t n, int32_t parts, int32_t top_steps,
                         int32_t limit, int32_t* perm, int32_t* parts_out) {
    if (n < 0 || n > PDQ_LDS_N || (n > 0 && (!ranks || !perm)) || parts < 1 || parts > pdq::FAN_PARTS_MAX ||
        top_steps < 1 || top_steps > pdq::FAN_STEPS_MAX)
        return CA_EINVAL;
    for (int32_t i = 0; i < n; i++)
        if (ranks[i] >= 256) return CA_EINVAL;
    if (parts_out) *parts_out = 0;
    if (n == 0) return CA_OK;
    CA_HIP_CHECK(hipSetDevice(device));
    DevBuf meta, rk, sorted, e, scr, stack, pstack, fan;
    int rc;
    if ((rc = meta.reserve(sizeof(GroupMeta))) != CA_OK || (rc = rk.reserve(sizeof(uint32_t) * (size_t)n)) != CA_OK ||
        (rc = sorted.reserve(sizeof(uint32_t) * (size_t)n)) != CA_OK ||
        (rc = e.reserve(sizeof(uint64_t) * (size_t)n)) != CA_OK || (rc = scr.reserve(sizeof(uint64_t) * (size_t)n)) != CA_OK ||
        (rc = stack.reserve(sizeof(pdq::Frame) * ((size_t)n / 2 + 4))) != CA_OK ||
        (rc = pstack.reserve(sizeof(pdq::Frame) * ((size_t)n / 2 + 2 * pdq::FAN_PARTS_MAX + 4))) != CA_OK ||
        (rc = fan.reserve(sizeof(int32_t) * pdq::FAN_STRIDE)) != CA_OK)
        return rc;
    GroupMeta gm = {};
    gm.off = 0;
    gm.count = n;
    CA_HIP_CHECK(hipMemcpy(meta.ptr, &gm, sizeof(gm), hipMemcpyHostToDevice));
    CA_HIP_CHECK(hipMemcpy(rk.ptr, ranks, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice));
    CA_HIP_CHECK(hipMemset(fan.ptr, 0, sizeof(int32_t) * pdq::FAN_STRIDE));
    const int32_t lds_n = n;
    const size_t lds = pdq_lds_bytes(lds_n);
    if ((rc = ensure_dyn_lds((const void*)k_pdq_sort, lds)) != CA_OK) return rc;
    if ((rc = ensure_dyn_lds((const void*)k_pdq_sort_parts, lds)) != CA_OK) return rc;
    // every length fans here (fan_min -1): a root of at most T_SMALL positions is handed
    // over as a short frame
    hipLaunchKernelGGL(k_pdq_sort, dim3(1), dim3(pdq::NT), lds, 0, meta.as<GroupMeta>(), nullptr, nullptr, nullptr, 0,
                       rk.as<uint32_t>(), sorted.as<uint32_t>(), e.as<uint64_t>(), scr.as<uint64_t>(),
                       stack.as<pdq::Frame>(), lds_n, 1, std::max(limit, 0), nullptr, nullptr, fan.as<int32_t>(), 1,
                       (const int32_t*)nullptr, (const ca_template*)nullptr, (const int64_t*)nullptr, 0, parts, -1,
                       top_steps);
    CA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pdq_sort_parts, dim3(parts, 1), dim3(pdq::NT), lds, 0, meta.as<GroupMeta>(), nullptr,
                       sorted.as<uint32_t>(), e.as<uint64_t>(), stack.as<pdq::Frame>(), pstack.as<pdq::Frame>(), lds_n,
                       (const int32_t*)nullptr, (int32_t*)nullptr, fan.as<int32_t>(), 1);
    CA_HIP_CHECK(hipGetLastError());
    CA_HIP_CHECK(hipMemcpy(perm, sorted.ptr, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    int32_t rec[pdq::FAN_STRIDE];
    CA_HIP_CHECK(hipMemcpy(rec, fan.ptr, sizeof(rec), hipMemcpyDeviceToHost));
    if (!rec[pdq::FAN_FANNED]) return CA_EINVAL;        // (not the LDS store: cannot happen for ranks < 256)
    if (parts_out) *parts_out = rec[pdq::FAN_NPARTS];
    return CA_OK;
}

#ifdef CASIM_PROF
int ca_debug_pdq_prof(uint64_t* out, int32_t reset) {
    CA_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(pdq::g_pdq_prof), sizeof(uint64_t) * (32 + 256)));
    CA_HIP_CHECK(hipMemcpyFromSymbol(out + 32 + 256, HIP_SYMBOL(pdq::g_pdq_pis), sizeof(uint64_t) * 8));
    CA_HIP_CHECK(hipMemcpyFromSymbol(out + 32 + 256 + 8, HIP_SYMBOL(pdq::g_pdq_wg), sizeof(uint64_t) * 3 * 128));
    if (reset) {
        static const uint64_t z[32 + 256] = {};
        CA_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(pdq::g_pdq_prof), z, sizeof z));
        CA_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(pdq::g_pdq_pis), z, sizeof(uint64_t) * 8));
    }
    return CA_OK;
}

// two-launch sort: out[3 g + k] = k_pdq_sort's workgroup of group g (kernel, prologue, spill +
// split cycles), then out[384 + 4 (16 g + j) + k] = part j of group g in k_pdq_sort_parts
// (load, steps, short frames, ids out); 384 + 8192 words, the parts' zeroed after the copy
int ca_debug_pdq_fan_prof(uint64_t* out) {
    CA_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(pdq::g_pdq_wg), sizeof(uint64_t) * 3 * 128));
    CA_HIP_CHECK(hipMemcpyFromSymbol(out + 3 * 128, HIP_SYMBOL(pdq::g_pdq_part), sizeof(uint64_t) * 4 * 128 * 16));
    static const uint64_t z[4 * 128 * 16] = {};
    CA_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(pdq::g_pdq_part), z, sizeof z));
    return CA_OK;
}

int ca_debug_chain_prof(uint64_t* out, int32_t n_groups) {
    if (n_groups > 1024) n_groups = 1024;
    CA_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chain_prof), sizeof(uint64_t) * NPROF * (size_t)n_groups));
    return CA_OK;
}
int ca_debug_rt_prof(uint64_t* out, int32_t n_groups) {     // k_run_table phases: 3 per group
    if (n_groups > 1024) n_groups = 1024;
    CA_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rt_prof), sizeof(uint64_t) * 3 * (size_t)n_groups));
    return CA_OK;
}
#endif

}  // extern "C"
