// Pod equivalence groups on the device (ca_pod_groups_*; DESIGN.md §4 "pod groups").
//
// equivalence.BuildPodGroups (core/scaleup/equivalence/groups.go:38-102) on the interned
// records: a pod without a controller (similar_class < 0) or of a DaemonSet is a group of its
// own; the pods of one similar class (controller UID + labels + spec) share a group, for at
// most 10 classes per controller, taken in the order their first pods occur; a pod of a later
// class is a group of its own every time.  Groups are in the order of their first pods, pods
// inside a group in input order.  The loop is sequential in the reference; here it is
//   1. compact   the unschedulable positions u (tile counts, one scan over tiles, in-tile ranks)
//   2. first     first[c] = min u over the eligible pods of class c (atomicMin: a minimum
//                does not depend on the order it is taken in)
//   3. cap       class c is registered iff fewer than 10 classes of its owner have a smaller
//                first[] (one wave per owner: ten passes, each the next smallest first[])
//   4. leaders   a pod leads a group unless it is a later pod of a registered class; group id
//                = exclusive scan of the leader flags, a follower takes its class's id
//   5. place     eg_pod = the pods in a stable order by group id: least-significant-digit
//                passes of 8 bits (per-tile digit histograms, a scan over [digit][tile], in-tile
//                ranks from wave ballots); eg_off from the boundaries of the sorted ids.
// A pod's slot is the number of earlier pods of its group and nothing else: no slot is handed
// out by an atomic counter.  Integer and bit operations only; the number of launches depends
// on n (one sort pass per byte of n - 1) and on whether class_owner is given, not on the data.
#include "mirror.h"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

using namespace casim;

namespace {

constexpr int PG_TILE = 2048;          // positions per workgroup pass (abi.POD_GROUP_TILE)
constexpr int PG_PER = PG_TILE / 256;  // positions per thread
constexpr int32_t PG_INF = INT32_MAX;  // first[] of a class without an unschedulable pod
constexpr int PG_MAX_PER_OWNER = 10;   // groups.go:57

// device counters of one build
enum { PGC_NU = 0, PGC_NEG = 1, PGC_SORTED = 2, PGC_N = 4 };   // unschedulable pods, groups, a sort pass's total (= NU)

// inclusive scan of one value per thread over the 256 threads of a block (wsum: 4 words of LDS;
// a barrier must separate two calls)
__device__ inline int32_t pg_block_scan(int32_t v, int32_t* wsum) {
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

__global__ void __launch_bounds__(256) k_pg_fill(int32_t* __restrict__ a, int32_t n, int32_t v) {
    for (int32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) a[i] = v;
}

// exclusive scan of a[0 .. len) in place by one workgroup; the total goes to *total
__global__ void __launch_bounds__(256) k_pg_scan(int32_t* __restrict__ a, int32_t len, int32_t* __restrict__ total) {
    __shared__ int32_t wsum[4];
    int32_t running = 0;
    for (int32_t base = 0; base < len; base += 256) {
        const int32_t i = base + (int32_t)threadIdx.x;
        const int32_t v = i < len ? a[i] : 0;
        const int32_t x = pg_block_scan(v, wsum);
        if (i < len) a[i] = running + x - v;
        running += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = running;
}

__device__ inline bool pg_listed(const int32_t* node, int32_t k) { return node == nullptr || node[k] < 0; }

// 1a. unschedulable positions per tile (thread t of a tile holds positions base + 8t .. 8t + 7)
__global__ void __launch_bounds__(256) k_pg_count(const int32_t* __restrict__ node, int32_t n, int32_t* __restrict__ tile_cnt) {
    __shared__ int32_t wsum[4];
    const int32_t p0 = (int32_t)blockIdx.x * PG_TILE + (int32_t)threadIdx.x * PG_PER;
    int32_t c = 0;
    for (int j = 0; j < PG_PER; j++)
        if (p0 + j < n && pg_listed(node, p0 + j)) c++;
    (void)pg_block_scan(c, wsum);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// 1b + 2. u of every unschedulable position: its pod and its eligible class (or -1), and the
// class's first occurrence
__global__ void __launch_bounds__(256) k_pg_compact(const int32_t* __restrict__ node, const int32_t* __restrict__ order,
                                                    int32_t n, const ca_pod_spec* __restrict__ spec,
                                                    const int32_t* __restrict__ tile_base, int32_t* __restrict__ upod,
                                                    int32_t* __restrict__ ucls, int32_t* __restrict__ first, int32_t n_cls) {
    __shared__ int32_t wsum[4];
    const int32_t p0 = (int32_t)blockIdx.x * PG_TILE + (int32_t)threadIdx.x * PG_PER;
    int32_t c = 0;
    for (int j = 0; j < PG_PER; j++)
        if (p0 + j < n && pg_listed(node, p0 + j)) c++;
    int32_t u = tile_base[blockIdx.x] + pg_block_scan(c, wsum) - c;
    for (int j = 0; j < PG_PER; j++) {
        const int32_t k = p0 + j;
        if (k >= n || !pg_listed(node, k)) continue;
        const int32_t i = order ? order[k] : k;
        int32_t cl = spec[i].similar_class;
        if (cl < 0 || cl >= n_cls || (spec[i].flags & CA_POD_DAEMONSET)) cl = -1;   // (cl >= n_cls: refused by the host)
        upod[u] = i;
        ucls[u] = cl;
        if (cl >= 0) atomicMin(&first[cl], u);
        u++;
    }
}

// 3. one wave per owner over its classes owner_cls[owner_off[o] .. owner_off[o + 1]): the tenth
// smallest first[] is the last registered one
__global__ void __launch_bounds__(256) k_pg_cap(const int32_t* __restrict__ owner_off, const int32_t* __restrict__ owner_cls,
                                                int32_t n_owners, const int32_t* __restrict__ first,
                                                uint8_t* __restrict__ reg) {
    const int lane = threadIdx.x & 63;
    const int32_t o = (int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6);
    if (o >= n_owners) return;
    const int32_t a = owner_off[o], b = owner_off[o + 1];
    int32_t thr = -1;
    bool all = false;
    for (int r = 0; r < PG_MAX_PER_OWNER; r++) {
        int32_t mn = PG_INF;
        for (int32_t j = a + lane; j < b; j += 64) {
            const int32_t f = first[owner_cls[j]];
            if (f > thr && f < mn) mn = f;
        }
        for (int s = 32; s > 0; s >>= 1) mn = min(mn, __shfl_xor(mn, s, 64));
        if (mn == PG_INF) { all = true; break; }
        thr = mn;
    }
    if (all) thr = PG_INF - 1;
    for (int32_t j = a + lane; j < b; j += 64) {
        const int32_t c = owner_cls[j];
        reg[c] = first[c] <= thr ? 1 : 0;
    }
}

__device__ inline bool pg_leader(int32_t u, int32_t cl, const int32_t* first, const uint8_t* reg) {
    return cl < 0 || (reg && !reg[cl]) || first[cl] == u;
}

// 4a. leaders per tile of u
__global__ void __launch_bounds__(256) k_pg_lead_count(const int32_t* __restrict__ cnt, const int32_t* __restrict__ ucls,
                                                       const int32_t* __restrict__ first, const uint8_t* __restrict__ reg,
                                                       int32_t* __restrict__ tile_cnt) {
    __shared__ int32_t wsum[4];
    const int32_t nu = cnt[PGC_NU];
    const int32_t p0 = (int32_t)blockIdx.x * PG_TILE + (int32_t)threadIdx.x * PG_PER;
    int32_t c = 0;
    for (int j = 0; j < PG_PER; j++)
        if (p0 + j < nu && pg_leader(p0 + j, ucls[p0 + j], first, reg)) c++;
    (void)pg_block_scan(c, wsum);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// 4b. the leaders' group ids; a registered class's id is kept for its followers
__global__ void __launch_bounds__(256) k_pg_lead_ids(const int32_t* __restrict__ cnt, const int32_t* __restrict__ ucls,
                                                     const int32_t* __restrict__ first, const uint8_t* __restrict__ reg,
                                                     const int32_t* __restrict__ tile_base, int32_t* __restrict__ key,
                                                     int32_t* __restrict__ cls_gid) {
    __shared__ int32_t wsum[4];
    const int32_t nu = cnt[PGC_NU];
    const int32_t p0 = (int32_t)blockIdx.x * PG_TILE + (int32_t)threadIdx.x * PG_PER;
    int32_t c = 0;
    for (int j = 0; j < PG_PER; j++)
        if (p0 + j < nu && pg_leader(p0 + j, ucls[p0 + j], first, reg)) c++;
    int32_t g = tile_base[blockIdx.x] + pg_block_scan(c, wsum) - c;
    for (int j = 0; j < PG_PER; j++) {
        const int32_t u = p0 + j;
        if (u >= nu) break;
        const int32_t cl = ucls[u];
        if (!pg_leader(u, cl, first, reg)) { key[u] = -1; continue; }
        key[u] = g;
        if (cl >= 0 && first[cl] == u && !(reg && !reg[cl])) cls_gid[cl] = g;
        g++;
    }
}

// 4c. the followers' group ids
__global__ void __launch_bounds__(256) k_pg_follow(const int32_t* __restrict__ cnt, const int32_t* __restrict__ ucls,
                                                   const int32_t* __restrict__ cls_gid, int32_t* __restrict__ key) {
    const int32_t nu = cnt[PGC_NU];
    for (int32_t u = blockIdx.x * 256 + threadIdx.x; u < nu; u += gridDim.x * 256)
        if (key[u] < 0) key[u] = cls_gid[ucls[u]];
}

// 5a. digit histogram of a tile, stored [digit][tile] so that one linear scan gives every
// (digit, tile) its first output position
__global__ void __launch_bounds__(256) k_pg_hist(const int32_t* __restrict__ cnt, const int32_t* __restrict__ key,
                                                 int32_t shift, int32_t n_tiles, int32_t* __restrict__ hist) {
    __shared__ int32_t h[256];
    const int32_t nu = cnt[PGC_NU];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int32_t base = (int32_t)blockIdx.x * PG_TILE;
    for (int r = 0; r < PG_PER; r++) {
        const int32_t u = base + r * 256 + (int32_t)threadIdx.x;
        if (u < nu) atomicAdd(&h[(key[u] >> shift) & 255], 1);      // (a count: order-free)
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * (size_t)n_tiles + blockIdx.x] = h[threadIdx.x];
}

// 5b. stable scatter of a tile: rounds of 256 keys in position order; inside a round a key's
// rank among the keys of its digit is (keys of the digit in earlier waves) + (earlier lanes of
// its wave with the digit: eight ballots give the lanes with an equal digit)
__global__ void __launch_bounds__(256) k_pg_scatter(const int32_t* __restrict__ cnt, const int32_t* __restrict__ key,
                                                    const int32_t* __restrict__ val, int32_t shift, int32_t n_tiles,
                                                    const int32_t* __restrict__ hist, int32_t* __restrict__ key_out,
                                                    int32_t* __restrict__ val_out) {
    __shared__ int32_t run[256], wh[4][256];
    const int32_t nu = cnt[PGC_NU];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    run[threadIdx.x] = hist[(size_t)threadIdx.x * (size_t)n_tiles + blockIdx.x];
    for (int q = 0; q < 4; q++) wh[q][threadIdx.x] = 0;
    __syncthreads();
    const int32_t base = (int32_t)blockIdx.x * PG_TILE;
    for (int r = 0; r < PG_PER; r++) {
        if (base + r * 256 >= nu) break;                             // (uniform over the block)
        const int32_t u = base + r * 256 + (int32_t)threadIdx.x;
        const bool valid = u < nu;
        const int32_t k = valid ? key[u] : 0, v = valid ? val[u] : 0;
        const int32_t d = (k >> shift) & 255;
        unsigned long long peers = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const unsigned long long bal = __ballot((d >> b) & 1);
            peers &= ((d >> b) & 1) ? bal : ~bal;
        }
        const int32_t before = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && before == 0) wh[w][d] = __popcll(peers);        // the digit's first lane of the wave
        __syncthreads();
        if (valid) {
            int32_t pos = run[d] + before;
            for (int q = 0; q < w; q++) pos += wh[q][d];
            key_out[pos] = k;
            val_out[pos] = v;
        }
        __syncthreads();
        {
            int32_t add = 0;
            for (int q = 0; q < 4; q++) { add += wh[q][threadIdx.x]; wh[q][threadIdx.x] = 0; }
            run[threadIdx.x] += add;
        }
        __syncthreads();
    }
}

// 5c. the sorted ids' boundaries: eg_off[g] = first position of id g, eg_off[n_eg] = n_u; the
// sample of group g (its first pod) beside it
__global__ void __launch_bounds__(256) k_pg_offsets(const int32_t* __restrict__ cnt, const int32_t* __restrict__ key,
                                                    const int32_t* __restrict__ val, int32_t* __restrict__ eg_off,
                                                    int32_t* __restrict__ samples) {
    const int32_t nu = cnt[PGC_NU];
    for (int32_t u = blockIdx.x * 256 + threadIdx.x; u <= nu; u += gridDim.x * 256) {
        if (u == nu) { eg_off[cnt[PGC_NEG]] = nu; continue; }
        const int32_t k = key[u];
        if (u == 0 || key[u - 1] != k) { eg_off[k] = u; samples[k] = val[u]; }
    }
}

int32_t grid_for(int64_t n) { return (int32_t)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256)); }

}  // namespace

extern "C" {

int ca_pod_groups_create(ca_mirror* m, const ca_podset* s, const int32_t* order, int32_t n, const int32_t* node,
                         const int32_t* class_owner, int32_t n_classes, ca_pod_groups** out) {
    if (out) *out = nullptr;
    if (!m || !s || !out || s->m != m || n < 0 || n_classes < 0) return CA_EINVAL;
    if (!order && n > s->t.n_pods) return CA_EINVAL;
    // every check before any launch or allocation (order and node are the caller's arrays; the
    // classes come from the pod set's compact host column, not from the records)
    if (class_owner)
        for (int32_t c = 0; c < n_classes; c++)
            if (class_owner[c] < 0) return CA_EINVAL;
    const int32_t np_ = s->t.n_pods;
    for (int32_t k = 0; k < n; k++) {
        const int32_t i = order ? order[k] : k;
        if ((uint32_t)i >= (uint32_t)np_) return CA_EINVAL;
        if (class_owner && (!node || node[k] < 0) && s->h_sim[(size_t)i] >= n_classes) return CA_EINVAL;
    }
    const int32_t NC = class_owner ? n_classes : s->n_sim;      // classes an eligible pod can carry
    // the owners' classes as a CSR (a pass over the classes); owner ids need not be dense
    std::vector<int32_t> owner_off, owner_cls;
    int32_t n_owners = 0;
    if (class_owner && NC > 0) {
        std::vector<std::pair<int32_t, int32_t>> oc((size_t)NC);
        for (int32_t c = 0; c < NC; c++) oc[(size_t)c] = {class_owner[c], c};
        std::sort(oc.begin(), oc.end());
        owner_cls.resize((size_t)NC);
        for (int32_t j = 0; j < NC; j++) {
            if (j == 0 || oc[(size_t)j].first != oc[(size_t)j - 1].first) owner_off.push_back(j);
            owner_cls[(size_t)j] = oc[(size_t)j].second;
        }
        n_owners = (int32_t)owner_off.size();
        owner_off.push_back(NC);
    }
    CA_HIP_CHECK(hipSetDevice(m->device));
    ca_pod_groups* g = new ca_pod_groups();
    g->m = m;
    g->s = s;
    g->device = m->device;
    int rc = CA_OK;
    auto fail = [&](int code) { (void)hipStreamSynchronize(m->stream); delete g; return code; };
    if (hipEventCreate(&g->ev0) != hipSuccess || hipEventCreate(&g->ev1) != hipSuccess) {
        set_last_error("ca_pod_groups_create: event creation failed");
        return fail(CA_EDEVICE);
    }
    // the result: eg_off [n + 1] | samples [n] | eg_pod [n] (at most n groups of at most n pods)
    const size_t N = (size_t)std::max(n, 1);
    if ((rc = g->d_out.reserve(sizeof(int32_t) * (3 * N + 1))) != CA_OK) return fail(rc);
    g->d_eg_off = g->d_out.as<int32_t>();
    g->d_samples = g->d_eg_off + N + 1;
    g->d_eg_pod = g->d_samples + N;
    g->h_eg_off.assign(1, 0);
    if (n == 0) {
        if (hipMemsetAsync(g->d_eg_off, 0, sizeof(int32_t), m->stream) != hipSuccess ||
            hipStreamSynchronize(m->stream) != hipSuccess) {
            set_last_error("ca_pod_groups_create: clearing the offsets failed");
            return fail(CA_EDEVICE);
        }
        *out = g;
        return CA_OK;
    }
    hipStream_t st = m->stream;
    const int32_t n_tiles = (n + PG_TILE - 1) / PG_TILE;
    const size_t NCa = (size_t)std::max(NC, 1);
    // scratch words: counters | tile counts | hist [256][tiles] | order | node | upod | ucls | key A | key B | val B |
    // first | class ids | owner CSR ; then the registered bytes
    DevBuf d_w;
    const size_t o_cnt = 0, o_tile = o_cnt + PGC_N, o_hist = o_tile + (size_t)n_tiles, o_order = o_hist + 256 * (size_t)n_tiles,
                 o_node = o_order + N, o_upod = o_node + N, o_ucls = o_upod + N, o_keyA = o_ucls + N, o_keyB = o_keyA + N,
                 o_valB = o_keyB + N, o_first = o_valB + N, o_cgid = o_first + NCa, o_ooff = o_cgid + NCa,
                 o_ocls = o_ooff + (size_t)n_owners + 1, o_reg = o_ocls + NCa, words = o_reg + (NCa + 3) / 4;
    if ((rc = d_w.reserve(sizeof(int32_t) * words)) != CA_OK) return fail(rc);
    int32_t* W = d_w.as<int32_t>();
    int32_t *cnt = W + o_cnt, *tile = W + o_tile, *hist = W + o_hist, *d_order = order ? W + o_order : nullptr,
            *d_node = node ? W + o_node : nullptr, *upod = W + o_upod, *ucls = W + o_ucls, *keyA = W + o_keyA,
            *keyB = W + o_keyB, *valB = W + o_valB, *first = W + o_first, *cgid = W + o_cgid, *d_ooff = W + o_ooff,
            *d_ocls = W + o_ocls;
    uint8_t* reg = class_owner && NC > 0 ? reinterpret_cast<uint8_t*>(W + o_reg) : nullptr;
#define PG_CHECK(expr)                                                              \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess) {                                                     \
            set_last_error(std::string(#expr) + ": " + hipGetErrorString(_e));      \
            return fail(CA_EDEVICE);                                                \
        }                                                                           \
    } while (0)
    if (order) PG_CHECK(hipMemcpyAsync(d_order, order, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    if (node) PG_CHECK(hipMemcpyAsync(d_node, node, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    if (reg) {
        PG_CHECK(hipMemcpyAsync(d_ooff, owner_off.data(), sizeof(int32_t) * owner_off.size(), hipMemcpyHostToDevice, st));
        PG_CHECK(hipMemcpyAsync(d_ocls, owner_cls.data(), sizeof(int32_t) * owner_cls.size(), hipMemcpyHostToDevice, st));
    }
    int32_t launches = 0;
#define PG_LAUNCH(kernel, grid, ...)                                                \
    do {                                                                            \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, __VA_ARGS__);      \
        PG_CHECK(hipGetLastError());                                                \
        launches++;                                                                 \
    } while (0)
    PG_CHECK(hipEventRecord(g->ev0, st));
    if (NC > 0) PG_LAUNCH(k_pg_fill, grid_for(NC), first, NC, PG_INF);
    PG_LAUNCH(k_pg_count, n_tiles, d_node, n, tile);
    PG_LAUNCH(k_pg_scan, 1, tile, n_tiles, cnt + PGC_NU);
    PG_LAUNCH(k_pg_compact, n_tiles, d_node, d_order, n, s->t.spec.as<ca_pod_spec>(), tile, upod, ucls, first, NC);
    if (reg) PG_LAUNCH(k_pg_cap, (n_owners + 3) / 4, d_ooff, d_ocls, n_owners, first, reg);
    PG_LAUNCH(k_pg_lead_count, n_tiles, cnt, ucls, first, reg, tile);
    PG_LAUNCH(k_pg_scan, 1, tile, n_tiles, cnt + PGC_NEG);
    PG_LAUNCH(k_pg_lead_ids, n_tiles, cnt, ucls, first, reg, tile, keyA, cgid);
    PG_LAUNCH(k_pg_follow, grid_for(n), cnt, ucls, cgid, keyA);
    // one pass per byte of the largest possible id, n - 1; the last pass lands in eg_pod
    int passes = 1;
    while (passes < 4 && ((int64_t)(n - 1) >> (8 * passes)) != 0) passes++;
    const int32_t *kin = keyA, *vin = upod;
    int32_t* kout = keyB;
    for (int p = 0; p < passes; p++) {
        // values alternate so that the last pass writes eg_pod: ... -> valB -> eg_pod
        int32_t* vout = ((passes - 1 - p) & 1) ? valB : g->d_eg_pod;
        PG_LAUNCH(k_pg_hist, n_tiles, cnt, kin, 8 * p, n_tiles, hist);
        PG_LAUNCH(k_pg_scan, 1, hist, 256 * n_tiles, cnt + PGC_SORTED);
        PG_LAUNCH(k_pg_scatter, n_tiles, cnt, kin, vin, 8 * p, n_tiles, hist, kout, vout);
        kin = kout; vin = vout;
        kout = (kout == keyB) ? keyA : keyB;
    }
    PG_LAUNCH(k_pg_offsets, grid_for((int64_t)n + 1), cnt, kin, vin, g->d_eg_off, g->d_samples);
    PG_CHECK(hipEventRecord(g->ev1, st));
    int32_t h_cnt[PGC_N] = {0, 0, 0, 0};
    PG_CHECK(hipMemcpyAsync(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    PG_CHECK(hipStreamSynchronize(st));
    g->n_pods = h_cnt[PGC_NU];
    g->n_eg = h_cnt[PGC_NEG];
    if (g->n_pods < 0 || g->n_pods > n || g->n_eg < 0 || g->n_eg > g->n_pods) {
        set_last_error("ca_pod_groups_create: inconsistent counts from the device");
        return fail(CA_EDEVICE);
    }
    g->h_eg_off.assign((size_t)g->n_eg + 1, 0);
    g->h_eg_pod.assign((size_t)g->n_pods, 0);
    if (g->n_eg > 0) {
        PG_CHECK(hipMemcpyAsync(g->h_eg_off.data(), g->d_eg_off, sizeof(int32_t) * ((size_t)g->n_eg + 1), hipMemcpyDeviceToHost, st));
        PG_CHECK(hipMemcpyAsync(g->h_eg_pod.data(), g->d_eg_pod, sizeof(int32_t) * (size_t)g->n_pods, hipMemcpyDeviceToHost, st));
    } else {
        PG_CHECK(hipMemsetAsync(g->d_eg_off, 0, sizeof(int32_t), st));
    }
    PG_CHECK(hipStreamSynchronize(st));
    PG_CHECK(hipEventElapsedTime(&g->build_ms, g->ev0, g->ev1));
    g->launches = launches;
#undef PG_LAUNCH
#undef PG_CHECK
    *out = g;
    return CA_OK;
}

int ca_pod_groups_info(const ca_pod_groups* g, int32_t* n_eg, int32_t* n_pods) {
    if (!g) return CA_EINVAL;
    if (n_eg) *n_eg = g->n_eg;
    if (n_pods) *n_pods = g->n_pods;
    return CA_OK;
}

int ca_pod_groups_fetch(const ca_pod_groups* g, int32_t* eg_off, int32_t* eg_pod) {
    if (!g) return CA_EINVAL;
    if (eg_off) std::memcpy(eg_off, g->h_eg_off.data(), sizeof(int32_t) * ((size_t)g->n_eg + 1));
    if (eg_pod && g->n_pods > 0) std::memcpy(eg_pod, g->h_eg_pod.data(), sizeof(int32_t) * (size_t)g->n_pods);
    return CA_OK;
}

int ca_pod_groups_timings(const ca_pod_groups* g, float* out, int32_t cap) {
    if (!g || (cap > 0 && !out)) return CA_EINVAL;
    if (cap > 0) out[0] = g->build_ms;
    if (cap > 1) out[1] = (float)g->launches;
    return 2;
}

int ca_pod_groups_destroy(ca_pod_groups* g) {
    if (!g) return CA_EINVAL;
    (void)hipSetDevice(g->device);
    delete g;
    return CA_OK;
}

}  // extern "C"
