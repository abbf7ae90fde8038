// nodegroupset.hip — the statement of ScaleUp after ExpanderStrategy.BestOption that reads the
// options' pod lists again: filterNodeGroupsByPods
// (CA/core/scaleup/orchestrator/orchestrator.go:293, body :596-628), on the Estimate plan's
// device-resident lists (DESIGN.md §4 "Similar node groups").
//
//   ca_estimate_plan_groups_missing_pods   per candidate group: how many positions of the
//                                          required group's list name a pod the candidate's list
//                                          lacks, and the first such position
//
// The reference builds one map[*Pod]bool per candidate; here a candidate is one bitmap row over
// the pod set (k_mark_lists) and the required list is tested against every row
// (k_test_required).  Pods are compared by pod-set index.
//
// The body is casim::estimate_plan_missing_pods, which takes the required list as a
// (device pointer, total, offset, n) source: the plan's own group for the entry point above, a
// list exported by another device's plan and uploaded here for the sharded plan (multi.hip:
// estimate_plan_export_list / estimate_plan_missing_pods_of).
#include "mirror.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace casim {
namespace {

// Both kernels tile a list as k_option_sums does (expander.hip): tiles are cut at multiples of
// 4 ids from the list buffer's base, every lane loads aligned 16-byte quads, and the positions
// before the group's offset (the previous group's) and from n_scheduled on (stale ids of an
// earlier, longer run, or -1) are masked.
constexpr int MP_THREADS = 256;
constexpr int MP_QUADS = 2;                                // 16-byte loads per lane
constexpr int MP_TILE = MP_THREADS * MP_QUADS * 4;         // 2048 ids, 8 KB
constexpr int MP_ROWS = 64;                                // most rows one k_test_required block walks
constexpr int64_t MP_BLOCK_TESTS = 16384;                  // bit tests a block should at least have
constexpr int64_t MP_GRID_TARGET = 512;                    // blocks wanted before a block takes more rows
constexpr size_t MP_SCRATCH_DEFAULT = (size_t)64 << 20;    // bitmap rows resident at once, bytes

// The tile's ids and which of them are counted positions of the list [a, e).  ok bit 4q + j.
struct TileIds {
    int32_t id[MP_QUADS * 4];
    uint32_t ok;
};

__device__ inline TileIds load_tile(const int32_t* __restrict__ sched_pod, int32_t total, int64_t base, int32_t a,
                                    int32_t e, int32_t tid) {
    TileIds t;
    t.ok = 0;
#pragma unroll
    for (int q = 0; q < MP_QUADS; q++) {
        const int64_t i = base + (q * MP_THREADS + tid) * 4;
#pragma unroll
        for (int j = 0; j < 4; j++) t.id[4 * q + j] = -1;
        if (i >= e) continue;
        if (i + 4 <= total) {
            const int4 v = *reinterpret_cast<const int4*>(sched_pod + i);
            t.id[4 * q] = v.x; t.id[4 * q + 1] = v.y; t.id[4 * q + 2] = v.z; t.id[4 * q + 3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) t.id[4 * q + j] = i + j < total ? sched_pod[i + j] : -1;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (i + j >= a && i + j < e) t.ok |= 1u << (4 * q + j);
    }
    return t;
}

// roff / rns / tpre: offset, n_scheduled and the exclusive prefix of the tile counts of every
// distinct candidate (a row), over all batches; this launch marks rows [r0, r1), whose tiles are
// tpre[r0] + blockIdx.x.  rows: (r1 - r0) x W words, zeroed.  bad: ids outside the pod set.
__global__ void __launch_bounds__(MP_THREADS) k_mark_lists(const int32_t* __restrict__ sched_pod, int32_t total,
                                                          const int32_t* __restrict__ roff,
                                                          const int32_t* __restrict__ rns,
                                                          const int32_t* __restrict__ tpre, int32_t r0, int32_t r1,
                                                          uint32_t* __restrict__ rows, int32_t W, int32_t n_pods,
                                                          uint32_t* __restrict__ bad) {
    __shared__ int32_t found[4];                  // the tile's row, its offset, n_scheduled, first tile
    const int32_t tid = (int32_t)threadIdx.x;
    if (tid == 0) found[0] = -1;
    __syncthreads();
    const int32_t b = tpre[r0] + (int32_t)blockIdx.x;
    // the row r with tpre[r] <= b < tpre[r + 1]: binary steps down to one candidate per lane,
    // then the lanes (as k_option_sums finds its group)
    int32_t lo = r0, hi = r1;
    while (hi - lo > MP_THREADS) {
        const int32_t mid = (lo + hi) >> 1;
        if (tpre[mid] <= b) lo = mid; else hi = mid;
    }
    if (lo + tid < hi) {
        const int32_t i = lo + tid;
        const int32_t t0 = tpre[i], t1 = tpre[i + 1];
        if (t0 <= b && b < t1) { found[0] = i; found[1] = roff[i]; found[2] = rns[i]; found[3] = t0; }
    }
    __syncthreads();
    const int32_t r = found[0];
    if (r < r0 || r >= r1) return;
    const int32_t a = found[1], e = a + found[2];
    if (a < 0 || e < a || e > total) return;     // (a table that does not describe the buffer must not become an address)
    const int64_t base = (int64_t)(a & ~3) + (int64_t)(b - found[3]) * MP_TILE;
    const TileIds t = load_tile(sched_pod, total, base, a, e, tid);
    uint32_t* row = rows + (size_t)(r - r0) * (size_t)W;
    uint32_t nbad = 0;
#pragma unroll
    for (int k = 0; k < MP_QUADS * 4; k++) {
        if (!(t.ok >> k & 1)) continue;
        const uint32_t id = (uint32_t)t.id[k];
        if (id >= (uint32_t)n_pods) { nbad++; continue; }
        atomicOr(&row[id >> 5], 1u << (id & 31));
    }
    if (nbad) atomicAdd(bad, nbad);
}

// Block (x, y): tile x of the required list [a, a + n), rows [y * rc, min(y * rc + rc, R)) of
// this batch.  n_missing / first: the batch's slice of the per-row results (first starts at
// INT32_MAX).  The tile's ids stay in registers; a row's word is read once per id (no reuse
// inside a block, so rows are not staged in LDS).
__global__ void __launch_bounds__(MP_THREADS) k_test_required(const int32_t* __restrict__ sched_pod, int32_t total,
                                                             int32_t a, int32_t n,
                                                             const uint32_t* __restrict__ rows, int32_t W, int32_t R,
                                                             int32_t rc, int32_t n_pods,
                                                             uint32_t* __restrict__ n_missing,
                                                             int32_t* __restrict__ first, uint32_t* __restrict__ bad) {
    __shared__ uint32_t s_cnt[MP_ROWS];
    __shared__ int32_t s_min[MP_ROWS];
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t e = a + n;
    if (a < 0 || n < 0 || e > total || rc < 1 || rc > MP_ROWS) return;
    const int32_t row0 = (int32_t)blockIdx.y * rc, row1 = min(row0 + rc, R);
    if (tid < MP_ROWS) { s_cnt[tid] = 0; s_min[tid] = INT32_MAX; }
    __syncthreads();
    const int64_t base = (int64_t)(a & ~3) + (int64_t)blockIdx.x * MP_TILE;
    TileIds t = load_tile(sched_pod, total, base, a, e, tid);
    uint32_t nbad = 0;
    uint32_t word[MP_QUADS * 4], bit[MP_QUADS * 4];
#pragma unroll
    for (int k = 0; k < MP_QUADS * 4; k++) {
        const uint32_t id = (uint32_t)t.id[k];
        if ((t.ok >> k & 1) && id >= (uint32_t)n_pods) { nbad++; t.ok &= ~(1u << k); }
        word[k] = (t.ok >> k & 1) ? id >> 5 : 0u;
        bit[k] = id & 31;
    }
    if (nbad && blockIdx.y == 0) atomicAdd(bad, nbad);
    // list position of this wave's lane 0 in quad q, element j: pos0 + q * MP_THREADS * 4 + j; a
    // lane further on adds 4 per lane, so a ballot's lowest lane holds its smallest position
    const int64_t pos0 = base + (int64_t)(tid & ~63) * 4 - a;
    for (int32_t r = row0; r < row1; r++) {
        const uint32_t* __restrict__ row = rows + (size_t)r * (size_t)W;
        uint32_t w[MP_QUADS * 4];
#pragma unroll
        for (int k = 0; k < MP_QUADS * 4; k++) w[k] = (t.ok >> k & 1) ? row[word[k]] : 0u;
        uint32_t cnt = 0;
        int64_t mn = INT32_MAX;
#pragma unroll
        for (int k = 0; k < MP_QUADS * 4; k++) {
            const bool miss = (t.ok >> k & 1) && !(w[k] >> bit[k] & 1);
            const unsigned long long m = __ballot(miss);
            if (m) {
                cnt += (uint32_t)__popcll(m);
                const int64_t pos = pos0 + (int64_t)(k >> 2) * MP_THREADS * 4 + (int64_t)(__ffsll(m) - 1) * 4 + (k & 3);
                mn = pos < mn ? pos : mn;
            }
        }
        if (cnt && (tid & 63) == 0) {
            atomicAdd(&s_cnt[r - row0], cnt);
            atomicMin(&s_min[r - row0], (int32_t)mn);
        }
    }
    __syncthreads();
    if (tid < row1 - row0 && s_cnt[tid]) {
        atomicAdd(&n_missing[row0 + tid], s_cnt[tid]);
        atomicMin(&first[row0 + tid], s_min[tid]);
    }
}

}  // namespace
}  // namespace casim

namespace casim {

int estimate_plan_missing_pods(ca_estimate_plan* p, const RequiredList* ext, int32_t required_group,
                               const int32_t* groups, int32_t n_groups, int32_t* n_missing, int32_t* first_missing) {
    if (!p || n_groups < 0 || (n_groups > 0 && (!groups || !n_missing))) return CA_EINVAL;
    PlanLists v;
    estimate_plan_lists(p, &v);
    const int32_t G = v.G;
    if (ext) {
        if (ext->n < 0 || ext->off < 0 || (int64_t)ext->off + ext->n > ext->total || (ext->n > 0 && !ext->d_ids))
            return CA_EINVAL;
        required_group = -1;                               // no candidate is the required group itself
    } else if (required_group < 0 || required_group >= G) {
        return CA_EINVAL;
    }
    for (int32_t k = 0; k < n_groups; k++) if (groups[k] < 0 || groups[k] >= G) return CA_EINVAL;
    if (!v.final_lists) return CA_ESTATE;
    MissingPodsScratch& sc = *v.missing;
    sc.timed = false;
    if (n_groups == 0) return CA_OK;
    for (int32_t g = 0; g < G; g++) {
        const int32_t n = v.h_nsched[g];
        if (n < 0 || n > v.h_off[g + 1] - v.h_off[g]) { set_last_error("missing pods: n_scheduled outside its group"); return CA_EDEVICE; }
    }
    // the required list: the plan's own group, or the caller's source
    const int32_t* const req_ids = ext ? ext->d_ids : v.d_sched_pod;
    const int32_t req_total = ext ? ext->total : v.total;
    const int32_t req_a = ext ? ext->off : v.h_off[required_group];
    const int32_t req_n = ext ? ext->n : v.h_nsched[required_group];
    // Slots the lists' lengths answer: an empty required list is included in anything, a group
    // includes itself, an empty candidate misses every position.  No other inclusion follows
    // from the lengths (either list may repeat an id), so every other distinct candidate is a row.
    sc.row_of.assign((size_t)G, -1);
    std::vector<int32_t>& row_group = sc.row_group;
    row_group.clear();
    for (int32_t k = 0; k < n_groups; k++) {
        const int32_t g = groups[k];
        if (req_n == 0 || g == required_group) {
            n_missing[k] = 0;
            if (first_missing) first_missing[k] = -1;
        } else if (v.h_nsched[g] == 0) {
            n_missing[k] = req_n;
            if (first_missing) first_missing[k] = 0;
        } else if (sc.row_of[g] < 0) {
            sc.row_of[g] = (int32_t)row_group.size();
            row_group.push_back(g);
        }
    }
    const int32_t R = (int32_t)row_group.size();
    if (R == 0) return CA_OK;

    const int32_t n_pods = v.s->n_host;
    const int32_t W = std::max(1, (int32_t)(((int64_t)n_pods + 31) / 32));
    size_t cap = MP_SCRATCH_DEFAULT;
    if (const char* e = knob_env("CASIM_MISSING_SCRATCH")) cap = (size_t)std::max(0LL, atoll(e));
    const size_t row_bytes = (size_t)W * sizeof(uint32_t);
    if (cap < row_bytes) { set_last_error("missing pods: one bitmap row exceeds the scratch bound"); return CA_ECAPACITY; }
    const int32_t per_batch = (int32_t)std::min<size_t>(cap / row_bytes, (size_t)R);

    // d_in: [row offset | row n_scheduled | tile prefix (R + 1)]; d_out: [n_missing R | bad 1 | first R]
    const size_t n_in = 3 * (size_t)R + 1, n_out = 2 * (size_t)R + 1;
    const size_t out_at = (n_in * sizeof(int32_t) + 15) & ~(size_t)15;
    // the plan's device before any reserve: DevBuf allocates on the calling thread's current
    // device, and the sharded plan calls this on threads that have not chosen one (multi.hip)
    CA_HIP_CHECK(hipSetDevice(v.m->device));
    int rc;
    if ((rc = sc.h.reserve(out_at + n_out * sizeof(int32_t))) != CA_OK) return rc;
    if ((rc = sc.d_in.reserve(n_in * sizeof(int32_t))) != CA_OK) return rc;
    if ((rc = sc.d_out.reserve(n_out * sizeof(int32_t))) != CA_OK) return rc;
    if ((rc = sc.d_rows.reserve((size_t)per_batch * row_bytes)) != CA_OK) return rc;
    int32_t* roff = sc.h.as<int32_t>();
    int32_t* rns = roff + R;
    int32_t* tpre = rns + R;
    int64_t tiles = 0;
    for (int32_t r = 0; r < R; r++) {
        const int32_t a = v.h_off[row_group[r]], n = v.h_nsched[row_group[r]];
        roff[r] = a;
        rns[r] = n;
        tpre[r] = (int32_t)tiles;
        tiles += ((int64_t)(a + n) - (a & ~3) + MP_TILE - 1) / MP_TILE;
    }
    if (tiles > INT32_MAX) return CA_ECAPACITY;
    tpre[R] = (int32_t)tiles;
    const int64_t req_tiles = ((int64_t)(req_a + req_n) - (req_a & ~3) + MP_TILE - 1) / MP_TILE;
    int32_t* h_out = reinterpret_cast<int32_t*>(static_cast<char*>(sc.h.ptr) + out_at);

    hipStream_t st = v.m->stream;
    if (!sc.ev0) {
        CA_HIP_CHECK(hipEventCreate(&sc.ev0));
        CA_HIP_CHECK(hipEventCreate(&sc.ev1));
    }
    CA_HIP_CHECK(hipMemcpyAsync(sc.d_in.ptr, roff, n_in * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const int32_t* d_roff = sc.d_in.as<int32_t>();
    uint32_t* d_nmiss = sc.d_out.as<uint32_t>();
    uint32_t* d_bad = d_nmiss + R;
    int32_t* d_first = sc.d_out.as<int32_t>() + R + 1;
    CA_HIP_CHECK(hipMemsetAsync(d_nmiss, 0, ((size_t)R + 1) * sizeof(int32_t), st));
    CA_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_first), INT32_MAX, (size_t)R, st));
    CA_HIP_CHECK(hipEventRecord(sc.ev0, st));
    for (int32_t r0 = 0; r0 < R; r0 += per_batch) {
        const int32_t r1 = std::min(R, r0 + per_batch), nb = r1 - r0;
        // rows a k_test_required block walks: enough of them for MP_BLOCK_TESTS bit tests, more
        // once tiles x rows would pass MP_GRID_TARGET blocks, MP_ROWS at most
        const int64_t per_tile = std::min<int64_t>(req_n, MP_TILE);
        int64_t rows_blk = std::max((MP_BLOCK_TESTS + per_tile - 1) / per_tile,
                                    (req_tiles * nb + MP_GRID_TARGET - 1) / MP_GRID_TARGET);
        rows_blk = std::max<int64_t>(1, std::min<int64_t>(rows_blk, MP_ROWS));
        const int64_t chunks = (nb + rows_blk - 1) / rows_blk;
        if (chunks > 65535) return CA_ECAPACITY;
        CA_HIP_CHECK(hipMemsetAsync(sc.d_rows.ptr, 0, (size_t)nb * row_bytes, st));
        hipLaunchKernelGGL(k_mark_lists, dim3((uint32_t)(tpre[r1] - tpre[r0])), dim3(MP_THREADS), 0, st, v.d_sched_pod,
                           v.total, d_roff, d_roff + R, d_roff + 2 * (size_t)R, r0, r1, sc.d_rows.as<uint32_t>(), W,
                           n_pods, d_bad);
        CA_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_test_required, dim3((uint32_t)req_tiles, (uint32_t)chunks), dim3(MP_THREADS), 0, st,
                           req_ids, req_total, req_a, req_n, sc.d_rows.as<uint32_t>(), W, nb, (int32_t)rows_blk,
                           n_pods, d_nmiss + r0, d_first + r0, d_bad);
        CA_HIP_CHECK(hipGetLastError());
    }
    CA_HIP_CHECK(hipEventRecord(sc.ev1, st));
    CA_HIP_CHECK(hipMemcpyAsync(h_out, sc.d_out.ptr, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    CA_HIP_CHECK(hipStreamSynchronize(st));
    sc.timed = true;
    if (h_out[R] != 0) {
        set_last_error("missing pods: a scheduled pod id outside the pod set");
        return CA_EDEVICE;
    }
    for (int32_t k = 0; k < n_groups; k++) {
        const int32_t g = groups[k];
        if (req_n == 0 || g == required_group || v.h_nsched[g] == 0) continue;
        const int32_t r = sc.row_of[g];
        n_missing[k] = h_out[r];
        if (first_missing) first_missing[k] = h_out[R + 1 + r] == INT32_MAX ? -1 : h_out[R + 1 + r];
    }
    return CA_OK;
}

int estimate_plan_export_list(const ca_estimate_plan* p, int32_t group, int32_t* h_ids, int32_t n) {
    if (!p) return CA_EINVAL;
    PlanLists v;
    estimate_plan_lists(p, &v);
    if (group < 0 || group >= v.G || n < 0 || (n > 0 && !h_ids)) return CA_EINVAL;
    if (!v.final_lists) return CA_ESTATE;
    if (n > v.h_nsched[group] || n > v.h_off[group + 1] - v.h_off[group]) return CA_EINVAL;
    if (n == 0) return CA_OK;
    CA_HIP_CHECK(hipSetDevice(v.m->device));
    CA_HIP_CHECK(hipMemcpyAsync(h_ids, v.d_sched_pod + v.h_off[group], sizeof(int32_t) * (size_t)n,
                                hipMemcpyDeviceToHost, v.m->stream));
    CA_HIP_CHECK(hipStreamSynchronize(v.m->stream));
    return CA_OK;
}

int estimate_plan_missing_pods_of(ca_estimate_plan* p, const int32_t* h_ids, int32_t n, const int32_t* groups,
                                  int32_t n_groups, int32_t* n_missing, int32_t* first_missing) {
    if (!p || n < 0 || (n > 0 && !h_ids)) return CA_EINVAL;
    PlanLists v;
    estimate_plan_lists(p, &v);
    MissingPodsScratch& sc = *v.missing;
    RequiredList req;
    if (n > 0) {
        // the upload is ordered before the core's kernels by the plan's stream
        CA_HIP_CHECK(hipSetDevice(v.m->device));
        int rc;
        if ((rc = sc.d_req.reserve(sizeof(int32_t) * (size_t)n)) != CA_OK) return rc;
        CA_HIP_CHECK(hipMemcpyAsync(sc.d_req.ptr, h_ids, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice,
                                    v.m->stream));
        req.d_ids = sc.d_req.as<int32_t>();
    }
    req.total = req.n = n;
    const int rc = estimate_plan_missing_pods(p, &req, -1, groups, n_groups, n_missing, first_missing);
    // (a core that returned without a launch has not waited for the upload: h_ids is the caller's again)
    if (n > 0) CA_HIP_CHECK(hipStreamSynchronize(v.m->stream));
    return rc;
}

}  // namespace casim

using namespace casim;

extern "C" {

int ca_estimate_plan_groups_missing_pods(ca_estimate_plan* p, int32_t required_group, const int32_t* groups,
                                         int32_t n_groups, int32_t* n_missing, int32_t* first_missing) {
    return estimate_plan_missing_pods(p, nullptr, required_group, groups, n_groups, n_missing, first_missing);
}

int ca_estimate_plan_groups_missing_pods_ms(const ca_estimate_plan* p, float* kernel_ms) {
    if (!p || !kernel_ms) return CA_EINVAL;
    PlanLists v;
    estimate_plan_lists(p, &v);
    *kernel_ms = 0;
    if (v.missing->timed) CA_HIP_CHECK(hipEventElapsedTime(kernel_ms, v.missing->ev0, v.missing->ev1));
    return CA_OK;
}

}  // extern "C"
