// expander.hip — the step after Estimate in ScaleUp: ExpanderStrategy.BestOption
// (CA/core/scaleup/orchestrator/orchestrator.go:195) for the least-waste and most-pods
// filters, on the Estimate plan's device-resident pod lists.
//
//   ca_estimate_plan_option_sums   resourcesForPods (CA/expander/waste/waste.go:74-87) of every
//                                  option: k_option_sums over the resident lists
//   ca_estimate_plan_option_price_sums   totalPodPrice (CA/expander/price/price.go:126-134) of
//                                  every option: k_option_price_sums, the in-order float64 sum
//   ca_estimate_plan_fetch_group   one option's pod list (the one the expander picked)
//   ca_expander_best_options       Filter.BestOptions of waste.go:36-72 and
//                                  mostpods.go:33-53, host code, the Go loops restated
//
// resourcesForPods sums the containers' cpu / memory requests of an option's pods: per pod
// that is ca_pod_spec.score_milli_cpu / score_memory, which the podset keeps per score class
// (d_cls[pod], d_cls_sc[class] = {cpu, memory}).  The sums are wrapping int64 adds, so block
// order cannot change them.
#include "mirror.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace casim {
namespace {

// A block sums one tile of OS_TILE list positions of one group.  Tiles are cut at multiples
// of 4 ids from the list buffer's base, so every lane loads aligned 16-byte quads whatever
// the group's offset: the first tile of a group starts at its offset rounded down, and the
// positions before the offset (the previous group's) and past n_scheduled (stale ids of an
// earlier run, or -1) are masked.
constexpr int OS_THREADS = 256;
constexpr int OS_QUADS = 2;                                // 16-byte loads per lane
constexpr int OS_TILE = OS_THREADS * OS_QUADS * 4;         // 2048 ids, 8 KB
constexpr int OS_CLS_LDS = 2048;                           // score classes counted in LDS (8 KB)

__device__ inline int64_t wave_sum(int64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)(uint64_t)v, o, 64);
        const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)((uint64_t)v >> 32), o, 64);
        v = (int64_t)((uint64_t)v + (((uint64_t)hi << 32) | lo));
    }
    return v;
}

// goff / gns / tpre: the groups' offsets, n_scheduled and the exclusive prefix of their tile
// counts (tpre[G] = gridDim.x).  sums: G x {cpu, memory}, then one counter of ids outside the
// podset (none in a final list; they are skipped and the call fails).
// COUNT: n_cls <= OS_CLS_LDS — the tile's classes are counted with LDS atomics and each
// class's count x {cpu, memory} is formed once; else each id gathers its class's pair.
template <bool COUNT>
__global__ void __launch_bounds__(OS_THREADS) k_option_sums(const int32_t* __restrict__ sched_pod, int32_t total,
                                                           const int32_t* __restrict__ goff,
                                                           const int32_t* __restrict__ gns,
                                                           const int32_t* __restrict__ tpre, int32_t G,
                                                           const int32_t* __restrict__ cls,
                                                           const int64_t* __restrict__ cls_sc, int32_t n_cls,
                                                           int32_t n_pods, unsigned long long* __restrict__ sums) {
    __shared__ uint32_t cnt[COUNT ? OS_CLS_LDS : 1];
    __shared__ int64_t red[2][OS_THREADS / 64];
    __shared__ uint32_t bad_ids;
    __shared__ int32_t found[4];                  // the tile's group, its offset, n_scheduled, first tile
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t b = (int32_t)blockIdx.x;
    // The group of this tile: the one g with tpre[g] <= b < tpre[g + 1] (groups without tiles
    // have an empty range).  Binary steps narrow [lo, hi) to one candidate per lane, then
    // every lane tests its own with loads that do not depend on one another: with up to 256
    // groups the search is one round trip to memory, not a chain of them.
    int32_t lo = 0, hi = G;
    while (hi - lo > OS_THREADS) {
        const int32_t mid = (lo + hi) >> 1;
        if (tpre[mid] <= b) lo = mid; else hi = mid;
    }
    if (lo + tid < hi) {
        const int32_t i = lo + tid;
        const int32_t t0 = tpre[i], t1 = tpre[i + 1], go = goff[i], gn = gns[i];
        if (t0 <= b && b < t1) { found[0] = i; found[1] = go; found[2] = gn; found[3] = t0; }
    }
    // (the first classes' sums are requested now, for the end of the tile)
    longlong2 sc_first = make_longlong2(0, 0);
    if (COUNT && tid < n_cls) sc_first = *reinterpret_cast<const longlong2*>(cls_sc + 2 * (size_t)tid);
    if (COUNT)
        for (int32_t c = tid; c < n_cls; c += OS_THREADS) cnt[c] = 0;
    if (tid == 0) bad_ids = 0;
    __syncthreads();
    const int32_t g = found[0];
    const int32_t a = found[1], e = a + found[2];
    const int64_t base = (int64_t)(a & ~3) + (int64_t)(b - found[3]) * OS_TILE;   // (may pass 2^31 in the last tile)
    // (every tile has its group; a prefix that does not say so must not become an address)
    if ((uint32_t)g >= (uint32_t)G || a < 0 || e < a || e > total) return;
    uint64_t cpu = 0, mem = 0;
    uint32_t bad = 0;
#pragma unroll
    for (int q = 0; q < OS_QUADS; q++) {
        const int64_t i = base + (q * OS_THREADS + tid) * 4;
        if (i >= e) continue;
        int32_t id[4];
        if (i + 4 <= total) {
            const int4 v = *reinterpret_cast<const int4*>(sched_pod + i);
            id[0] = v.x; id[1] = v.y; id[2] = v.z; id[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) id[j] = i + j < total ? sched_pod[i + j] : -1;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (i + j < a || i + j >= e) continue;
            if ((uint32_t)id[j] >= (uint32_t)n_pods) { bad++; continue; }
            const int32_t c = cls[id[j]];
            if ((uint32_t)c >= (uint32_t)n_cls) { bad++; continue; }
            if (COUNT) {
                atomicAdd(&cnt[c], 1u);
            } else {
                const longlong2 sc = *reinterpret_cast<const longlong2*>(cls_sc + 2 * (size_t)c);
                cpu += (uint64_t)sc.x;
                mem += (uint64_t)sc.y;
            }
        }
    }
    if (COUNT) {
        __syncthreads();
        for (int32_t c = tid; c < n_cls; c += OS_THREADS) {
            const uint64_t n = cnt[c];
            if (n == 0) continue;
            const longlong2 sc = c == tid ? sc_first : *reinterpret_cast<const longlong2*>(cls_sc + 2 * (size_t)c);
            cpu += n * (uint64_t)sc.x;
            mem += n * (uint64_t)sc.y;
        }
    }
    if (bad) atomicAdd(&bad_ids, bad);
    const int64_t wc = wave_sum((int64_t)cpu), wm = wave_sum((int64_t)mem);
    if ((tid & 63) == 0) { red[0][tid >> 6] = wc; red[1][tid >> 6] = wm; }
    __syncthreads();
    if (tid == 0) {
        uint64_t c = 0, m = 0;
        for (int w = 0; w < OS_THREADS / 64; w++) { c += (uint64_t)red[0][w]; m += (uint64_t)red[1][w]; }
        atomicAdd(&sums[2 * (size_t)g], (unsigned long long)c);
        atomicAdd(&sums[2 * (size_t)g + 1], (unsigned long long)m);
        if (bad_ids) atomicAdd(&sums[2 * (size_t)G], (unsigned long long)bad_ids);
    }
}

// ---- price expander: totalPodPrice of every option (CA/expander/price/price.go:126-134) ----
// The sum is float64 and the reference adds left to right, so an option's total is one serial
// chain of IEEE adds: no option is split, and nothing is reduced across lanes.  One wave per
// option.  Its 64 lanes cooperate on the loads only: a chunk of PS_CHUNK consecutive list
// positions is loaded as one aligned quad per lane (cut from the buffer's base, as above),
// the four 8-byte prices of each lane are gathered, and the chunk goes through the wave's LDS
// row, from which every lane reads the same address (a broadcast) and adds: the accumulator
// is uniform over the wave.  The next chunk's prices and the ids of the chunk after it are in
// flight while the current chunk is added.
//
// A position that does not count (before the group's offset, from n_scheduled on, or an id
// outside the pod set) is handed over as -0.0: x + -0.0 == x bit for bit for every x, +0.0,
// the subnormals and NaN included, and the chain starts at +0.0, so such a position is
// dropped without a branch on the chain.
constexpr int PS_WAVES = 4;                        // options per block
constexpr int PS_THREADS = PS_WAVES * 64;
constexpr int PS_CHUNK = 64 * 4;                   // list positions per wave and chunk (2 KB of prices)
constexpr int PS_STEP = 16;                        // prices read from the row ahead of the chain
constexpr int PS_WAIT_LDS = 0xC07F;                // s_waitcnt lgkmcnt(0), the other counters left alone
static_assert(PS_CHUNK % PS_STEP == 0 && PS_STEP / 2 <= 15, "whole steps; the wait's count is 4 bits");

// Four ids at any 4-byte boundary (the shifted quad below is not 16-byte aligned).
struct __attribute__((aligned(4))) PsIds { int32_t x, y, z, w; };
// The ids of one lane's quad as loaded, and how far the load was shifted (below).
struct PsQuad { PsIds v; int32_t d; };

// The ids of chunk c: one 16-byte load per lane and no branch (the two results of a branch would
// be merged in registers, and that waits for the load, which is to stay in flight over the
// chain).  The quad at i, or, where that would pass the buffer's end, the buffer's last quad:
// ps_gather undoes the shift.  total >= 4 (the host sums a shorter buffer).
__device__ inline PsQuad ps_load_ids(const int32_t* __restrict__ sched_pod, int32_t total, int64_t base, int32_t c,
                                     int32_t lane) {
    const int64_t i = base + (int64_t)c * PS_CHUNK + lane * 4;
    const int64_t last = (int64_t)total - 4;
    const int64_t at = i < last ? i : last;
    PsQuad q;
    q.v = *reinterpret_cast<const PsIds*>(sched_pod + at);
    q.d = (int32_t)(i - at < 4 ? i - at : 4);
    return q;
}

// The prices of one lane's quad as loaded, and which of them count (bit j: position j).
struct PsPrices { double v[4]; uint32_t ok; };

// The prices of chunk c's quad q of the list [a, e), e <= total.  Position i + j of the buffer is
// q.v[j + q.d], in the quad for every i + j < total.  Branch-free like ps_load_ids, and for the
// same reason: the four ids are settled first, then the four loads are issued back to back (a
// position that does not count reads price[0]; the buffer holds at least one value), and
// ps_counted puts -0.0 in its place once the loads have landed.
__device__ inline PsPrices ps_gather(const PsQuad& q, const double* __restrict__ price, int32_t n_pods, int64_t base,
                                     int32_t a, int32_t e, int32_t c, int32_t lane, uint32_t* bad) {
    PsPrices p;
    const int64_t i = base + (int64_t)c * PS_CHUNK + lane * 4;
    const int32_t w[8] = {q.v.x, q.v.y, q.v.z, q.v.w, -1, -1, -1, -1};
    int32_t id[4];
    p.ok = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        id[j] = w[j];
#pragma unroll
        for (int d = 1; d <= 4; d++) id[j] = q.d == d ? w[j + d] : id[j];
        const bool counted = i + j >= a && i + j < e;
        const bool known = (uint32_t)id[j] < (uint32_t)n_pods;
        *bad += counted && !known ? 1u : 0u;
        p.ok |= counted && known ? 1u << j : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) p.v[j] = price[p.ok >> j & 1 ? id[j] : 0];
    return p;
}

// x + -0.0 == x for every x: what a position that does not count hands to the chain
__device__ inline double ps_counted(const PsPrices& p, int j) { return p.ok >> j & 1 ? p.v[j] : -0.0; }

// goff / gns: the groups' offsets and n_scheduled; order: the groups by falling n_scheduled (the
// longest chains start first).  out: G totals, then one counter of ids outside the pod set.
__global__ void __launch_bounds__(PS_THREADS) k_option_price_sums(const int32_t* __restrict__ sched_pod, int32_t total,
                                                                 const int32_t* __restrict__ goff,
                                                                 const int32_t* __restrict__ gns,
                                                                 const int32_t* __restrict__ order, int32_t G,
                                                                 const double* __restrict__ price, int32_t n_pods,
                                                                 double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double row[PS_WAVES][PS_CHUNK];
    const int32_t lane = (int32_t)threadIdx.x & 63, w = (int32_t)threadIdx.x >> 6;
    const int32_t slot = (int32_t)blockIdx.x * PS_WAVES + w;
    if (slot >= G) return;
    // (one option per wave: its group, offset and length are the same in every lane; saying so
    // keeps the loop bounds in scalar registers)
    const int32_t g = __builtin_amdgcn_readfirstlane(order[slot]);
    if ((uint32_t)g >= (uint32_t)G) return;
    unsigned long long* bad_ids = reinterpret_cast<unsigned long long*>(out + G);
    const int32_t a = __builtin_amdgcn_readfirstlane(goff[g]), n = __builtin_amdgcn_readfirstlane(gns[g]);
    // (a list that does not lie in the buffer must not become an address)
    if (a < 0 || n < 0 || (int64_t)a + n > total || total < 4) {
        if (lane == 0) atomicAdd(bad_ids, 1ull);
        return;
    }
    const int32_t e = a + n;
    const int64_t base = a & ~3;
    const int32_t chunks = n > 0 ? (int32_t)((e - base + PS_CHUNK - 1) / PS_CHUNK) : 0;
    double* my = row[w];
    double acc = 0.0;
    uint32_t bad = 0;
    PsQuad ids = ps_load_ids(sched_pod, total, base, 0, lane);
    PsPrices cur = ps_gather(ids, price, n_pods, base, a, e, 0, lane, &bad);
    ids = ps_load_ids(sched_pod, total, base, 1, lane);
    for (int32_t c = 0; c < chunks; c++) {
        // (the wave's earlier reads of the row are done: a wave's LDS operations stay in order)
        *reinterpret_cast<double2*>(my + lane * 4) = make_double2(ps_counted(cur, 0), ps_counted(cur, 1));
        *reinterpret_cast<double2*>(my + lane * 4 + 2) = make_double2(ps_counted(cur, 2), ps_counted(cur, 3));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the next chunk's prices and the ids after them: in flight during the chain below
        const PsPrices nxt = ps_gather(ids, price, n_pods, base, a, e, c + 1, lane, &bad);
        ids = ps_load_ids(sched_pod, total, base, c + 2, lane);
        // The chain: the whole row in steps of PS_STEP (every lane wrote its four values, so
        // what is added beside the counted positions is -0.0: up to 3 positions before the
        // offset in chunk 0, and the rest of the last chunk).  Every lane reads the same address.
        // The steps are unrolled without a branch: the next step's values are requested before
        // this step's are added, into the other half of buf, and one counted wait per step (for
        // all but the PS_STEP / 2 reads just issued) stands in for a wait per read.
        double2 buf[2][PS_STEP / 2];
#pragma unroll
        for (int j = 0; j < PS_STEP / 2; j++) buf[0][j] = *reinterpret_cast<const double2*>(my + 2 * j);
#pragma unroll
        for (int s = 0; s < PS_CHUNK / PS_STEP; s++) {
            if (s + 1 < PS_CHUNK / PS_STEP) {
#pragma unroll
                for (int j = 0; j < PS_STEP / 2; j++)
                    buf[(s + 1) & 1][j] = *reinterpret_cast<const double2*>(my + (s + 1) * PS_STEP + 2 * j);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (s + 1 < PS_CHUNK / PS_STEP) __builtin_amdgcn_s_waitcnt(PS_WAIT_LDS | ((PS_STEP / 2) << 8));
            else __builtin_amdgcn_s_waitcnt(PS_WAIT_LDS);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < PS_STEP / 2; j++) {
                acc += buf[s & 1][j].x;
                acc += buf[s & 1][j].y;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        cur = nxt;
    }
    if (bad) atomicAdd(bad_ids, (unsigned long long)bad);
    if (lane == 0) out[g] = acc;
}

}  // namespace
}  // namespace casim

using namespace casim;

extern "C" {

int ca_estimate_plan_option_sums(ca_estimate_plan* p, int64_t* req_milli_cpu, int64_t* req_memory) {
    if (!p) return CA_EINVAL;
    PlanLists v;
    estimate_plan_lists(p, &v);
    if (v.G > 0 && (!req_milli_cpu || !req_memory)) return CA_EINVAL;
    if (!v.final_lists) return CA_ESTATE;
    OptionSumsScratch& sc = *v.scratch;
    sc.timed = false;
    const int32_t G = v.G;
    if (G == 0) return CA_OK;
    CA_HIP_CHECK(hipSetDevice(v.m->device));
    hipStream_t st = v.m->stream;
    const size_t n_in = 3 * (size_t)G + 1, n_sums = 2 * (size_t)G + 1;
    const size_t sums_at = (n_in * sizeof(int32_t) + 15) & ~(size_t)15;
    int rc;
    if ((rc = sc.h.reserve(sums_at + n_sums * sizeof(int64_t))) != CA_OK) return rc;
    if ((rc = sc.d_in.reserve(n_in * sizeof(int32_t))) != CA_OK) return rc;
    if ((rc = sc.d_sums.reserve(n_sums * sizeof(int64_t))) != CA_OK) return rc;
    int32_t* off = sc.h.as<int32_t>();
    int32_t* ns = off + G;
    int32_t* tpre = ns + G;
    int64_t tiles = 0;
    for (int32_t g = 0; g < G; g++) {
        const int32_t a = v.h_off[g], n = v.h_nsched[g];
        if (n < 0 || n > v.h_off[g + 1] - a) { set_last_error("option sums: n_scheduled outside its group"); return CA_EDEVICE; }
        off[g] = a;
        ns[g] = n;
        tpre[g] = (int32_t)tiles;
        if (n > 0) tiles += ((int64_t)(a + n) - (a & ~3) + OS_TILE - 1) / OS_TILE;
    }
    tpre[G] = (int32_t)tiles;
    int64_t* h_sums = reinterpret_cast<int64_t*>(static_cast<char*>(sc.h.ptr) + sums_at);
    if (tiles == 0) {
        std::memset(h_sums, 0, n_sums * sizeof(int64_t));
    } else {
        if (!sc.ev0) {
            CA_HIP_CHECK(hipEventCreate(&sc.ev0));
            CA_HIP_CHECK(hipEventCreate(&sc.ev1));
        }
        CA_HIP_CHECK(hipMemcpyAsync(sc.d_in.ptr, off, n_in * sizeof(int32_t), hipMemcpyHostToDevice, st));
        CA_HIP_CHECK(hipMemsetAsync(sc.d_sums.ptr, 0, n_sums * sizeof(int64_t), st));
        const int32_t* d_off = sc.d_in.as<int32_t>();
        const bool count = v.s->n_cls <= OS_CLS_LDS;
        CA_HIP_CHECK(hipEventRecord(sc.ev0, st));
        hipLaunchKernelGGL(count ? k_option_sums<true> : k_option_sums<false>, dim3((uint32_t)tiles), dim3(OS_THREADS), 0,
                           st, v.d_sched_pod, v.total, d_off, d_off + G, d_off + 2 * (size_t)G, G,
                           v.s->d_cls.as<int32_t>(), v.s->d_cls_sc.as<int64_t>(), v.s->n_cls, v.s->n_host,
                           sc.d_sums.as<unsigned long long>());
        CA_HIP_CHECK(hipGetLastError());
        CA_HIP_CHECK(hipEventRecord(sc.ev1, st));
        CA_HIP_CHECK(hipMemcpyAsync(h_sums, sc.d_sums.ptr, n_sums * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        CA_HIP_CHECK(hipStreamSynchronize(st));
        sc.timed = true;
        if (h_sums[2 * (size_t)G] != 0) {
            set_last_error("option sums: a scheduled pod id outside the pod set");
            return CA_EDEVICE;
        }
    }
    for (int32_t g = 0; g < G; g++) {
        req_milli_cpu[g] = h_sums[2 * (size_t)g];
        req_memory[g] = h_sums[2 * (size_t)g + 1];
    }
    return CA_OK;
}

int ca_estimate_plan_option_sums_ms(const ca_estimate_plan* p, float* kernel_ms) {
    if (!p || !kernel_ms) return CA_EINVAL;
    PlanLists v;
    estimate_plan_lists(p, &v);
    *kernel_ms = 0;
    if (v.scratch->timed) CA_HIP_CHECK(hipEventElapsedTime(kernel_ms, v.scratch->ev0, v.scratch->ev1));
    return CA_OK;
}

int ca_estimate_plan_option_price_sums(ca_estimate_plan* p, const double* pod_price, int32_t n_prices,
                                       double* total_pod_price) {
    if (!p) return CA_EINVAL;
    PlanLists v;
    estimate_plan_lists(p, &v);
    if (n_prices != v.s->n_host || (n_prices > 0 && !pod_price)) return CA_EINVAL;
    if (v.G > 0 && !total_pod_price) return CA_EINVAL;
    if (!v.final_lists) return CA_ESTATE;
    PriceSumsScratch& sc = *v.price;
    sc.timed = false;
    const int32_t G = v.G;
    if (G == 0) return CA_OK;
    CA_HIP_CHECK(hipSetDevice(v.m->device));
    hipStream_t st = v.m->stream;
    // staging: [off | n_scheduled | order] int32, the prices, the totals and the counter
    const size_t n_in = 3 * (size_t)G, n_out = (size_t)G + 1;
    const size_t price_at = (n_in * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t out_at = price_at + (size_t)n_prices * sizeof(double);
    int rc;
    if ((rc = sc.h.reserve(out_at + n_out * sizeof(double))) != CA_OK) return rc;
    if ((rc = sc.d_in.reserve(n_in * sizeof(int32_t))) != CA_OK) return rc;
    if ((rc = sc.d_price.reserve(std::max<size_t>((size_t)n_prices, 1) * sizeof(double))) != CA_OK) return rc;
    if ((rc = sc.d_out.reserve(n_out * sizeof(double))) != CA_OK) return rc;
    int32_t* off = sc.h.as<int32_t>();
    int32_t* ns = off + G;
    int32_t* order = ns + G;
    for (int32_t g = 0; g < G; g++) {
        const int32_t a = v.h_off[g], n = v.h_nsched[g];
        if (a < 0 || n < 0 || n > v.h_off[g + 1] - a || (int64_t)a + n > v.total) {
            set_last_error("option price sums: n_scheduled outside its group");
            return CA_EDEVICE;
        }
        off[g] = a;
        ns[g] = n;
        order[g] = g;
    }
    if (v.total < 4) {          // less than one quad of list positions: summed here, in the same order
        int32_t ids[4] = {0, 0, 0, 0};
        if (v.total > 0)
            CA_HIP_CHECK(hipMemcpy(ids, v.d_sched_pod, sizeof(int32_t) * (size_t)v.total, hipMemcpyDeviceToHost));
        for (int32_t g = 0; g < G; g++) {
            double t = 0.0;
            for (int32_t k = 0; k < ns[g]; k++) {
                const int32_t id = ids[off[g] + k];
                if ((uint32_t)id >= (uint32_t)n_prices) {
                    set_last_error("option price sums: a scheduled pod id outside the pod set");
                    return CA_EDEVICE;
                }
                t += pod_price[id];
            }
            total_pod_price[g] = t;
        }
        return CA_OK;
    }
    // the longest chains first; equal lengths keep their group order
    std::stable_sort(order, order + G, [ns](int32_t x, int32_t y) { return ns[x] > ns[y]; });
    double* h_price = reinterpret_cast<double*>(static_cast<char*>(sc.h.ptr) + price_at);
    double* h_out = reinterpret_cast<double*>(static_cast<char*>(sc.h.ptr) + out_at);
    if (n_prices > 0) std::memcpy(h_price, pod_price, (size_t)n_prices * sizeof(double));
    if (!sc.ev0) {
        CA_HIP_CHECK(hipEventCreate(&sc.ev0));
        CA_HIP_CHECK(hipEventCreate(&sc.ev1));
    }
    CA_HIP_CHECK(hipMemcpyAsync(sc.d_in.ptr, off, n_in * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (n_prices > 0)
        CA_HIP_CHECK(hipMemcpyAsync(sc.d_price.ptr, h_price, (size_t)n_prices * sizeof(double), hipMemcpyHostToDevice,
                                    st));
    CA_HIP_CHECK(hipMemsetAsync(sc.d_out.ptr, 0, n_out * sizeof(double), st));
    const int32_t* d_off = sc.d_in.as<int32_t>();
    CA_HIP_CHECK(hipEventRecord(sc.ev0, st));
    hipLaunchKernelGGL(k_option_price_sums, dim3((uint32_t)((G + PS_WAVES - 1) / PS_WAVES)), dim3(PS_THREADS), 0, st,
                       v.d_sched_pod, v.total, d_off, d_off + G, d_off + 2 * (size_t)G, G, sc.d_price.as<double>(),
                       n_prices, sc.d_out.as<double>());
    CA_HIP_CHECK(hipGetLastError());
    CA_HIP_CHECK(hipEventRecord(sc.ev1, st));
    CA_HIP_CHECK(hipMemcpyAsync(h_out, sc.d_out.ptr, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    CA_HIP_CHECK(hipStreamSynchronize(st));
    sc.timed = true;
    uint64_t bad;
    std::memcpy(&bad, h_out + G, sizeof(bad));
    if (bad != 0) {
        set_last_error("option price sums: a scheduled pod id outside the pod set");
        return CA_EDEVICE;
    }
    std::memcpy(total_pod_price, h_out, (size_t)G * sizeof(double));
    return CA_OK;
}

int ca_estimate_plan_option_price_sums_ms(const ca_estimate_plan* p, float* kernel_ms) {
    if (!p || !kernel_ms) return CA_EINVAL;
    PlanLists v;
    estimate_plan_lists(p, &v);
    *kernel_ms = 0;
    if (v.price->timed) CA_HIP_CHECK(hipEventElapsedTime(kernel_ms, v.price->ev0, v.price->ev1));
    return CA_OK;
}

int ca_estimate_plan_fetch_group(const ca_estimate_plan* p, int32_t group, int32_t* sched_pod, int32_t cap,
                                 int32_t* n) {
    if (!p || !n || cap < 0 || (cap > 0 && !sched_pod)) return CA_EINVAL;
    PlanLists v;
    estimate_plan_lists(p, &v);
    if (group < 0 || group >= v.G) return CA_EINVAL;
    if (!v.final_lists) return CA_ESTATE;
    const int32_t ns = v.h_nsched[group];
    *n = ns;
    if (ns > cap) return CA_ECAPACITY;
    if (ns > 0) {
        CA_HIP_CHECK(hipSetDevice(v.m->device));
        CA_HIP_CHECK(hipMemcpy(sched_pod, v.d_sched_pod + v.h_off[group], sizeof(int32_t) * (size_t)ns,
                               hipMemcpyDeviceToHost));
    }
    return CA_OK;
}

// Filter.BestOptions.  Go's int64 arithmetic wraps; its float64 conversions, divisions and the
// one addition are IEEE (this unit is built with -ffp-contract=off), so the scores are Go's bit
// for bit, NaN (0 / 0 at node_count 0) and the infinities included.
int ca_expander_best_options(int32_t filter, const ca_estimate_result* results, const int64_t* req_milli_cpu,
                             const int64_t* req_memory, const int64_t* cap_milli_cpu, const int64_t* cap_memory,
                             const int32_t* options, int32_t n_options, int32_t* best, int32_t* n_best,
                             double* scores) {
    if (n_options < 0 || !n_best || (n_options > 0 && (!results || !options || !best))) return CA_EINVAL;
    if (filter != CA_EXPANDER_MOST_PODS && filter != CA_EXPANDER_LEAST_WASTE) return CA_EINVAL;
    if (filter == CA_EXPANDER_LEAST_WASTE && n_options > 0 &&
        (!req_milli_cpu || !req_memory || !cap_milli_cpu || !cap_memory))
        return CA_EINVAL;
    for (int32_t k = 0; k < n_options; k++) if (options[k] < 0) return CA_EINVAL;
    int32_t nb = 0;
    bool have = false;                       // leastWastedOptions / maxOptions != nil
    if (filter == CA_EXPANDER_MOST_PODS) {   // mostpods.go:33-53
        int64_t max_pods = 0;
        for (int32_t k = 0; k < n_options; k++) {
            const int64_t np = results[options[k]].n_scheduled;
            if (scores) scores[k] = (double)np;
            if (np == max_pods) best[nb++] = k, have = true;
            if (np > max_pods) {
                max_pods = np;
                nb = 0;
                best[nb++] = k;
                have = true;
            }
        }
    } else {                                 // waste.go:36-72
        double least = 0;
        for (int32_t k = 0; k < n_options; k++) {
            const int32_t o = options[k];
            const int64_t nodes = results[o].node_count;
            const int64_t avail_cpu = (int64_t)((uint64_t)cap_milli_cpu[o] * (uint64_t)nodes);
            const int64_t avail_mem = (int64_t)((uint64_t)cap_memory[o] * (uint64_t)nodes);
            const double wasted_cpu = (double)wsub(avail_cpu, req_milli_cpu[o]) / (double)avail_cpu;
            const double wasted_mem = (double)wsub(avail_mem, req_memory[o]) / (double)avail_mem;
            const double score = wasted_cpu + wasted_mem;
            if (scores) scores[k] = score;
            if (score == least) best[nb++] = k, have = true;
            if (!have || score < least) {
                least = score;
                nb = 0;
                best[nb++] = k;
                have = true;
            }
        }
    }
    // best[] holds positions in options[] so far (a position is never below its slot)
    for (int32_t i = 0; i < nb; i++) best[i] = options[best[i]];
    *n_best = nb;
    return CA_OK;
}

}  // extern "C"
