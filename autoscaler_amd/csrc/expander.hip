// expander.hip — the step after Estimate in ScaleUp: ExpanderStrategy.BestOption
// (CA/core/scaleup/orchestrator/orchestrator.go:195) for the least-waste and most-pods
// filters, on the Estimate plan's device-resident pod lists.
//
//   ca_estimate_plan_option_sums   resourcesForPods (CA/expander/waste/waste.go:74-87) of every
//                                  option: k_option_sums over the resident lists
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
