// mirror.h — the ClusterSnapshot mirror: host journal + device SoA rows.
//
// Host side keeps the authoritative rows (so Fork/Revert/Commit are O(changes),
// DeltaClusterSnapshot semantics, CA/simulator/clustersnapshot/delta.go:43-475);
// device rows are re-synchronised lazily (dirty rows only) before a kernel reads them.
#pragma once
#include "casim_internal.h"
#include "podcols_host.h"
#include <array>
#include <memory>
#include <deque>
#include <cstdlib>
#include <new>
#include <sys/mman.h>

namespace casim {

enum { J_FORK = 1, J_ADD_NODE, J_ADD_POD, J_REMOVE_POD, J_REMOVE_NODE };

struct JournalEntry {
    int32_t kind, node, pod, slot;
    uint64_t ports[CA_PORT_WORDS];
};

struct NodeRow {
    ca_node_spec spec;
    int64_t req_cpu = 0, req_mem = 0, req_eph = 0;
    int64_t req_scalar[CA_MAX_SCALAR] = {0};
    int64_t npods = 0;
    uint64_t ports[CA_PORT_WORDS] = {0};
    std::vector<int32_t> pods;   // NodeInfo.Pods order
};

struct PodRow {
    ca_pod_spec spec;            // selector indices re-based on the mirror tables
    int32_t node = -1;
};

struct ca_mirror_impl;

// Device pod table: hot rows + full records + selector tables.
struct DevPodTable {
    DevBuf hot, spec, terms, reqs, names;
    int32_t n_pods = 0, n_terms = 0, n_reqs = 0, n_names = 0;
    int upload(const ca_pod_spec* pods, int32_t n, const ca_selector_term* terms, int32_t nt,
               const ca_selector_req* reqs, int32_t nr, const int32_t* names, int32_t nn, hipStream_t st);
    // the same with the hot rows and records copied into the page-locked `stage` first (host
    // threads) and the copies left queued on st: the caller syncs st before stage is reused
    int upload_staged(const ca_pod_spec* pods, int32_t n, const ca_selector_term* terms, int32_t nt,
                      const ca_selector_req* reqs, int32_t nr, const int32_t* names, int32_t nn, HostBuf& stage,
                      hipStream_t st);
    // append pods [n_pods, n_pods + k) and the selector tables' new tails (the mirror's
    // tables only grow between Clear()s), keeping what is on the device
    int append(const ca_pod_spec* new_pods, int32_t k, const ca_selector_term* terms, int32_t nt,
               const ca_selector_req* reqs, int32_t nr, const int32_t* names, int32_t nn, hipStream_t st);
    // append src's records idx[0..k) (already on the device: a podset), in order; the
    // records must hold no selector-table or PreFilter-name references
    int append_gather(const DevPodTable& src, const int32_t* idx, int32_t k, DevBuf& d_idx, hipStream_t st);
};

// Per-mirror scratch of ca_find_nodes_to_remove, kept across calls (no per-call
// hipMalloc); host staging is page-locked.
struct SweepScratch {
    DevBuf in, lin, need, out, todo, tab, wl;
    DevBuf tev, tdest;              // table lanes' evaluation counts and pod destinations (first round)
    DevBuf tfp, vp, mode;           // table rows' fit-point classes; visible-node prefix counts; class mode
    DevBuf bsum;                    // per 64-node block: maxima of the visible rows (sweep.hip BlockSum)
    DevBuf chainl;                  // the host walk's serial exact chain: candidates in order
    DevBuf bmap;                    // a multi-device range's block map (k_walk_map)
    HostBuf h_in, h_tab, h_out, h_todo, h_lin, h_wl, h_tfp, h_l0, h_chainl, h_bmap;
    // the host walk's table rounds: each round's compact rows (main and side rows), read in
    // place by the walk for the rest of the call; pooled across calls
    std::deque<HostBuf> rbuf;
    // device mappings of h_todo and the round buffers (cleared whenever one of them moves)
    std::vector<std::pair<void*, void*>> dmap;
    // the device pipeline of the last call shape, replayed as a graph (sweep.hip sweep_core)
    hipGraphExec_t gexec = nullptr;
    uint64_t gkey = 0, gseen = 0;
    // serial-only calls (sweep_core): the next call's mode and the measured ms per candidate
    bool serial_next = false;
    int32_t serial_calls = 0;
    int32_t serial_C = 0, serial_S = 0;     // shape of the call that decided serial_next
    float serial_ms_per = 0, pipe_ms_per = 0;
    ~SweepScratch() {
        if (gexec) (void)hipGraphExecDestroy(gexec);
    }
};

// Per-mirror scratch of ca_filter_out_schedulable / ca_try_schedule_pods (filter.hip).
struct FilterScratch {
    DevBuf in, zero, out;          // inputs (order, hints, class tables), zeroed state, outputs
    DevBuf acc;                    // ca_try_schedule_pods: isNodeAcceptable, one bit per node
    HostBuf h_in, h_out;
    DevPodTable pods;              // the pending table when the caller passes no podset
    HostBuf h_pods;                // ... staged in page-locked memory (its copies run beside the preparation)
    DevBuf gather_idx;             // podset indices of the placed pods (mirror records gathered on the device)
    float kernel_ms = 0, total_ms = 0;
    int32_t phases = 0, steps = 0, ring_scans = 0, windows = 0;
    float seq_share = 0, walk_cycles_per_pod = 0;   // CASIM_PROF builds: sequencer walk share, cycles/pod
    // feasibility-bitmap path (filter.hip k_fb_*): pods, shapes, static classes, bitmaps
    DevBuf fb_in, fb_bits;
    HostBuf h_fb;
    int32_t path = 0;              // last call: 1 bitmap walk, 0 window sequencer
    int32_t fb_shapes = 0, fb_classes = 0;
    float fb_cyc_per_pod[3] = {0, 0, 0};   // CASIM_PROF builds: bitmap walk cycles per pod (head, run, place)
    int32_t fb_stat_lds = 0;                // bitmap walk: static words in LDS
};

// Per-mirror scratch of the planner's device chain (plan_chain.hip), freed with the mirror
// and allocated on its device.
struct PlanChainScratch {
    DevBuf in, work, out;
    HostBuf h_in, h_out;
};

// Per-mirror scratch of ca_mirror_utilization / ca_scale_down_candidates_create (scaledown.hip),
// kept across calls.
struct UtilScratch {
    DevBuf in;                     // one call's inputs: [pod -> node | node rows | override ids, rows, bitmap | eligible]
    HostBuf h_in;                  // ... staged in page-locked memory, one H2D copy per call
    DevBuf acc;                    // per-node sums (util_core.h UtilSum): all zero between calls
    size_t acc_rows = 0;           // rows of acc that exist and are zero
    bool acc_dirty = false;        // a call ended without its node kernel clearing acc: zero it first
    DevBuf info, drain;            // the last call's ca_util_info rows and drain bits, [n_nodes]
    DevBuf cls;                    // ca_scale_down_candidates_create: [counts | empty | cand | status | class]
    HostBuf h_cls;
    int32_t n_nodes = 0;           // rows valid in info / drain
    float stage_ms = 0;            // host time of the last call's pod -> node staging fill (resident: the column sync)
    size_t table_pods = 0;         // resident calls: pods on nodes (the slot table's upper bound)
    int64_t h2d_bytes = 0, d2h_bytes = 0;   // bytes the last call moved across PCIe
};

// The resident per-pod columns (podcols.hip): each mirror pod's node, its slot in the node's
// NodeInfo.Pods list and the util row its caller set.  They exist from the first call of a
// resident entry point until ca_mirror_clear; the host rows stay authoritative and
// ca_mirror::sync_pod_cols brings the device copy up to date before a kernel reads it.
struct PodCols {
    PodColDirty dirty;             // node / slot entries
    PodColDirty rdirty;            // util rows and has-row flags (same `synced`)
    PodRowTable rows;              // the host copy of the util rows
    DevBuf d_node, d_slot, d_has, d_row;   // [cap] int32, int32, uint8, ca_util_pod
    size_t cap = 0;
    DevBuf d_stage;                // one sync's scatter entries
    HostBuf h_stage;               // one sync's ranges and entries, page-locked
    DevBuf d_mv;                   // ca_scale_down_candidates_create_resident: maps, table, lists
    HostBuf h_mv;
    hipEvent_t ev = nullptr;       // after the move-list kernels
    enum { ST_FULL = 0, ST_STAGED, ST_ENTRIES, ST_TAIL, ST_REORDERS, ST_SHIFTS, ST_ROWS, ST_BYTES, ST_N };
    int64_t stat[ST_N] = {0};      // ca_mirror_pod_column_stats
    ~PodCols() {
        if (ev) (void)hipEventDestroy(ev);
    }
};

// Dirty-row staging of sync_nodes: one H2D copy + a scatter kernel.
struct RowStage {
    DevBuf d;
    HostBuf h;
    HostBuf full;                  // page-locked staging: full-table hot + ext columns, appended pod records
};

// ca_plan_removals (planner.hip): the last call's moves and counters.
struct PlanStats {
    int32_t rounds = 0, conflicts = 0, simulated = 0;
    int32_t path = 0;              // 1: the device chain (plan_chain.hip), 0: speculative windows
    std::vector<uint64_t> chain_prof;   // the chain's phase cycle counters (plan_chain.hip PC_*)
    float host_ms[5] = {0, 0, 0, 0, 0};  // sync, launch+kernel, kernel, readback, replay
    float total_ms = 0;
    std::vector<ca_plan_move> moves;
};

struct Stats {
    int32_t rounds = 0;
    float kernel_ms = 0, sort_ms = 0, total_ms = 0;
    int32_t lin_sensitive = 0;    // batch output depends on the input lastIndex
    int32_t had_success = 0;      // some FitsAnyNode call of the batch succeeded
    float exact_ms = 0;           // sweep: device time of the exact pass
    float walk_ms = 0;            // sweep: host time up to the end of the exact pass
};

}  // namespace casim

namespace casim {
// The mirror's pod records: ids are never reused (Revert detaches pods, Clear() starts over),
// so the table only grows — every planner run appends its committed copies, every
// FilterOutSchedulable call its placements.  Rows live in fixed chunks of 2^16 records that
// are never moved: growing a contiguous vector past its capacity copied every record
// (~40 MB at C3 size: a 30 ms stall inside whichever call crossed the boundary).  Chunks
// come from 2 MiB-aligned anonymous mappings with transparent huge pages asked for (4 KiB
// first-touch faults cost more than the records' copies).
template <class T> class ChunkVec {
  public:
    static constexpr size_t kBits = 16, kRows = (size_t)1 << kBits, kMask = kRows - 1;
    ChunkVec() = default;
    ChunkVec(const ChunkVec&) = delete;
    ChunkVec& operator=(const ChunkVec&) = delete;
    ~ChunkVec() {
        clear();
        for (T* c : chunks_) unmap(c);
    }
    size_t size() const { return n_; }
    bool empty() const { return n_ == 0; }
    size_t capacity() const { return chunks_.size() * kRows; }
    T& operator[](size_t i) { return chunks_[i >> kBits][i & kMask]; }
    const T& operator[](size_t i) const { return chunks_[i >> kBits][i & kMask]; }
    T& back() { return (*this)[n_ - 1]; }
    void reserve(size_t n) {
        while (capacity() < n) chunks_.push_back(map());
    }
    void push_back(const T& v) {
        reserve(n_ + 1);
        new (&(*this)[n_]) T(v);
        n_++;
    }
    void resize(size_t n) {                     // (grow: value-initialised rows; shrink: dropped)
        reserve(n);
        for (size_t i = n_; i < n; i++) new (&(*this)[i]) T();
        for (size_t i = n; i < n_; i++) (*this)[i].~T();
        n_ = n;
    }
    void clear() { resize(0); }                 // (the chunks stay mapped for the next load)
    void resize_for_overwrite(size_t n) {       // grow without initialising: the caller writes every new row
        static_assert(std::is_trivially_destructible<T>::value, "rows dropped without destructors");
        if (n <= n_) { resize(n); return; }
        reserve(n);
        n_ = n;
    }

  private:
    static constexpr size_t kHuge = (size_t)2 << 20;
    static size_t bytes() { return (kRows * sizeof(T) + kHuge - 1) & ~(kHuge - 1); }
    static T* map() {
        const size_t sz = bytes();
        char* base = static_cast<char*>(mmap(nullptr, sz + kHuge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
        if (base == MAP_FAILED) throw std::bad_alloc();
        char* al = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(base) + kHuge - 1) & ~(uintptr_t)(kHuge - 1));
        if (al > base) munmap(base, (size_t)(al - base));                       // keep [al, al + sz)
        if (base + sz + kHuge > al + sz) munmap(al + sz, (size_t)(base + sz + kHuge - (al + sz)));
        (void)madvise(al, sz, MADV_HUGEPAGE);
        return reinterpret_cast<T*>(al);
    }
    static void unmap(T* c) { munmap(c, bytes()); }
    std::vector<T*> chunks_;
    size_t n_ = 0;
};
}  // namespace casim

namespace casim {
// A candidate range of a multi-device sweep (multi.hip) runs the pipeline in three calls
// on its own device, the host composing the ranges between them:
//   SP_PROBE    the probe at the guesses from guess_base (lastIndex + the pods to move of
//               every earlier sensitive candidate of the whole call); out: adv = the range's
//               advance as the probe saw it (the sum k_sweep_est would take)
//   SP_MAP      windows centred from est_base (the previous ranges' probe advances), the
//               tables, the chunk walks and k_walk_map; out: map[] (64 lastIndex-out values
//               by class of the first row, the row's fit points, the class mode), S
//   SP_RESOLVE  the walk from the true input (*last_index), the table gather and the exact
//               pass — the tail of a normal call, host walk included, so it is always exact
// Device state (probe outputs, guesses, tables, chunk maps) stays in the mirror's sweep
// scratch between the calls; nothing else may use the mirror meanwhile.
enum { SP_FULL = 0, SP_PROBE = CA_SWEEP_PHASE_PROBE, SP_MAP = CA_SWEEP_PHASE_MAP, SP_RESOLVE = CA_SWEEP_PHASE_RESOLVE };
// the map record k_walk_map writes (sweep.hip): 64 lastIndex-out values by class, then the
// first row's SWEEP_FPW fit points, then the class mode flag
constexpr int SWEEP_FPW = 65;
constexpr int SWEEP_MAP_HEAD = 64;                     // offset of the fit points
constexpr int SWEEP_MAP_MODE = 64 + SWEEP_FPW;         // offset of the mode flag
constexpr int SWEEP_MAP_INTS = 64 + SWEEP_FPW + 1;
static_assert(SWEEP_MAP_INTS == CA_SWEEP_MAP_INTS, "casim.h map record size");
// the public record (casim.h ca_sweep_phase): kind, guess_base (PROBE in), est_base (MAP
// in), adv / succ (PROBE out), n_sensitive, map_ran / map_ok / map (MAP out)
using SweepPhase = ca_sweep_phase;

// ca_mirror_reorder_nodes' argument check (CA_OK, CA_EINVAL or CA_ESTATE; nothing changed)
int mirror_reorder_check(const ca_mirror* m, const int32_t* order, int32_t n);
int64_t removal_plan_sensitive_pods(const ca_removal_plan* p);
bool removal_plan_phase_ok(const ca_removal_plan* p);             // no scope cut in the range
int32_t sweep_fp_class(const int32_t* fp, int32_t n, int32_t L);  // class of L in a row's fit points
int removal_plan_run_phase(ca_removal_plan* p, int32_t* hints, int32_t* last_index, ca_removal_result* results,
                           int32_t* out_dest, SweepPhase* ph);
}  // namespace casim

struct ca_mirror {
    int32_t device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;

    std::vector<casim::NodeRow> nodes;
    casim::ChunkVec<casim::PodRow> pods;             // by pod id (never moved)
    std::vector<ca_selector_term> terms;
    std::vector<ca_selector_req> reqs;
    std::vector<int32_t> pf_names;
    std::vector<casim::JournalEntry> journal;
    std::vector<casim::NodeRow> removed_nodes;   // rows of journaled RemoveNode ops (J_REMOVE_NODE.slot)
    int32_t depth = 0;
    int64_t n_scope_blockers = 0;          // pods in the snapshot with CA_POD_REQUIRED_ANTI_AFFINITY

    // device rows
    casim::DevBuf d_hot, d_ext, d_static;
    size_t d_cap = 0;                      // rows allocated
    size_t d_rows = 0;                     // rows valid on device
    std::vector<int32_t> dirty_rows;       // rows whose dynamic part changed
    std::vector<uint8_t> dirty_flag;
    bool static_dirty = true;              // static/ext columns need a full upload
    bool all_dirty = true;
    // ca_mirror_sync_stats: counters since create / Clear() (casim.h has the order)
    enum { SS_FULL = 0, SS_STAGED, SS_ROWS_STAGED, SS_STATIC, SS_GROWTHS, SS_DEVICE_ROWS, SS_FILL_THREADS,
           SS_PLACED_THREADS, SS_N };
    int64_t sync_stat[SS_N] = {0};
    // ca_mirror_reorder_nodes: the list order changed this many times since create (never
    // reset: a removal plan remembers the epoch it was created in); counters of
    // ca_mirror_reorder_stats (since create / Clear()); the pinned [order | inverse] pair and
    // its device copy followed by the gathered columns (not a row buffer: no SS_GROWTHS)
    int64_t order_epoch = 0;
    enum { RS_CALLS = 0, RS_DEVICE, RS_LAST_US, RS_N };
    int64_t reorder_stat[RS_N] = {0};
    casim::HostBuf h_reorder;
    casim::DevBuf d_reorder;

    // device pod table (mirror pods), appended lazily
    casim::DevPodTable d_pods;
    size_t d_pods_synced = 0;              // pods whose records are on device
    size_t d_terms_synced = 0;

    // scratch
    casim::DevBuf d_scratch0, d_scratch1, d_scratch2, d_scratch3;
    casim::DevBuf d_mask;                  // per-node match mask
    std::vector<uint8_t> h_scratch;
    casim::Stats sweep_stats;
    casim::PlanStats plan;
    casim::SweepScratch sw;
    casim::FilterScratch fo;
    casim::PlanChainScratch pc;
    casim::RowStage rs;
    casim::UtilScratch ut;
    casim::HostBuf podset_stage;           // ca_podset_create: the records' page-locked staging
    // resident HintingSimulator hints (hints.go:29-72): node per mirror pod, -1 = none
    casim::DevBuf d_pod_hints;
    size_t d_hints_n = 0;
    int ensure_pod_hints();                // grow to pods.size(), new entries -1
    // resident per-pod columns (podcols.hip); null until a resident entry point is called
    std::unique_ptr<casim::PodCols> pcol;
    int ensure_pod_cols();                 // bring them into being (all dirty)
    int sync_pod_cols();                   // push stale entries, the tail and changed util rows
    int reorder_pod_cols(const int32_t* d_inv, int32_t n);   // node column through the inverse permutation
    void pcol_mark(int32_t pod) { if (pcol) pcol->dirty.mark(pod); }
    void pcol_mark_node(int32_t node) {    // every pod now on `node`
        if (pcol) for (int32_t id : nodes[node].pods) pcol->dirty.mark(id);
    }
    int64_t n_ext_pods = 0;                // pods stored with host ports / extended requests
    int64_t n_eph_pods = 0;                // pods stored with ephemeral-storage requests
    int64_t n_oos_pods = 0;                // pods stored with CA_POD_OUT_OF_SCOPE (never decremented:
                                           // 0 lets the sweep's scope cut skip the per-pod check)

    int remap_hints_removed(int32_t pos, int32_t code, bool restore);   // resident hints around a RemoveNode
    int32_t removals = 0;                  // RemoveNode calls so far: hint codes of removed nodes
    int sync_nodes();                      // push dirty rows to the device
    int sync_pods();                       // push new pod records to the device
    void mark_dirty(int32_t node);
    void node_apply(int32_t node, const ca_pod_spec& p, int sign);
    void add_pod_to_node(int32_t pod, int32_t node);
    int32_t store_pod(const ca_pod_table* t, int32_t idx, int32_t node);
    void reserve_more(size_t n_pods_add, size_t n_journal_add);    // geometric growth before a batch
    // store_pod + add_pod_to_node of pod idx[k] on node[k] for every k with node[k] >= 0, in
    // order (ids in out_id, -1 for the others); large batches on a few host threads
    // device_rows: the caller's kernel already wrote the placed nodes' free resources to
    // d_hot (FilterOutSchedulable's bitmap walk), so they stay clean where fill_hot agrees
    void add_placed_batch(const ca_pod_table* t, const int32_t* idx, const int32_t* node, int32_t n,
                          int32_t* out_id, bool device_rows = false, bool known_plain = false);
    int32_t store_moved_copy(int32_t pod);  // the copy findPlaceFor schedules (cluster.go:235-240)
    // the planner's committed moves, candidate by candidate: RemovePod of each moved pod,
    // then the copies (ids pods.size() + t, t-th move) AddPod'ed on their nodes; large
    // batches on the worker pool, split by node (planner.hip).  CA_EDEVICE if mv[t].new_pod
    // is not the id the copy gets.
    int replay_moves(const ca_plan_move* mv, int32_t nm);
    void journal_push(int32_t kind, int32_t node, int32_t pod, int32_t slot, const uint64_t* ports);
    void fill_hot(int32_t i, casim::NodeHot& h) const;
    void fill_ext(int32_t i, casim::NodeExt& e) const;
    void fill_static(int32_t i, casim::NodeStatic& s) const;
};

struct ca_podset {
    ca_mirror* m = nullptr;
    casim::DevPodTable t;
    int32_t n_host = 0;                // pods in the set
    bool any_oos = false;              // some pod carries CA_POD_OUT_OF_SCOPE (no host copy of the records)
    bool any_refs = false;             // some pod references selector terms or PreFilter names
    // Score classes: pods with equal (score_milli_cpu, score_memory) — the only inputs of
    // calculatePodScore (binpacking_estimator.go:164-193) — share a class, numbered in
    // first-occurrence order.  d_cls[pod] = class, d_cls_sc[c] = {score_milli_cpu,
    // score_memory}.  Used by the Estimate bucket sort (estimate.hip).
    int32_t n_cls = 0;
    casim::DevBuf d_cls, d_cls_sc;
    casim::DevBuf d_cls_rep;           // a pod of each class (its first in the set)
    std::vector<int64_t> h_req;        // per pod: request cpu, memory (compact copies for plan creation)
    std::vector<uint8_t> h_pflags;     // per pod: 1 host ports, 2 extended-resource requests
    bool any_ports = false, any_scalar = false;
    bool req_below_2p53 = true;        // every pod's cpu, memory and ephemeral request: exact in float64
    std::vector<int32_t> h_cls;        // host copies: class per pod, {cpu, memory} per class
    std::vector<int64_t> h_cls_sc;
    // every class's pods carry identical records apart from their controller
    // (similar_class): interchangeable for the FFD chain, so Estimate can run the chain on
    // the stable class order while Go's sort.Slice order of their ids is computed beside it
    // — provided no two classes of a group tie on their float64 score against the group's
    // template (checked per plan: ca_estimate_plan::decouple_ok)
    bool cls_uniform = false;
    // BuildPodGroups' view of the records (podgroups.hip): per pod its similar class, or -1 for
    // a pod that is always a group of its own (no controller, DaemonSet); n_sim = max + 1
    std::vector<int32_t> h_sim;
    int32_t n_sim = 0;
};

// Pod equivalence groups built on the device (podgroups.hip): a CSR over the unschedulable
// pods of a pod set, resident for ca_expansion_plan_run_groups (the samples) and
// ca_estimate_plan_create_groups (the lists' source), with a host copy for fetch and for the
// plan's per-group facts.
struct ca_pod_groups {
    ca_mirror* m = nullptr;
    const ca_podset* s = nullptr;
    int32_t device = 0;                    // m->device (destroy does not touch the mirror)
    int32_t n_eg = 0, n_pods = 0;
    casim::DevBuf d_out;                   // eg_off | samples | eg_pod
    int32_t* d_eg_off = nullptr;           // [n_eg + 1]
    int32_t* d_samples = nullptr;          // [n_eg]: eg_pod[eg_off[e]]
    int32_t* d_eg_pod = nullptr;           // [n_pods]
    std::vector<int32_t> h_eg_off, h_eg_pod;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float build_ms = 0.f;                  // device time of the build (events around its launches)
    int32_t launches = 0;
    ~ca_pod_groups() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

namespace casim {
// Buffers and events of ca_estimate_plan_option_sums (expander.hip), kept in the plan so a
// caller that picks an option every loop allocates them once.
struct OptionSumsScratch {
    DevBuf d_in, d_sums;            // [off | n_scheduled | tile prefix] of the groups; G x 2 sums + 1
    HostBuf h;                      // page-locked staging of both
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;             // ev0 / ev1 bracket a kernel of the last call
    ~OptionSumsScratch() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// Buffers and events of ca_estimate_plan_groups_missing_pods (nodegroupset.hip), kept in the
// plan like OptionSumsScratch.
struct MissingPodsScratch {
    DevBuf d_in, d_out;             // [off | n_scheduled | tile prefix] of the rows; [n_missing | bad ids | first]
    DevBuf d_rows;                  // one batch of bitmap rows over the pod set
    DevBuf d_req;                   // a required list uploaded from another device's plan (multi.hip)
    HostBuf h;                      // page-locked staging of d_in and d_out
    std::vector<int32_t> row_of, row_group;   // group -> row or -1; row -> group
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;             // ev0 / ev1 bracket the kernels of the last call
    ~MissingPodsScratch() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// Buffers and events of ca_estimate_plan_option_price_sums (expander.hip), kept in the plan
// like OptionSumsScratch.
struct PriceSumsScratch {
    DevBuf d_in, d_price, d_out;    // [off | n_scheduled | launch order] of the groups; the pod prices; G totals + bad ids
    HostBuf h;                      // page-locked staging of all three
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;             // ev0 / ev1 bracket the kernel of the last call
    ~PriceSumsScratch() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// What expander.hip and nodegroupset.hip read of an Estimate plan (the struct itself is private
// to estimate.hip).
struct PlanLists {
    ca_mirror* m = nullptr;
    const ca_podset* s = nullptr;
    int32_t G = 0, total = 0;
    const int32_t* h_off = nullptr;        // [G + 1] group offsets into the lists
    const int32_t* h_nsched = nullptr;     // [G] n_scheduled of the last run (0 for a group not CA_OK)
    const int32_t* d_sched_pod = nullptr;  // the device lists, sched_pod layout
    bool final_lists = false;              // the last run left its final ids in d_sched_pod
    OptionSumsScratch* scratch = nullptr;
    MissingPodsScratch* missing = nullptr;
    PriceSumsScratch* price = nullptr;
};
void estimate_plan_lists(const ca_estimate_plan* p, PlanLists* out);

// The required list of filterNodeGroupsByPods as k_test_required reads it: ids [off, off + n)
// of a device buffer of `total` ids on the plan's device.  A plan's own group g is
// (d_sched_pod, total, h_off[g], h_nsched[g]); a list exported from another device and
// uploaded is (buf, n, 0, n).  first_missing positions are relative to `off` either way.
struct RequiredList {
    const int32_t* d_ids = nullptr;
    int32_t total = 0, off = 0, n = 0;
};
// The body of ca_estimate_plan_groups_missing_pods (nodegroupset.hip).  ext == nullptr: the
// required list is the plan's own group `required_group`.  Otherwise `*ext` is the required
// list, required_group is ignored and no candidate is "the required group itself".
int estimate_plan_missing_pods(ca_estimate_plan* p, const RequiredList* ext, int32_t required_group,
                               const int32_t* groups, int32_t n_groups, int32_t* n_missing, int32_t* first_missing);
// The sharded plan's exchange (multi.hip): the first n ids of `group`'s list into page-locked
// h_ids, one stream-ordered D2H; and the core above with n ids of page-locked h_ids uploaded
// into the plan's own scratch as the required list.
int estimate_plan_export_list(const ca_estimate_plan* p, int32_t group, int32_t* h_ids, int32_t n);
int estimate_plan_missing_pods_of(ca_estimate_plan* p, const int32_t* h_ids, int32_t n, const int32_t* groups,
                                  int32_t n_groups, int32_t* n_missing, int32_t* first_missing);
}  // namespace casim
