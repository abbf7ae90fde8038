// Stand-alone check of the Estimate plan's Go-order sort record (autoscaler_amd/csrc/
// sort_reuse_host.h): which runs may use the stored ids, and how the ids' epoch advances and
// wraps.  Host code only; build it with the host sanitizers and run it on a CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/host/sort_reuse_host_check.cpp -o sort_reuse_host_check && ./sort_reuse_host_check
#include <climits>
#include <cstdio>
#include <cstdlib>
#include "../../autoscaler_amd/csrc/sort_reuse_host.h"

using namespace casim;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static GoSortKey default_key() {
    GoSortKey k;
    k.fan_parts = 8; k.fan_min = 4096; k.fan_steps = 4; k.n_sorts = 10;
    k.decoupled = 1; k.fold = 1; k.fanned = 1; k.go_order = 1;
    return k;
}

static void keys() {
    const GoSortKey k = default_key();
    CHECK(go_sort_key_equal(k, k));
    // every field alone makes two keys differ
    for (int f = 0; f < 8; f++) {
        GoSortKey o = k;
        switch (f) {
            case 0: o.fan_parts = 4; break;
            case 1: o.fan_min = 0; break;
            case 2: o.fan_steps = 1; break;
            case 3: o.n_sorts = 11; break;
            case 4: o.decoupled = 0; break;
            case 5: o.fold = 0; break;
            case 6: o.fanned = 0; break;
            default: o.go_order = 0; break;
        }
        CHECK(!go_sort_key_equal(k, o));
        CHECK(!go_sort_key_equal(o, k));
        GoSortRecord r;
        r.valid = true; r.epoch = 3; r.key = k;
        CHECK(!go_sort_reusable(r, o, true));
    }
}

static void records() {
    const GoSortKey k = default_key();
    GoSortRecord r;
    CHECK(!go_sort_reusable(r, k, true));               // a new plan: nothing stored
    r.valid = true; r.epoch = 1; r.key = k;
    CHECK(go_sort_reusable(r, k, true));
    CHECK(!go_sort_reusable(r, k, false));              // CASIM_SORT_REUSE=0
    r.valid = false;
    CHECK(!go_sort_reusable(r, k, true));               // invalidated: a failed or coupled run
    r.valid = true; r.epoch = 0;
    CHECK(!go_sort_reusable(r, k, true));               // epoch 0 means "none" in a fan record
    r.epoch = INT32_MAX;
    CHECK(go_sort_reusable(r, k, true));
    GoSortKey coupled = k;
    coupled.decoupled = 0;
    r.key = coupled;
    CHECK(!go_sort_reusable(r, coupled, true));         // a run that is not decoupled never reuses
}

static void epochs() {
    bool wrapped = true;
    CHECK(go_sort_next_epoch(0, &wrapped) == 1 && !wrapped);
    CHECK(go_sort_next_epoch(1, &wrapped) == 2 && !wrapped);
    CHECK(go_sort_next_epoch(INT32_MAX - 1, &wrapped) == INT32_MAX && !wrapped);
    CHECK(go_sort_next_epoch(INT32_MAX, &wrapped) == 1 && wrapped);
    CHECK(go_sort_next_epoch(-5, &wrapped) == 1 && wrapped);
    // a walk across the wrap: epochs stay positive and never repeat without a cleared table
    int32_t e = INT32_MAX - 3;
    int clears = 0;
    for (int i = 0; i < 8; i++) {
        const int32_t n = go_sort_next_epoch(e, &wrapped);
        CHECK(n > 0);
        CHECK(wrapped || n == e + 1);
        CHECK(!wrapped || n == 1);
        clears += wrapped ? 1 : 0;
        e = n;
    }
    CHECK(clears == 1 && e == 5);
}

int main() {
    keys();
    records();
    epochs();
    std::printf("sort reuse host checks ok\n");
    return 0;
}
