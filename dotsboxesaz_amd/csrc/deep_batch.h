// deep_batch.h -- the launch plan of a BATCH of deep endgame solves (dbaz_tables_solve), host only and without
// HIP types: solver.hip launches what it lists, tests/test_deep_batch_plan.py compiles it with g++.
//
// n roots with F[i] free edges each go into a pool of n_tables tables of 2^max_free bytes.  Root i always owns slot i (byte
// offset i << max_free), so the table index a caller passes later is its root index.  Roots of equal F share their launches:
// a GROUP is the roots of one F in ascending root index, the groups are ordered deepest first, and a launch of a group has
// grid.y = the group's size.  Per group
//   plain   F < DEEP_BATCH_MIN_LOW or low_bits == -1: k_solver_layer, F + 1 launches (popcount layers F .. 0 of all bits),
//           grid.x = ceil(2^F / DEEP_BATCH_LAYER_THREADS)
//   else    k_solver_subcube with L = default_low_bits(F) or the given low_bits: one launch per popcount layer
//           k = F - L .. 0 of the high bits, grid.x = C(F - L, k), the high patterns of that layer
// low_bits has dbaz_deep_solve's meaning and applies to every root.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#define DEEP_BATCH_MAX_FREE 31        // SOLVER_MAX_E
#define DEEP_BATCH_MIN_LOW 4          // SOLVER_MIN_LOW
#define DEEP_BATCH_MAX_LOW 16         // SOLVER_MAX_LOW
#define DEEP_BATCH_MAX_HIGH 20        // SOLVER_MAX_HIGH
#define DEEP_BATCH_LAYER_THREADS 256  // threads of a k_solver_layer workgroup, one mask each
#define DEEP_BATCH_MAX_TABLES 65535   // a group's roots are grid.y of its launches

// 12 of 24 bits (3x3), 14 of 31 (3x4) measured fastest: small subcubes leave more workgroups per launch
static inline int default_low_bits(int E) { return std::min(14, std::max(E / 2, std::min(E, 8))); }

struct DeepBatchGroup {
    int32_t F, L;         // L: low bits of the subcube kernel (0 for a plain group)
    bool plain;
    int32_t first, count; // the group's roots are order[first .. first + count)
};

struct DeepBatchLaunch {
    int32_t group, k;     // popcount layer k of the high bits (subcube) or of all bits (plain)
    uint32_t grid_x, grid_y;
};

struct DeepBatchPlan {
    std::vector<int32_t> order;           // the root indices, group by group
    std::vector<DeepBatchGroup> groups;   // deepest first
    std::vector<DeepBatchLaunch> launches; // in launch order: group by group, k descending
    int32_t bad_root = -1;                // the root a refusal names (-1: none, or not about one root)
    std::string error;
};

static inline int64_t deep_batch_slot_offset(int32_t root, int max_free) { return (int64_t)root << max_free; }

static inline uint32_t deep_batch_binomial(int n, int k)
{
    uint64_t c = 1;
    for (int i = 1; i <= k; i++) c = c * (uint64_t)(n - k + i) / (uint64_t)i; // exact: c is C(n - k + i, i) after step i
    return (uint32_t)c;
}

static inline int deep_batch_refuse(DeepBatchPlan &p, int32_t root, const char *fmt, int a, int b, int c)
{
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    p.bad_root = root;
    p.error = buf;
    p.order.clear();
    p.groups.clear();
    p.launches.clear();
    return -1;
}

// 0 and the plan, or -1 with p.error (and p.bad_root where one root is the reason) and an empty plan
static inline int deep_batch_plan(const int32_t *F, int n, int max_free, int n_tables, int low_bits, DeepBatchPlan &p)
{
    p = DeepBatchPlan();
    if (max_free < 0 || max_free > DEEP_BATCH_MAX_FREE || n_tables < 1 || n_tables > DEEP_BATCH_MAX_TABLES)
        return deep_batch_refuse(p, -1, "a pool of %d tables of 2^%d bytes: 1 <= n_tables <= %d, max_free <= 31", n_tables, max_free, DEEP_BATCH_MAX_TABLES);
    if (n < 1 || !F) return deep_batch_refuse(p, -1, "%d roots: a solve takes at least one (the pool holds %d)", n, n_tables, 0);
    if (n > n_tables) return deep_batch_refuse(p, -1, "%d roots do not fit a pool of %d tables", n, n_tables, 0);
    for (int i = 0; i < n; i++) {
        if (F[i] < 0 || F[i] > max_free)
            return deep_batch_refuse(p, i, "root %d has %d free edges: a table of this pool holds 2^%d bytes", i, F[i], max_free);
        const bool plain = low_bits == -1 || F[i] < DEEP_BATCH_MIN_LOW;
        const int L = low_bits == 0 ? default_low_bits(F[i]) : low_bits;
        if (!plain && (L < DEEP_BATCH_MIN_LOW || L > DEEP_BATCH_MAX_LOW || L > F[i] || F[i] - L > DEEP_BATCH_MAX_HIGH))
            return deep_batch_refuse(p, i, "root %d: low_bits %d is out of range for its %d free edges (max(4, F - 20) <= low_bits <= min(F, 16); "
                                           "0 = default, -1 = plain kernel)", i, low_bits, F[i]);
    }
    p.order.resize(n);
    for (int i = 0; i < n; i++) p.order[i] = i;
    std::stable_sort(p.order.begin(), p.order.end(), [F](int32_t a, int32_t b) { return F[a] > F[b]; });
    for (int at = 0; at < n;) {
        DeepBatchGroup g;
        g.F = F[p.order[at]];
        g.plain = low_bits == -1 || g.F < DEEP_BATCH_MIN_LOW;
        g.L = g.plain ? 0 : low_bits == 0 ? default_low_bits(g.F) : low_bits;
        g.first = at;
        while (at < n && F[p.order[at]] == g.F) at++;
        g.count = at - g.first;
        const int32_t gi = (int32_t)p.groups.size();
        p.groups.push_back(g);
        const int top = g.plain ? g.F : g.F - g.L;
        for (int k = top; k >= 0; k--) {
            DeepBatchLaunch l;
            l.group = gi;
            l.k = k;
            l.grid_x = g.plain ? (uint32_t)((((uint64_t)1 << g.F) + DEEP_BATCH_LAYER_THREADS - 1) / DEEP_BATCH_LAYER_THREADS)
                               : deep_batch_binomial(top, k);
            l.grid_y = (uint32_t)g.count;
            p.launches.push_back(l);
        }
    }
    return 0;
}
