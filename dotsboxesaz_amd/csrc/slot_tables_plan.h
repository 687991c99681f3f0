// slot_tables_plan.h -- the launch plan of the deep slot tables inside the search (dbaz_attach_tables), host only
// and without HIP types: engine.hip launches what it lists, tests/test_slot_tables_plan.py compiles it with g++.
//
// A pass over the slots is a FIXED launch sequence, a pure function of max_free = M: k_slot_requests, then S launches of
// k_slot_solve.  The requests of a pass exist only on the device, so the host cannot group them by F as deep_batch_plan groups
// the roots of dbaz_tables_solve; instead every listed root walks its OWN layers, one per launch:
//   depth[F]    what deep_batch_plan gives a single root of F free edges with low_bits = 0: plain (F < DEEP_BATCH_MIN_LOW,
//               k_solver_layer's body, popcount layers F .. 0 of all bits) or the subcube body with L = default_low_bits(F),
//               popcount layers F - L .. 0 of the high bits; top = the first of those layers
//   launch s    handles, for every listed root, the root's layer k = depth[F].top - s; a root with k < 0 is finished
//   S           the largest top + 1 over F <= M: 11 at M = 20, 13 at M = 24
//   widest[s]   the largest number of workgroup-sized work items one root has in launch s: C(top, k) high patterns (subcube) or 1
//               (plain: 2^F <= 8 masks); the fixed grid strides over (root, item) pairs of n_roots x widest[s]
//   lds_bytes   2^(the largest L of any F <= M): the dynamic LDS of every launch
#pragma once

#include <stdint.h>

#include <algorithm>

#include "deep_batch.h"

struct SlotTablesDepth {
    int32_t L;   // low bits of the subcube body (0 for a plain depth)
    int32_t top; // the root's first layer: F (plain) or F - L
    bool plain;
};

struct SlotTablesPlan {
    int32_t max_free = -1;
    int32_t n_launches = 0;                           // S
    int32_t max_low = 0;                              // the largest L
    uint32_t lds_bytes = 0;                           // 2^max_low
    SlotTablesDepth depth[DEEP_BATCH_MAX_FREE + 1];   // entries F <= max_free hold
    uint32_t widest[DEEP_BATCH_MAX_FREE + 1];         // entries s < n_launches hold
};

static inline SlotTablesDepth slot_tables_depth(int F)
{
    SlotTablesDepth d;
    d.plain = F < DEEP_BATCH_MIN_LOW;
    d.L = d.plain ? 0 : default_low_bits(F);
    d.top = F - d.L;
    return d;
}

// the layer of a root of depth d that launch s handles (< 0: the root is finished), and its work items in that launch
static inline int slot_tables_layer(const SlotTablesDepth &d, int s) { return d.top - s; }
static inline uint32_t slot_tables_width(const SlotTablesDepth &d, int s)
{
    const int k = slot_tables_layer(d, s);
    if (k < 0) return 0;
    return d.plain ? 1u : deep_batch_binomial(d.top, k);
}

// 0 and the plan, or -1 for a max_free outside 0 .. 31 (the plan is empty)
static inline int slot_tables_plan(int max_free, SlotTablesPlan &p)
{
    p = SlotTablesPlan();
    for (int i = 0; i <= DEEP_BATCH_MAX_FREE; i++) {
        p.depth[i] = SlotTablesDepth{0, 0, true};
        p.widest[i] = 0;
    }
    if (max_free < 0 || max_free > DEEP_BATCH_MAX_FREE) return -1;
    p.max_free = max_free;
    for (int F = 0; F <= max_free; F++) {
        p.depth[F] = slot_tables_depth(F);
        p.n_launches = std::max(p.n_launches, p.depth[F].top + 1);
        p.max_low = std::max(p.max_low, p.depth[F].L);
    }
    p.lds_bytes = 1u << p.max_low;
    for (int s = 0; s < p.n_launches; s++)
        for (int F = 0; F <= max_free; F++) p.widest[s] = std::max(p.widest[s], slot_tables_width(p.depth[F], s));
    return 0;
}
