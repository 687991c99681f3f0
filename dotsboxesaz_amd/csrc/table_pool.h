// table_pool.h -- the pool of table regions that the slots of an engine share (dbaz_attach_tables_pool): its device
// layout and the rule by which a pass hands regions out.  Plain C++, host and device; the kernels of solver.hip (k_pool_decide,
// k_pool_grant, k_pool_reset) call this copy, and tests/table_pool_main.cpp runs it on the host.
//
// The pool is n_tables regions, a stack of the free ones and four figures.  A pass first pushes every region that is given back
// (in any order: which region a slot receives changes no result), then grants: the asking slots are ranked in ascending slot
// order, and the slot of rank r takes the r-th region from the top of the stack as long as regions last.  A slot that asks and
// gets nothing is denied and counted; nothing waits for a later pass.
//
// Wait mode (dbaz_attach_tables_pool_wait, TablePoolState::wait_mode): such a slot is not denied.  Its request stays standing, so
// every later pass ranks it with that pass's askers under the same rule -- the caller keeps its flag in `ask` raised -- until a
// region is free for it.  The grants are the same function of (free regions, asking flags); only the count of the unserved goes
// into `waited` (slot-passes spent waiting, cumulative) and `waiting` (the unserved of the last pass) instead of `denied`.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TABLE_POOL_HD __host__ __device__ inline
#else
#define TABLE_POOL_HD inline
#endif

#define TABLE_POOL_GROUP 1024 // slots that k_pool_grant's one workgroup ranks per round

// next to the free stack int32 [n_tables]: stack[0 .. top) are the free regions
struct TablePoolState {
    int32_t n_tables;
    int32_t top;        // free regions
    int32_t high_water; // the most regions held at once
    int32_t wait_mode;  // 1: an asking slot that gets nothing waits (its request stands); 0: it is denied
    int64_t denied;     // asking slots that got nothing (wait_mode 0)
    int64_t waited;     // wait_mode 1: what `denied` would have counted -- slot-passes spent waiting
    int32_t waiting;    // wait_mode 1: the slots left waiting by the last pass
    int32_t pad;
};

// the stack after a clear-all: every region free, region 0 on top
TABLE_POOL_HD int32_t table_pool_initial(int32_t n_tables, int32_t i) { return n_tables - 1 - i; }

// The grant rule.  n_free: the free regions when the grants of the pass begin (after all its releases); rank: how many asking
// slots have a lower slot index.  Returns the stack position whose region the slot takes, or -1: denied.
TABLE_POOL_HD int32_t table_pool_grant(int32_t n_free, int64_t rank) { return rank < (int64_t)n_free ? n_free - 1 - (int32_t)rank : -1; }

// the pool's figures once all n_asking slots of a pass have their answer
TABLE_POOL_HD void table_pool_settle(TablePoolState &s, int64_t n_asking)
{
    const int32_t granted = n_asking < (int64_t)s.top ? (int32_t)n_asking : s.top;
    s.top -= granted;
    if (s.wait_mode) {
        s.waited += n_asking - granted;
        s.waiting = (int32_t)(n_asking - granted);
    } else {
        s.denied += n_asking - granted;
    }
    const int32_t in_use = s.n_tables - s.top;
    if (in_use > s.high_water) s.high_water = in_use;
}

// One region goes back (sequential form; k_pool_decide takes its stack position with an atomic instead).  False: the stack is
// full already or the region is none of the pool's, and nothing is written.
TABLE_POOL_HD bool table_pool_release(TablePoolState &s, int32_t *stack, int32_t region)
{
    if ((uint32_t)region >= (uint32_t)s.n_tables || (uint32_t)s.top >= (uint32_t)s.n_tables) return false;
    stack[s.top++] = region;
    return true;
}

// The grants of one pass over all slots, one slot after the other: table[slot] becomes the region of every granted slot and stays
// as it is for the others.  k_pool_grant does the same with the ranks of TABLE_POOL_GROUP slots per round.
TABLE_POOL_HD void table_pool_grant_all(TablePoolState &s, const int32_t *stack, const uint8_t *ask, int32_t n_slots, int32_t *table)
{
    const int32_t n_free = s.top;
    int64_t rank = 0;
    for (int32_t slot = 0; slot < n_slots; slot++) {
        if (!ask[slot]) continue;
        const int32_t pos = table_pool_grant(n_free, rank++);
        if (pos >= 0) table[slot] = stack[pos];
    }
    table_pool_settle(s, rank);
}
