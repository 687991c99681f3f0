// solver.h -- geometry of the exact small-board solver (solver.hip), host + device.
// Kept apart from common.h / nn.h: the solver needs no dbaz_engine and none of the search or network definitions.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/dbaz.h"

#define SOLVER_MAX_E 31              // table int8 D[2^E] of at most 2 GiB
#define SOLVER_MAX_BOXES 16          // 2*R*C + R + C <= 31  =>  R*C <= 12
#define SOLVER_NO_BOX 0x80000000u    // bit 31 is never set in a mask (E <= 31): a box mask that never matches
#define SOLVER_MIN_LOW 4             // low_bits of the subcube kernel: 16-byte vectors of table entries
#define SOLVER_MAX_LOW 16            // 64 KB of LDS, low masks as uint16
#define SOLVER_MAX_HIGH 20           // high patterns of one solve: a work list of at most 2^20 workgroups over all launches
#define SOLVER_THREADS 512

// Compact edge i = rank of the edge's action index p*H*W + l*W + c among the real edges (ascending); a position's mask has
// bit i set when edge i is drawn.  Passed by value to the kernels.
struct SolverGeo {
    int32_t rows, cols, HW, A, E, n_boxes;
    uint32_t other[SOLVER_MAX_E][2];  // per edge: the three OTHER edges of each box it borders (SOLVER_NO_BOX: no such box)
    uint32_t box[SOLVER_MAX_BOXES];   // the four edges of every box
    uint8_t action[SOLVER_MAX_E + 1]; // compact edge -> action index
};

// Q of drawing free edge e in position m, given D of the successor: the mover continues after a capture.
__host__ __device__ __forceinline__ int solver_move_q(uint32_t o0, uint32_t o1, uint32_t m, int d_next)
{
    const int c = (int)((m & o0) == o0) + (int)((m & o1) == o1);
    return c ? c + d_next : -d_next;
}

// What a feature row says beyond its edges: margin = (mover's boxes) - (opponent's boxes), and get_result
// (dots_boxes_game.py:51-59) of a finished game, early end included (DBAZ_RESULT_NONE otherwise).  n_boxes = R*C, closed = boxes
// with all four edges drawn, own_b2c = plane 2, the mover's doubled boxes_to_close.  Shared by solver.hip and endgame.hip.
struct RowFacts {
    int margin, res;
};
__host__ __device__ __forceinline__ RowFacts solver_facts(int n_boxes, int closed, int own_b2c)
{
    const int mine = (n_boxes - own_b2c) / 2, theirs = closed - mine;
    const int opp_b2c = n_boxes - 2 * theirs;
    RowFacts f;
    f.margin = mine - theirs;
    f.res = DBAZ_RESULT_NONE;
    if (own_b2c == 0 && opp_b2c == 0) f.res = 0;
    else if (own_b2c < 0) f.res = 1;
    else if (opp_b2c < 0) f.res = -1;
    return f;
}

// splitmix64 finaliser of key ^ seed * golden ratio: which of a position's optimal moves a seeded evaluator picks (key: the
// solver's mask of the position; the endgame solver's XOR of 1 << (a & 63) over the free edges a).  Shared by solver.hip and
// endgame.hip.
__host__ __device__ __forceinline__ uint64_t solver_pick_mix(uint64_t key, uint64_t seed)
{
    uint64_t x = key ^ (seed * 0x9E3779B97F4A7C15ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// The evaluator's epilogue, one wavefront per position, lane = one compact edge of it (at most 64): cand = the lane's edge is
// free and the game is open, q its worth, action its action index.  Returns the picked action in every lane (-1: no candidate):
// the k-th member of the optimal set in ascending lane (= action) order, k = 0 without a seed, otherwise
// solver_pick_mix(key, seed) % n_opt with key = XOR over the free real edges a of 1 << (a & 63) -- a function of the position
// alone, whatever subgame the lanes are numbered in.
static __device__ __forceinline__ int endgame_pick(bool cand, int q, int action, uint64_t pick_seed)
{
    int best = cand ? q : -1024;
    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
    uint64_t opt = __ballot(cand && q == best);
    if (!opt) return -1;
    int k = 0;
    if (pick_seed) {
        uint32_t lo = cand ? (uint32_t)(1ull << (action & 63)) : 0u, hi = cand ? (uint32_t)((1ull << (action & 63)) >> 32) : 0u;
        for (int o = 32; o > 0; o >>= 1) {
            lo ^= (uint32_t)__shfl_xor((int)lo, o);
            hi ^= (uint32_t)__shfl_xor((int)hi, o);
        }
        k = (int)(solver_pick_mix(((uint64_t)hi << 32) | lo, pick_seed) % (uint64_t)__popcll(opt));
    }
    for (; k > 0; k--) opt &= opt - 1ull;
    return __shfl(action, __ffsll((long long)opt) - 1);
}

// How solver.hip and endgame.hip report a failure: the message goes to `err` -- the handle's, or the family's per-thread slot for
// a failed create (no handle to keep it in) -- and the code comes back.
static inline int fail(std::string &err, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

#define CHECK_HIP(err, call)                                                                                        \
    do {                                                                                                            \
        hipError_t _err = (call);                                                                                   \
        if (_err != hipSuccess) return fail(err, DBAZ_EDEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_err), __FILE__, __LINE__); \
    } while (0)

// masks of `bits` bits in ascending popcount order; off[k] .. off[k + 1] holds popcount k
static inline void popcount_order(int bits, std::vector<uint32_t> &perm, std::vector<uint32_t> &off)
{
    const uint32_t n = 1u << bits;
    off.assign(bits + 2, 0);
    for (uint32_t m = 0; m < n; m++) off[__builtin_popcount(m) + 1]++;
    for (int k = 0; k <= bits; k++) off[k + 1] += off[k];
    std::vector<uint32_t> at(off.begin(), off.end() - 1);
    perm.resize(n);
    for (uint32_t m = 0; m < n; m++) perm[at[__builtin_popcount(m)]++] = m;
}

// The solved table as an evaluator of the search engine (engine.hip; kernel and contract: k_solver_eval in solver.hip).
// solver_serves: the handle is of this board and device (*solved: its table is complete).  solver_forward has nn_forward's
// contract (nn.h) on float feature planes: rows feat[list[j]], j < *n_dev <= max_n, to P[list[j] * AS + a] and V[list[j]].
bool solver_serves(const dbaz_solver *s, int rows, int cols, int device, bool *solved);
void solver_forward(const dbaz_solver *s, hipStream_t stream, const float *feat, const int32_t *list_dev, const int32_t *n_dev, int max_n,
                    uint64_t pick_seed, float *P, float *V, int AS);

// ---- deep slot tables inside the search (dbaz_attach_tables; kernels k_slot_requests / k_slot_solve in solver.hip, the launch
// plan in slot_tables_plan.h).  The engine owns the slot regions [n_slots][2^max_free], the headers and the requests (endgame.h);
// the dbaz_tables supplies the board and max_free and is not needed after the attach: the work lists of every F <= max_free are
// built into a buffer the engine owns, so a handle may be replaced and destroyed while the engine searches on.  SlotTables is what
// a pass needs besides: the per-F work-list table, the list of roots the pass solves and its two counters, all on the device.
struct EndgameReq;     // endgame.h
struct EndgameSlotHdr; // endgame.h
#define SLOT_TABLES_GRID 512 // at most this many workgroups per k_slot_solve launch: two per CU; not tuned (DESIGN.md 5 says what was measured)
struct SlotTables {
    int32_t rows, cols, max_free;
    int32_t n_launches;               // S of slot_tables_plan.h
    uint32_t lds_bytes;
    uint32_t widest[SOLVER_MAX_E + 1];
    void *depth_dev;                  // [32] per F: L, top, plain and where its work lists are
    void *geo_dev;                    // [n_slots] BatchGeo: the roots of the running pass, in the order the atomics gave
    uint32_t *count_dev;              // [2]: roots listed by the pass of even / odd number
    uint32_t pass;
    // the pooled form (dbaz_attach_tables_pool, table_pool.h): n_tables regions shared by the slots; 0: one region per slot, and
    // none of the pool's kernels is launched
    int32_t n_tables;
    void *pool_dev;                   // TablePoolState, the free stack int32 [n_tables] behind it
    uint8_t *ask_dev;                 // [n_slots] of the running pass: the slot needs a region for its solve
    int32_t wait_mode;                // 1 (dbaz_attach_tables_pool_wait): a slot that finds the pool dry waits for a region
};
bool tables_serves(const dbaz_tables *t, int rows, int cols, int device, int *max_free);
// Uploads what the passes need for every F <= max_free and fills *st; n_tables > 0: the pooled form with that many regions, all
// free.  The device buffers it allocated come back in allocs[6] (four, and two more for the pool; the rest nullptr; the caller
// frees them).  wait: the pool's wait mode (table_pool.h).  DBAZ_OK, or an error code with the message in
// dbaz_tables_last_error(t) and nothing kept.
int slot_tables_setup(dbaz_tables *t, int n_slots, int n_tables, SlotTables *st, void *allocs[6], bool wait = false);
// One pass on `stream`: every slot with a request keeps, drops or re-solves its table (slot_request_rule, endgame.h); S + 1 launches,
// nothing read back.  stats [2] as for endgame_tables.  The pooled form: S + 3 launches -- regions given back (a drop, or a game
// that ended) are free before any is granted, grants go to the asking slots in ascending slot order, a slot left without one is
// denied and counted, and its header stays invalid.  In wait mode it is not denied: its request stands, its header says
// ENDGAME_WAITING, and the pass that grants it a region leaves `step` there (the engine step the pass belongs to; endgame.h).
void slot_tables_pass(SlotTables *st, hipStream_t stream, EndgameReq *req, EndgameSlotHdr *hdr, int8_t *tables, int n_slots,
                      unsigned long long *stats, int step = 0);
// the pooled form at a clear-all point, after the headers were zeroed on `stream`: every region free, every header's table -1
void slot_tables_pool_reset(SlotTables *st, hipStream_t stream, EndgameSlotHdr *hdr, int n_slots);
// the pool's figures as they are on the device now (the caller has waited for the queued work); all 0 for the per-slot form
hipError_t slot_tables_pool_read(const SlotTables *st, int32_t *in_use, int32_t *high_water, int64_t *denied, int32_t *waiting = nullptr,
                                 int64_t *waited = nullptr);
