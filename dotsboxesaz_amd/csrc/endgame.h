// endgame.h -- sizes and device-side geometry of the exact endgame solver (endgame.hip).
// Needs solver.h (solver_move_q, solver_facts, popcount_order, SOLVER_NO_BOX) and include/dbaz.h only.
#pragma once

#include "solver.h"

#define ENDGAME_MAX_FREE 16   // 2^16 int8 = 64 KB of LDS per position, subgame masks as uint16
#define ENDGAME_THREADS 512   // SOLVER_THREADS; one lane per real edge during setup needs E < DBAZ_MAX_A <= ENDGAME_THREADS
#define ENDGAME_OFF_STRIDE (ENDGAME_MAX_FREE + 2)

// Real edge i = rank of the edge's action index among the real edges of the board (ascending), as in solver.h, for any board with
// A <= DBAZ_MAX_A.  The per-edge tables live in HBM (E < 256 edges do not fit the kernel arguments):
//   action [E]        real edge -> action index
//   nbr    [E][2][3]  per bordering box the action indices of its three OTHER edges (-1, -1, -1: no such box)
//   perm   [2^17 - 1] for every F = 0 .. 16 the masks of F bits in ascending popcount order, list F at 2^F - 1
//   off    [17][18]   off[F][k] .. off[F][k + 1]: the masks of popcount k within list F
struct EndgameGeo {
    int32_t rows, cols, HW, A, E, max_free;
    const uint8_t *action;
    const int16_t *nbr;
    const uint16_t *perm;
    const uint32_t *off;
};

// ---- one game's table as an evaluator inside the search (engine.hip / tree.hip; kernels: k_endgame_table, k_endgame_eval) --------
// D depends only on which edges are free: once a search root has F0 <= max_free free edges, every position that can follow it in
// that game is a subset of those edges.  The slot keeps the root's 2^F0-byte table in HBM and answers the leaves by lookup.
//
// begin_search (tree.hip) leaves a request for every search that starts under a model with an endgame attached; k_endgame_table,
// one workgroup per slot, returns at once where there is none.
struct EndgameReq {
    uint64_t free_edges[4]; // the root's free real edges by action index
    int64_t game;           // Slot::game_idx
    int32_t want;           // 1: a search has started; 2 (pooled deep attach only): the game is over, its region goes back; cleared by the pass
    int32_t model;          // the model that searches (its pick seed serves the leaves)
};

// Header of a slot's table.  The table serves a position of game `game` whose free edges are a subset of free_edges; compact edge
// j = the j-th of free_edges in ascending action order, bit j of a table index = compact edge j has been drawn since.
struct EndgameSlotHdr {
    uint64_t free_edges[4];
    int64_t game;                            // validity stamp: the slot's game when the table was solved
    int32_t valid, F0;
    int32_t model;
    int32_t table;                           // the region of `tables` that holds it: the slot's own (k_endgame_table, dbaz_attach_tables),
                                             // or one of the engine's pool (dbaz_attach_tables_pool; -1 there: the slot holds none)
    // dbaz_attach_tables_pool_wait only (0 otherwise).  ENDGAME_WAITING: the slot's solve request found the pool dry and stands;
    // k_select / k_select_multi leave the slot alone.  > 0: the engine step of the pass that granted it a region and solved its
    // table -- that pass runs next to k_select of the same step, which leaves the slot alone once more (tree.hip, set_phase_stamped)
    int32_t wait;
    int32_t pad;
    // sized for the deep attach (dbaz_attach_tables, k_slot_requests in solver.hip): k_endgame_table fills 16 entries at the most
    uint32_t other[SOLVER_MAX_E][2];         // solver_move_q's box masks over the compact edges
    uint8_t act[SOLVER_MAX_E];               // compact edge -> action index
};

#define ENDGAME_WAITING (-1) // EndgameSlotHdr::wait

// what the search side asks (tree.hip): does the slot's table serve the leaves of a search of game `game`
__host__ __device__ __forceinline__ bool endgame_hdr_serves(const EndgameSlotHdr &h, int64_t game) { return h.valid != 0 && h.game == game; }

// What a pass does with a slot's request (k_endgame_table, k_slot_requests): a position the slot's table still serves -- the same
// game, free edges a subset of the table's -- keeps the table; F > max_free drops it; anything else is solved.  free_edges: the
// request's, masked with the board's real edges.
struct SlotDecision {
    int F;
    bool keep, solve;
};
__host__ __device__ __forceinline__ SlotDecision slot_request_rule(const uint64_t (&free_edges)[4], int hdr_valid, int64_t hdr_game,
                                                                   const uint64_t (&hdr_free)[4], int64_t game, int max_free)
{
    SlotDecision d;
    d.F = 0;
    bool subset = true;
    for (int w = 0; w < 4; w++) {
        subset = subset && (free_edges[w] & ~hdr_free[w]) == 0ull;
        d.F += __builtin_popcountll(free_edges[w]);
    }
    d.keep = hdr_valid != 0 && hdr_game == game && subset;
    d.solve = !d.keep && d.F <= max_free;
    return d;
}

struct dbaz_endgame;
// the engine's side, like solver_serves / solver_forward (solver.h)
bool endgame_serves(const dbaz_endgame *g, int rows, int cols, int device, int *max_free);
size_t endgame_table_stride(const dbaz_endgame *g); // bytes of one slot's table region: max(16, 2^max_free)
// stats [2]: tables solved, leaves served (cumulative, device)
void endgame_tables(const dbaz_endgame *g, hipStream_t stream, EndgameReq *req, EndgameSlotHdr *hdr, int8_t *tables, int n_slots,
                    unsigned long long *stats);
// The slot tables as an evaluator, whoever solved them (k_endgame_table, or solver.hip's slot_tables_pass): k_endgame_eval with
// nn_forward's contract on rows of T = float (TreeBufs.feat planes) or int16 -- rows x[list[j]], j < *n_dev <= max_n, of slot
// list[j] / per_slot, to P[list[j] * AS + a] and V[list[j]]; seeds: the pick seed of each model.  No header claims more than
// max_free compact edges; a header's table is region EndgameSlotHdr::table of the n_tables regions of tab_stride >= 2^max_free bytes.
template <typename T>
void endgame_forward(int rows, int cols, int max_free, size_t tab_stride, int n_tables, hipStream_t stream, const EndgameSlotHdr *hdr, const int8_t *tables,
                     const T *x, const int32_t *list_dev, const int32_t *n_dev, int max_n, int per_slot, uint64_t seed0, uint64_t seed1, float *P,
                     float *V, int AS, unsigned long long *stats);

// ---- leaves solved from scratch inside the search (dbaz_attach_leaf_solver; kernel: k_endgame_leaves) ---------------------------
// A leaf with F <= the model's threshold that no table serves is listed by k_select / k_select_multi in the class of its F -- the
// classes of k_endgame_targets, deepest first: a class's workgroups hold 2^f_hi bytes of LDS -- and one fixed-grid launch per class
// the threshold reaches solves the listed leaves between select and expand.  An entry is the leaf's row (the slot, or
// slot * K + k in a wave) with the searching model in bit LEAF_SOLVE_MODEL_SHIFT.
#define LEAF_SOLVE_CLASSES 4
#define LEAF_SOLVE_MODEL_SHIFT 30
__host__ __device__ __forceinline__ int leaf_solve_class(int F) { return F >= 16 ? 0 : (F >= 14 ? 1 : (F >= 11 ? 2 : 3)); }
// list_dev [LEAF_SOLVE_CLASSES][cap] and cnt_dev [LEAF_SOLVE_CLASSES] are the caller's (the engine's); rows of x = TreeBufs.feat
// planes; rows outside [0, max_n) are skipped.  leaf_free: the largest threshold attached (classes above it are not launched);
// stats [17] (cumulative, device): leaves solved per F.  Nothing of g is written.
void endgame_solve_leaves(const dbaz_endgame *g, hipStream_t stream, int leaf_free, const int32_t *list_dev, const int32_t *cnt_dev, int cap,
                          const float *x, int max_n, uint64_t seed0, uint64_t seed1, float *P, float *V, int AS, unsigned long long *stats);

// ---- exact training targets (dbaz_exact_targets, include/dbaz.h): rows x_stride shorts apart, relabelled in place, queued on
// `stream`.  stats_host [4 + 17] (may be NULL) as dbaz_dataset_exact_targets documents it: asking for it waits for the stream.
// The message of a failure is dbaz_endgame_last_error(g)'s.
int endgame_targets(dbaz_endgame *g, hipStream_t stream, int32_t n, const int16_t *x, int x_stride, int pi_mode, int z_mode, float *pi, float *z,
                    int16_t *n_free, float *mass, uint8_t *relabelled, int64_t *stats_host);
