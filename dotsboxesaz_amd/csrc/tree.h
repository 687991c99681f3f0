// tree.h -- host launchers of the tree / rules kernels (tree.hip)
#pragma once
#include "common.h"
#include "endgame.h"
#include "forced_playouts.h"
#include "gumbel.h"
#include "playout_cap.h"

// Evaluators that answer through the evaluation list: k_select / k_select_multi append their leaves to eval_list / eval_list2 /
// list_m, a launch between select and expand fills evalP / evalV, and expand reads (p, v) from there -- the networks and the
// solved table (DBAZ_EVAL_SOLVER, solver.hip).  eval_is_nn stays the narrower "a network": transposition cache, full rounds.
__host__ __device__ inline bool eval_uses_list(int ev) { return eval_is_nn(ev) || ev == DBAZ_EVAL_SOLVER; }

// A leaf's (p, v): computed at expansion by the formula of its evaluator, or read from evalP / evalV, where a launch between
// select and expand or the host put them.  from_table: the leaf is answered from its slot's endgame table (EndgameBufs below),
// whatever the evaluator.
__host__ __device__ inline bool leaf_reads_eval_buffers(int ev, bool from_table) { return from_table || !eval_is_formula(ev); }
// the transposition probe and insert apply to leaves that the engine's own evaluator of the model answers
__host__ __device__ inline bool leaf_uses_transpositions(int ev, bool from_table) { return !from_table && ev != DBAZ_EVAL_EXTERNAL; }

// Read ceilings of the driver rule per model (> 0: a search under the rule runs min(rule, cap) reads; 0: the rule):
//   cap     dbaz_attach_solver's solver_reads, for a search that model's solved table serves
//   eg_cap  dbaz_attach_endgame's endgame_reads, for a search whose root has at most EndgameStart::max_free free edges
struct ReadCaps {
    int32_t cap[2];
    int32_t eg_cap[2];
};

// What begin_search needs of the endgame tables (endgame.h; all zero until dbaz_attach_endgame): where it leaves the request for
// the slot's table when a search starts, and each model's max_free (0: no endgame solver attached to that model).
struct EndgameStart {
    EndgameReq *req; // [n_slots]
    int32_t max_free[2];
    int32_t release; // 1 (dbaz_attach_tables_pool): a game that ends leaves a release request (EndgameReq::want = 2) for its slot's region
};

// the arguments of the kernels that start searches (k_search_begin, k_selfplay_start, k_advance_auto), next to the configuration
struct StartArgs {
    ReadCaps caps;
    EndgameStart eg;
    PlayoutCap pc; // dbaz_selfplay_set_playout_cap: the self-play driver's launches only (all zero = off for k_search_begin)
};

// Who answers a leaf, and so which list k_select / k_select_multi put it on.  ROUTE_NONE: nobody has to (terminal, duplicate, formula
// evaluator, transposition hit).  ROUTE_MODEL0 / 1: that model's evaluator, through eval_list / eval_list2 / list_m.  ROUTE_TABLE: the
// slot's endgame table.  ROUTE_SOLVE + c: the leaf solver, class c.  tree.hip: leaf_route decides, route_counter / route_put hold the lists.
enum { ROUTE_NONE = -1, ROUTE_MODEL0 = 0, ROUTE_MODEL1 = 1, ROUTE_TABLE = 2, ROUTE_SOLVE = 3, N_ROUTES = ROUTE_SOLVE + LEAF_SOLVE_CLASSES };

// One game's endgame table per slot as an evaluator inside the search (endgame.h; all zero until dbaz_attach_endgame): a leaf of a
// slot whose searching model has one attached and whose table serves the slot's game takes ROUTE_TABLE: it goes on `list` (length
// n_eval[3]), not on eval_list / eval_list2 / list_m, and expand reads its (p, v) from evalP / evalV whatever the evaluator.
struct EndgameBufs {
    const EndgameSlotHdr *hdr; // [n_slots]
    int32_t *list;             // [n_slots * kmax] slots, or slot * kmax + k in a wave
    int32_t *leaf;             // [n_slots * kmax] the route of the leaf (of simulation k) where it is >= ROUTE_TABLE, else 0
    int32_t model[2];          // 1 = the model has an endgame solver attached
    int32_t wait;              // 1 (dbaz_attach_tables_pool_wait) = a slot may be waiting for a region of the pool: see endgame_slot_waits
    // dbaz_attach_leaf_solver (all zero until then; independent of the table state above, but for `leaf`, which either attach
    // allocates): a non-terminal leaf with at most ls_free[model] free real edges that no table serves goes on the list of its
    // class of F (endgame.h) and is solved from scratch between select and expand; expand reads it like a table's leaf.
    int32_t ls_free[2];        // the model's threshold, 0 = no leaf solver attached to it
    int32_t *ls_list;          // [LEAF_SOLVE_CLASSES][ls_cap] entries
    int32_t *ls_cnt;           // [LEAF_SOLVE_CLASSES] the lists' lengths, zeroed by expand like n_eval
    int32_t ls_cap;            // n_slots * kmax
};

void tree_launch_search_begin(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots,
                              const int32_t *num_reads_dev, StartArgs sa);
// tree_launch_select, _expand_backup, _selfplay_start, _advance_auto: gumbel_level(c) (common.h), the maximum over both models of the
// handle's Gumbel setting, says which instantiation is launched; level 0 launches the ones without a trace of the rule
void tree_launch_select(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, const EndgameBufs &G = EndgameBufs());
void tree_launch_order_evals(hipStream_t s, const TreeBufs &B, int n_slots, int step);
void tree_launch_select_multi(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, const EndgameBufs &G = EndgameBufs());
void tree_launch_expand_backup_multi(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots,
                                     const EndgameBufs &G = EndgameBufs());
void tree_launch_expand_backup(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, const EndgameBufs &G = EndgameBufs());
void tree_launch_set_positions(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots,
                               const int16_t *moves_dev, const int32_t *offsets_dev);
void tree_launch_advance_manual(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots,
                                const int32_t *moves_dev, int reuse);
void tree_launch_selfplay_start(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, StartArgs sa);
void tree_launch_advance_auto(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, StartArgs sa);
void tree_launch_get_roots(hipStream_t s, const Geo &g, const TreeBufs &B, int n_slots, double *priors, float *tv,
                           int32_t *nv, int32_t *changed, int32_t *stats, float *q, float *root_tv, int32_t *root_nv,
                           uint64_t *edges, int16_t *b2c2, int8_t *to_play, int8_t *just_played, int8_t *result,
                           int8_t *expanded);
void tree_launch_get_leaves(hipStream_t s, const Geo &g, const TreeBufs &B, int n_slots, int16_t *leaf_x,
                            uint8_t *need_eval, int32_t *n_active);
void tree_launch_slot_summary(hipStream_t s, const TreeBufs &B, int n_slots, SlotSummary *out_dev);
void tree_launch_stop_search(hipStream_t s, const TreeBufs &B, int n_slots);
void tree_launch_count_active(hipStream_t s, const TreeBufs &B, int n_slots, int32_t *out3);
void tree_launch_rules(hipStream_t s, const Geo &g, int op, int n, uint64_t *edges, int16_t *b2c2, int8_t *to_play,
                       int8_t *just_played, const int32_t *moves, int8_t *n_closed, int8_t *closed_lc, uint8_t *valid,
                       int8_t *result, int16_t *x);
