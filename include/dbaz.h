/*
 * dbaz.h -- C ABI of the MI355X-native self-play rollout engine (libdbaz_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path of damlobster/DotsBoxesAZ:
 * rules + sequential PUCT search + batched policy/value evaluation + the
 * self-play driver.  The reference has no FFI layer of its own (it is pure
 * Python); each entry point below names the reference interface it replaces
 * (file:line relative to the reference repo).  The ctypes binding a maintainer
 * would add on the reference side is shown in INTEGRATION.md and shipped in
 * dotsboxesaz_amd/_lib.py.
 *
 * Conventions
 *   - every function returns 0 on success, a DBAZ_E* code otherwise;
 *     dbaz_last_error() returns the message (maps to ValueError for
 *     DBAZ_EILLEGAL, RuntimeError otherwise);
 *   - all pointers are HOST pointers unless the name ends in _dev; the caller
 *     owns every buffer; no torch types, no C++ types;
 *   - a handle is single-threaded; one handle per GPU / rank; no process-global
 *     state (board size is per handle, unlike BoxesState.init_static_fields; the
 *     message of a call that has no handle -- a failed create -- is kept per thread);
 *   - there is NO CPU fallback: without a HIP device dbaz_create fails.
 *
 * Board geometry: rows x cols boxes, H = rows+1, W = cols+1, A = 2*H*W action
 * slots, action = p*H*W + l*W + c (dots_boxes_game.py:62).  A <= 256.
 */
#ifndef DBAZ_H
#define DBAZ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DBAZ_OK 0
#define DBAZ_EINVAL 1   /* bad argument */
#define DBAZ_EILLEGAL 2 /* illegal move (reference: ValueError, dots_boxes_game.py:63-65) */
#define DBAZ_EDEVICE 3  /* HIP runtime error / no device */
#define DBAZ_EPOOL 4    /* per-game node pool exhausted: raise nodes_per_slot */
#define DBAZ_ESTATE 5   /* call sequence error */

#define DBAZ_MAX_A 256
#define DBAZ_ABI_VERSION 3 /* dbaz_version(): bumped whenever dbaz_config / dbaz_counters change layout or meaning */

/* dbaz_config.debug_flags */
#define DBAZ_DBG_EARLY_JOIN 1u  /* join the driver pass in front of the network launch (round 2's first order) */
#define DBAZ_DBG_NO_FALLBACK 2u /* reserved: formerly skipped the exact-f32 safety net of nn_precision = 1; dbaz_create rejects it */
#define DBAZ_DBG_LAZY_GC 4u     /* node collector recycles dropped nodes only when fewer than 64 indices are available (A/B) */
#define DBAZ_RESULT_NONE 2

/* evaluator kinds (what plays the role of async_nn, mcts.py:187) */
#define DBAZ_EVAL_FORMULA_HASH 0    /* integer-hash priors/value (bit-exact test evaluator) */
#define DBAZ_EVAL_FORMULA_UNIFORM 1 /* uniform priors, v = 0 (tree + rules only) */
#define DBAZ_EVAL_RESNET 2          /* ResNetZero, HIP MFMA kernels (nn.py:108-122) */
#define DBAZ_EVAL_SIMPLENN 3        /* SimpleNN, 3x3 boards (dots_boxes_nn.py:61-98) */
#define DBAZ_EVAL_EXTERNAL 4        /* caller supplies (p, v) per leaf: dbaz_select / dbaz_expand_backup */
#define DBAZ_EVAL_SOLVER 5          /* perfect play from a solved table (boards of at most 31 edges): dbaz_attach_solver */

typedef struct dbaz_engine dbaz_engine;

/* configuration.py:82-100 values + sizing */
typedef struct {
    int32_t rows, cols;
    int32_t n_slots;        /* concurrent games resident on the GPU */
    int32_t nodes_per_slot; /* node pool per game; 0 = 10*(mcts_num_read+2), up to 4x that while all pools fit 96 GiB */
    int32_t mcts_num_read;  /* self_play.mcts.mcts_num_read */
    double cpuct, cpuct_base; /* self_play.mcts.mcts_cpuct */
    double noise_alpha, noise_coeff; /* self_play.noise */
    int32_t reuse_tree;     /* self_play.reuse_mcts_tree */
    int32_t n_temp;         /* self_play.mcts.temperature {move_idx: T} */
    int32_t temp_idx[8];
    double temp_val[8];
    int32_t evaluator;      /* DBAZ_EVAL_* */
    int32_t device;         /* HIP device ordinal */
    uint64_t seed;          /* Philox key for move sampling / Dirichlet noise */
    int32_t max_out_rows;   /* capacity of the finished-sample buffer; 0 = max(4096, 2*n_slots*(E+1)) */
    int32_t nn_precision;   /* 0 = exact f32 MFMA; 1 = f16x3 split MFMA (f32-grade; an evaluation whose activations leave
                             * f16's range is redone in exact f32 on the device, counters.f32_fallback_evals) */
    int32_t match_play;     /* two-model match play (self_play.compute_elo, :309-344): the evaluator of a move's
                               search is model (root.to_play XOR game_idx&1) */
    int32_t evaluator2;     /* DBAZ_EVAL_* of model 1 (match play; any kind but DBAZ_EVAL_EXTERNAL) */
    int32_t transposition_cache; /* 0 = on for network evaluators (default), 1 = off, 2 = on for network AND formula
                             * evaluators (parity tests of the hit path).  The reference caches (p, v) by position hash
                             * (utils/proxies.py:35-43); results are identical either way */
    int32_t max_pending_evals; /* UCT_search's max_pending_evals (mcts.py:183) = self_play.mcts.max_async_searches
                             * (self_play.py:27-30): simulations of ONE tree in flight.  0 / 1 = the sequential search (all
                             * parity paths); K > 1 = waves of up to K selections with virtual loss, one batched evaluation per
                             * wave (dbaz_search / dbaz_search_timed, and the self-play driver when selfplay_pending != 0) */
    int32_t selfplay_pending;  /* self-play driver (dbaz_run / dbaz_step): 0 = one simulation per game and step (default: the
                             * batch comes from the concurrent games); 1 = every search of a game runs in waves of
                             * max_pending_evals simulations with the reference's bookkeeping (visits added at backup,
                             * mcts.py:105-132), as self_play.py:27-30 does with max_async_searches */
    int32_t eval_round;     /* "full rounds only" (DESIGN 4): 0 = the network's own round size (workgroups per launch round x
                             * samples per workgroup), -1 = off (every leaf is evaluated in the step that selected it),
                             * r > 0 = rounds of r leaves (tests: small runs through the same path) */
    int32_t eval_defer_max; /* with eval_round > 0: the largest left-over that is put off to the next step (0 = r - 1) */
    uint32_t debug_flags;   /* measurement aids, 0 in production: DBAZ_DBG_* */
    int32_t reserved[3];
} dbaz_config;

typedef struct {
    int64_t steps;          /* simulation steps launched */
    int64_t expansions;     /* completed _search calls (node expansions) */
    int64_t nn_evals;       /* leaves sent to the evaluator */
    int64_t terminal_leaves;
    int64_t sum_path;       /* sum over expansions of the search-path length (nodes) */
    int64_t games_finished;
    int64_t rows_ready;     /* sample rows waiting in the output buffer */
    int64_t moves_played;
    int64_t pool_high_water;/* max nodes in use in any slot */
    int32_t active_slots;   /* slots still playing */
    int32_t error_slots;    /* slots stopped by an error (pool exhausted) */
    int32_t blocked_slots;  /* finished games waiting for room in the output buffer: fetch samples */
    int32_t f32_fallback_evals; /* nn_precision = 1, ResNetZero: leaves whose f16x3 evaluation left f16's range and were
                                 * re-evaluated by the exact-f32 tower in the same step (normally 0) */
    /* HIP-event timing of the last timed region (dbaz_timing_begin/_end) */
    double ms_total, ms_tree, ms_nn;
    int64_t nn_launches;    /* conv-tower launches inside the timed region */
    double ms_nn_tower;     /* summed duration of the dominant conv kernel */
    int64_t cache_hits;     /* leaves whose (p, v) came from an already evaluated twin position of the same tree */
    int64_t pool_resets;    /* self-play driver: moves that started from a fresh root because the subtree kept by tree reuse would
                             * not have left mcts_num_read + 2 nodes of the slot's pool free (the reference's trees are unbounded;
                             * 0 unless a network concentrates its visits for many plies in a row: raise nodes_per_slot) */
} dbaz_counters;

const char *dbaz_last_error(const dbaz_engine *e); /* e may be NULL: error of the last dbaz_create */
int dbaz_version(void);            /* DBAZ_ABI_VERSION the library was built with */
const char *dbaz_build_info(void); /* "src=<sha256[:16] of csrc/ + include/dbaz.h> nn=<the same of the network kernels>": ties profiles/ counter files to a build */
int dbaz_nodes_per_slot(const dbaz_engine *e); /* the node pool size in effect (dbaz_config.nodes_per_slot = 0: the default rule) */

int dbaz_create(const dbaz_config *cfg, dbaz_engine **out);
void dbaz_destroy(dbaz_engine *e);
int dbaz_sync(dbaz_engine *e);

/* ---- G1-G6: batched rules on SoA states (dots_boxes_game.py:30-109) --------------
 * state i = { edges[4*i..4*i+3] : bitmask of played edges (= hash[0], :106-109),
 *             b2c2[2*i..2*i+1]  : 2*boxes_to_close (integers; :39,:86),
 *             to_play[i], just_played[i] (-1 = None) } */
int dbaz_rules_init(dbaz_engine *e, int32_t n, uint64_t *edges, int16_t *b2c2, int8_t *to_play,
                    int8_t *just_played);                                   /* __init__ :30-39 */
int dbaz_rules_valid_moves(dbaz_engine *e, int32_t n, const uint64_t *edges,
                           uint8_t *valid /*[n*A]*/);                       /* get_valid_moves :44-49 */
int dbaz_rules_play(dbaz_engine *e, int32_t n, uint64_t *edges, int16_t *b2c2, int8_t *to_play,
                    int8_t *just_played, const int32_t *moves,
                    int8_t *n_closed /*[n]; -1 = illegal, state untouched*/,
                    int8_t *closed_lc /*[n*4] (l,c) pairs, -1 padded; may be NULL*/); /* play_ :61-89 */
int dbaz_rules_result(dbaz_engine *e, int32_t n, const int16_t *b2c2, const int8_t *to_play,
                      int8_t *result /* 1,0,-1 or DBAZ_RESULT_NONE */);    /* get_result :51-59 */
int dbaz_rules_features(dbaz_engine *e, int32_t n, const uint64_t *edges, const int16_t *b2c2,
                        const int8_t *to_play, int16_t *x /*[n*3*H*W]*/);  /* get_features :96-100 */

/* ---- N1-N3: policy/value network (nn.py:108-129,155-160; dots_boxes_nn.py:61-105) ----
 * Weights arrive as state_dict entries under the reference's key names
 * ("resnet.resblocks.3.conv1.weight", ...), any order; dbaz_nn_commit folds the
 * eval-mode BatchNorms and uploads. */
/* kind DBAZ_EVAL_RESNET: channels <= 128 (zero-padded to 16/32/64/128), blocks, head_channels, value_fc as in
 * configuration.py:134-156.  kind DBAZ_EVAL_SIMPLENN: the other arguments are ignored; 3x3 boards only. */
int dbaz_nn_configure(dbaz_engine *e, int32_t kind /*DBAZ_EVAL_RESNET|SIMPLENN*/, int32_t channels,
                      int32_t blocks, int32_t head_channels, int32_t value_fc);
/* match play: subsequent dbaz_nn_configure/_set_tensor/_commit/_predict address model 0 or 1 */
int dbaz_nn_select_model(dbaz_engine *e, int32_t model);
int dbaz_nn_set_tensor(dbaz_engine *e, const char *key, const float *data, int64_t numel);
int dbaz_nn_commit(dbaz_engine *e);
/* NeuralNetWrapper.predict_sync: X float32 [n,3,H,W] -> softmax p [n,A], tanh v [n] */
int dbaz_nn_predict(dbaz_engine *e, int32_t n, const float *X, float *p, float *v);

/* ---- M1-M9: batched sequential search, one tree per slot (mcts.py) ----------------- */
/* per-call arguments of UCT_search: cpuct=(c, base), dirichlet=(alpha, coeff) (mcts.py:183,205,211) */
int dbaz_set_search_params(dbaz_engine *e, double cpuct, double cpuct_base, double noise_alpha, double noise_coeff);
/* create_root_uct_node for every slot: slot i starts from the position reached by
 * moves[offsets[i]..offsets[i+1]) (NULL, NULL = empty boards).  mcts.py:156-160 */
int dbaz_set_positions(dbaz_engine *e, const int16_t *moves, const int32_t *offsets);
/* UCT_search on every slot with max_pending_evals=1 semantics (mcts.py:183-244).
 *   num_reads[n_slots]  NULL = the driver rule min(4*n_valid!, mcts_num_read) (self_play.py:64-65)
 *   noise[n_slots*A]    Dirichlet sample per slot over ALL A slots (used if noise_alpha>0);
 *                       NULL = drawn on the device (Philox)
 * Blocks until every slot finished its reads.  Not for DBAZ_EVAL_EXTERNAL. */
int dbaz_search(dbaz_engine *e, const int32_t *num_reads, const double *noise);
/* the same with UCT_search's wall-clock cut-off (mcts.py:201-203,232-233; players.py:55-69 calls
 * UCT_search(node, int(1e12), ..., time_limit)): reads that have not started when time_limit_s (<= 0: 120 s) has
 * elapsed are dropped; the root expansion is never cut; the clock is read between waves */
int dbaz_search_timed(dbaz_engine *e, const int32_t *num_reads, const double *noise, double time_limit_s);
/* per-call max_pending_evals of a handle created with max_pending_evals = K > 1: 1 <= k <= K simulations in flight
 * (k = 1 through the same kernels reproduces the sequential search bit for bit).
 * virtual_visits = 0: the reference's bookkeeping -- a simulation's visits are added at backup, only `total_value -=
 * VIRTUAL_LOSS` marks its path while it is pending (mcts.py:105-132); with an evaluator that suspends once per call
 * the reference's searches run in exactly these waves, and the results are equal bit for bit (tests/golden/pending.npz).
 * virtual_visits = 1 (default): the visit is counted on every edge of the path at selection time as well, so the
 * simulations of a wave spread over the tree (the reference's in-flight leaves are mostly duplicates). */
int dbaz_set_pending(dbaz_engine *e, int32_t k, int32_t virtual_visits);
/* external-evaluator form of the same call: begin, then loop
 *   dbaz_select -> (evaluate leaves on the host) -> dbaz_expand_backup  until *n_active == 0 */
int dbaz_search_begin(dbaz_engine *e, const int32_t *num_reads, const double *noise);
int dbaz_select(dbaz_engine *e, int32_t *n_active,
                int16_t *leaf_x /*[n_slots*3HW] get_features of each leaf*/,
                uint8_t *need_eval /*[n_slots] 1 = non-terminal leaf of an active slot*/);
int dbaz_expand_backup(dbaz_engine *e, const float *p /*[n_slots*A]*/, const float *v /*[n_slots]*/);
/* root arrays after a search (what UCT_search returns / tests inspect); any pointer may be NULL */
int dbaz_get_roots(dbaz_engine *e, double *priors /*[n*A]*/, float *total_value /*[n*A]*/,
                   int32_t *visits /*[n*A]*/, int32_t *changed /*[n*A]*/,
                   int32_t *stats /*[n*3]: max_deepness, tree_size, terminal_count*/,
                   float *q_value /*[n]*/, float *root_tv /*[n]*/, int32_t *root_nv /*[n]*/);
/* root game states (edges/b2c2/to_play/just_played/result/expanded) */
int dbaz_get_root_states(dbaz_engine *e, uint64_t *edges, int16_t *b2c2, int8_t *to_play,
                         int8_t *just_played, int8_t *result, int8_t *expanded);
/* init_mcts_tree on every slot (mcts.py:163-180); moves[i] < 0 leaves slot i alone */
int dbaz_advance(dbaz_engine *e, const int32_t *moves, int32_t reuse_tree);

/* ---- D1-D3: self-play driver (self_play.py:19-156) ---------------------------------- */
/* Start playing games first_game_idx .. first_game_idx+n_games-1; every slot takes the next
 * unplayed index when its game ends (generate_games' chunking, self_play.py:291-306), handed out
 * in slot order at the next step, so a run plays the same games on the same slots every time
 * as long as the output buffer has room (slots that find it full wait in PH_EMIT in atomic order). */
int dbaz_selfplay_start(dbaz_engine *e, int64_t n_games, int64_t first_game_idx);
/* Start positions of the next dbaz_selfplay_start (SelfPlay.play_games(game_state, idxs),
 * self_play.py:51-55,76-80): start s is the position reached from the empty board by
 * moves[offsets[s] .. offsets[s+1]).  Game g starts from start (g / games_per_start) % n_starts,
 * g being the ABSOLUTE game index (>= 0).  n_starts = 1 is the reference's contract (one game_state for
 * all games); n_starts > 1 is an opening book.  n_starts = 0 (moves, offsets may be NULL) clears.
 * move_idx, the temperature schedule, scripts and the Philox streams count plies from the start position;
 * the first row of a game has move = -1.
 * Like dbaz_selfplay_script it applies to the next dbaz_selfplay_start only and is consumed by it.
 * Checked on the host with the rules the kernels run, before anything reaches the device:
 *   an illegal move in a start                                   -> DBAZ_EILLEGAL (names start and ply)
 *   a start that is already finished (the reference would record a game without rows; refused here),
 *   n_starts < 0 or > DBAZ_MAX_STARTS, games_per_start < 1, offsets negative or descending
 *                                                                -> DBAZ_EINVAL
 *   games of an earlier dbaz_selfplay_start still being played   -> DBAZ_ESTATE
 * A failed call leaves the starts of the previous successful call (if not yet consumed) in place.
 * Together with dbaz_selfplay_fastforward the next dbaz_selfplay_start returns DBAZ_EINVAL and drops both. */
#define DBAZ_MAX_STARTS 65536
int dbaz_selfplay_set_start(dbaz_engine *e, const int16_t *moves, const int32_t *offsets,
                            int32_t n_starts, int32_t games_per_start);
/* teacher forcing for parity tests: moves / Dirichlet vectors for game `game_idx`
 * (noise may be NULL).  Must be called before dbaz_selfplay_start. */
int dbaz_selfplay_script(dbaz_engine *e, int64_t game_idx, const int16_t *moves, int32_t n_moves,
                         const double *noise /*[n_moves*A]*/);
/* synthetic mid-game population for benchmarking: slot i is advanced by plies[i]
 * uniformly random legal moves before its first search. */
int dbaz_selfplay_fastforward(dbaz_engine *e, const int32_t *plies);
/* benchmark population, second knob: the FIRST search of slot i is cut to min(rule, first_reads[i]) reads
 * (0 = the rule), so that the slots' move boundaries -- re-rooting, tree reuse, game turnover -- are spread over a
 * whole search instead of falling into the same steps.  Like dbaz_selfplay_fastforward it applies to the next
 * dbaz_selfplay_start only and is never used on the parity paths. */
int dbaz_selfplay_stagger(dbaz_engine *e, const int32_t *first_reads);
/* benchmark population, third knob: the first plies[i] plies of slot i's FIRST game are searched with `reads` simulations
 * per move instead of mcts_num_read -- real search, network, temperature schedule and tree reuse, only cheaper -- so that
 * the slots reach mid-game positions of the kind search-based play produces (uniformly random plies, the fastforward knob,
 * give positions with more terminal leaves and transpositions than games do).  Applies to the next dbaz_selfplay_start. */
int dbaz_selfplay_quickplay(dbaz_engine *e, const int32_t *plies, int32_t reads);
/* Playout cap randomization (Wu 2019, section 3.1): a random share full_prob of the searches that the self-play driver starts
 * are full searches -- today's search to the bit: the driver rule's reads, root noise, a row that trains -- and every other
 * one is a fast search: min(driver rule, fast_reads) reads (solver_reads, endgame_reads, the stagger and quickplay budgets
 * apply on top, as for any search), the root prepared as UCT_search(..., dirichlet=(0.0, 0.0)) prepares it (a scripted noise
 * vector for that ply is ignored), and bit 0 of its replay row's flag word set (the int16 at byte 26 of the packed row, "pad"
 * in the numpy dtypes; 0 on every row otherwise).  Temperature schedule, move draw, tree reuse, the pool guard
 * (mcts_num_read + 2), transpositions, full rounds and endgame tables are untouched; explicit searches (dbaz_search*) never
 * see the cap.
 * The rule, in full: the search of game g (absolute index) at ply i (counted from the game's start position, like move_idx)
 * under seed s (dbaz_config.seed) is full iff  x < floor(full_prob * 2^32),  x being output word 0 of Philox4x32-10 with
 *   counter (lo32(g), hi32(g), i, 0x33333333)   and   key (lo32(s), hi32(s)),
 * g taken as its 64-bit two's complement pattern.  Philox4x32-10: ten times
 *   (c0, c1, c2, c3) <- (hi(0xCD9E8D57 * c2) ^ c1 ^ k0,  lo(0xCD9E8D57 * c2),  hi(0xD2511F53 * c0) ^ c3 ^ k1,  lo(0xD2511F53 * c0)),
 *   (k0, k1) <- (k0 + 0x9E3779B9, k1 + 0xBB67AE85)   (mod 2^32; hi / lo: the halves of the 64-bit product);
 * word 0 is c0 after the tenth round.  Check value: counter (1, 2, 3, 0x33333333), key (7, 0) gives 1157962352.
 * A function of (seed, game, ply) alone: never of slot, step, rank or schedule.
 *
 * dbaz_selfplay_set_playout_cap is a setting of the handle: it holds for every later dbaz_selfplay_start (not consumed).
 * full_prob >= 1.0 switches the cap off (the state after dbaz_create; fast_reads is then ignored); full_prob = 0 makes every
 * search fast.
 *   full_prob NaN or outside [0, 1], fast_reads < 1 while full_prob < 1, a match_play handle   -> DBAZ_EINVAL
 *   games of an earlier dbaz_selfplay_start still being played                                 -> DBAZ_ESTATE
 * A failed call changes nothing.
 * dbaz_get_playout_cap: the setting (full_prob as given; 1.0 and 0 when off) and the full and fast searches the driver has
 * started since the last dbaz_selfplay_start, which zeroes them (with the cap off every search counts as full).  Any output
 * pointer may be NULL.
 * dbaz_playout_cap_is_full: the rule above on the host -- no handle, no device: 1 = full, 0 = fast, -1 = full_prob NaN or
 * outside [0, 1].  full_prob >= 1.0 answers 1. */
int dbaz_selfplay_set_playout_cap(dbaz_engine *e, double full_prob, int32_t fast_reads);
int dbaz_get_playout_cap(dbaz_engine *e, double *full_prob, int32_t *fast_reads, int64_t *full_searches, int64_t *fast_searches);
int dbaz_playout_cap_is_full(uint64_t seed, int64_t game_idx, int32_t ply, double full_prob);
/* Forced playouts and policy target pruning (Wu 2019, section 3.2) at the root of the self-play driver's full searches.
 * Scope: the rule is active in a search iff k > 0 and the search is a full search of the driver (with the playout cap off every
 * search of the driver is full).  Fast searches, explicit searches (dbaz_search*, dbaz_select) and match play never see it.
 * All arithmetic below is float64, every operation rounded on its own (no fused multiply-add), in the order written.
 *
 * Forced playouts -- in the descent of a simulation, at the root level only, for a valid child c: with
 *   n = the child's visit count as the UCB of this simulation reads it,
 *   N = the root's own visit count as this simulation reads it (the N of its sqrt(N) and log terms; it restarts at 0 with
 *       every move, tree reuse or not),
 *   P = the child's float64 root prior (noise mixed in),
 * the child is forced iff   n > 0   and   (double)n * (double)n < (k * P) * (double)N.
 * A forced child's score is the constant 1e20 in place of prior_score + value_score; the argmax is the usual first maximum,
 * so the lowest forced index is taken.  Unvisited children are never forced (the first visits go by PUCT), and below the root
 * nothing changes.
 *
 * Pruning (prune = 1) -- when the driver records the row of such a search, after the move has been chosen from the raw visits:
 * the row's visits become n' below; the move, the tree (whose kept subtree carries the raw counts on), q_value, TreeStats
 * and z are what they would have been.  With N the root's visit count after the search, pbc = log((N + base + 1) / base) +
 * cpuct and sq = sqrt(N) (the values the next simulation would read), W, n, sgn the root's child_total_value (float32),
 * child_number_visits and +1 / -1 for a child whose player to move is / is not the root's:
 *   value(c)   = ((double)W / (double)(1 + n)) * sgn
 *   expl(c, m) = (pbc * (sq / (double)(m + 1))) * P
 *   1. c* = the first valid child with the maximum visit count; it keeps its visits n*.
 *   2. U* = expl(c*, n*) + value(c*).
 *   3. every other valid child with n > 0:  f = the smallest integer >= 0 with (double)f * (double)f >= (k * P) * (double)N,
 *      lo = max(0, n - f),  n' = the smallest integer m in [lo, n] with  expl(c, m) + value(c) < U*,  n' = n if there is none;
 *      then, if n' < n and n' == 1, n' = 0.
 *   4. every other child keeps its count (an unvisited or invalid one has 0).
 * The predicate of step 3 is monotone in m.  The row's flag word gets bit 1 (ROW_FLAG_PRUNED, value 2) whenever pruning ran on
 * it, also when nothing was cut.  With prune = 0 the search is forced, the raw visits are recorded and the bit stays clear.
 *
 * dbaz_selfplay_set_forced_playouts is a setting of the handle: it holds for every later dbaz_selfplay_start (not consumed).
 * k = 0 switches the rule off (the state after dbaz_create; prune is then ignored and reads back 0).
 *   k NaN, negative or above 16; prune outside {0, 1}; a match_play handle; a handle created with selfplay_pending   -> DBAZ_EINVAL
 *     (self-play in waves would inherit the rule through the shared descent, and nothing pins forced children among in-flight
 *     visits: the combination is refused)
 *   games of an earlier dbaz_selfplay_start still being played                                                     -> DBAZ_ESTATE
 * A failed call changes nothing.
 * dbaz_get_forced_playouts: the setting, and the rows pruning ran on and the visits it took out of them (the sum of n - n')
 * since the last dbaz_selfplay_start, which zeroes both.  Any output pointer may be NULL.
 * dbaz_prune_visits: steps 1-4 on the host -- no handle, no device -- from the very code the driver runs.  n_and_sign[i] =
 * n | (sgn > 0 ? 0x40000000 : 0); valid[i] != 0 for a valid child; out[i] = n'.  k = 0 copies the counts.  n_actions outside
 * 1 .. DBAZ_MAX_A, k outside [0, 16], root_N < 0 or a NULL pointer -> DBAZ_EINVAL. */
int dbaz_selfplay_set_forced_playouts(dbaz_engine *e, double k, int32_t prune);
int dbaz_get_forced_playouts(dbaz_engine *e, double *k, int32_t *prune, int64_t *rows_pruned, int64_t *visits_pruned);
int dbaz_prune_visits(int32_t n_actions, double k, double pbc, double sq, int64_t root_N, const double *P, const float *W,
                      const uint32_t *n_and_sign, const uint8_t *valid, int32_t *out);
/* Gumbel root search (Danihelka et al., ICLR 2022, "Policy improvement by planning with Gumbel") at the root of the self-play
 * driver's searches: candidates sampled without replacement by the Gumbel-top-m trick, the read budget spent by sequential
 * halving, and softmax(logits + sigma(completed Q)) as the policy target in place of the visit counts.
 * dbaz_selfplay_set_gumbel(e, m, c_visit, c_scale) is a setting of the handle: it holds for every later dbaz_selfplay_start.
 * m = 0 switches the rule off (the state after dbaz_create; the other two arguments are then ignored and read back 0).  With the
 * rule off every row is what it was.
 * Scope: with m > 0 every search that the self-play driver starts is a Gumbel search, full and fast searches of the playout cap
 * alike (a fast search still has capped reads and its row still carries bit 0).  Explicit searches (dbaz_search*, dbaz_select)
 * never see the rule, and match play sees it only through dbaz_match_set_search (below).  Below the root nothing changes
 * (unless the full mode is on: dbaz_selfplay_set_gumbel_mode, below).
 * All arithmetic below is float64, every operation rounded on its own (no fused multiply-add), in the order written.
 *
 * Root preparation -- where the root's priors are prepared for such a search (at its start, or after the root's expansion):
 *   The root is prepared as UCT_search(..., dirichlet=(0.0, 0.0)) prepares it, like a fast search: no Dirichlet noise.
 *   P(a) = the float64 root prior that results.
 *   C = the valid children with P(a) > 0; if there are none, all valid children.  m' = min(m, |C|).
 *   logit(a) = log(P(a)) for P(a) > 0, else -1e30.
 *   g(a) = -log(-log(u)), u = u01(words 0, 1) of Philox4x32-10 with counter (lo32(game), hi32(game), ply + 65536 a, 0x44444444)
 *     and the key (lo32(seed), hi32(seed)), u clamped to [2^-53, 1 - 2^-53]; u01(a, b) = ((a >> 5) 2^26 + (b >> 6)) 2^-53.
 *     A vector scripted for this (game, ply) through dbaz_selfplay_script is taken as g as is, whatever noise_alpha is and for
 *     fast searches too.  (On a handle with m = 0 scripts mean what they mean without the rule.)  Only a scripted vector is
 *     taken: one that the host left for the slot by other means is dropped when such a search starts.
 *   Kept per slot:  gl(a) = g(a) + logit(a);  n0(a) = the child's visit count as the tree holds it at this moment (non-zero
 *     under tree reuse);  R = the reads this search was started with (after the driver rule, fast_reads, solver_reads,
 *     endgame_reads, stagger and quickplay).
 *
 * Selection at the root level of every simulation -- with n(a), W(a), sgn(a) as this simulation reads them:
 *   n_s(a) = n(a) - n0(a),  t = sum_a n_s(a).
 *   q(a) = ((double)W / (double)(1 + n)) * sgn  for n(a) > 0  (the descent's own value_score).
 *   v_mix = sum_{n>0} P(a) q(a) / sum_{n>0} P(a), or 0 if the denominator is 0.  (The paper's mixed value without the raw
 *     network value of the root: once tree reuse has made a child the root, that value is not kept anywhere.)
 *   cq(a) = q(a) for n(a) > 0, else v_mix.
 *   n_max = the maximum of n over the valid children.
 *   sigma(a) = ((c_visit + (double)n_max) * c_scale) * cq(a).
 *   cv = considered(m', R, t), below.
 *   The simulation takes the first maximum of gl(a) + sigma(a) over the candidates with n_s(a) == cv.  If no candidate has
 *   n_s == cv, the candidates with the smallest n_s compete (this cannot happen while t < R; it makes the rule total).
 * Sum order: each sum over the A children is taken in two stages.  Lane i of 64 adds its entries i, i + 64, i + 128, i + 192 in
 * that order, absent ones (and the terms of children with n = 0) as +0.0; then six butterfly stages s = s + s[lane ^ o] for
 * o = 32, 16, ..., 1.
 *
 * considered(m', R, t) -- mctx's sequence of considered visits in closed form per phase.  For m' <= 1 it is t.  Otherwise
 *   L = ceil(log2(m'));  nc = m'; base = 0; pos = 0
 *   loop:  extra = max(1, R / (L * nc))   (integer division);  len = extra * nc
 *          if t < pos + len: return base + (t - pos) / nc
 *          pos += len; base += extra; nc = max(2, nc / 2)
 * The halving is implicit: a child that is picked leaves the set n_s == cv, so each phase visits the best nc children by
 * gl + sigma `extra` times each.
 *
 * The move: a scripted move wins.  Otherwise the first maximum of gl(a) + sigma(a) over the candidates with the maximum n_s, all
 * quantities read after the search.  Temperature is not used and the move-draw stream is not consumed.
 *
 * The row: x(a) = logit(a) + sigma(a) over the candidates (without g), M = max x, e(a) = exp(x(a) - M), pi'(a) = e(a) / sum e
 * (in the sum order above).  The row's visits[a] = (int32) floor(pi'(a) * 2^24 + 0.5); every non-candidate gets 0.  The row's
 * flag word gets bit 2 (ROW_FLAG_GUMBEL, value 4).  q_value, the tree statistics and z are what they were.  Every reader of the
 * row turns visits into pi by visits / visits.sum().
 *
 *   m < 0 or m > DBAZ_MAX_A; c_visit NaN, negative or above 1e6; c_scale NaN, <= 0 or above 1e3 (both only looked at for
 *   m > 0); a match_play handle; a handle created with selfplay_pending; a handle with forced playouts on      -> DBAZ_EINVAL
 *     (dbaz_selfplay_set_forced_playouts(k > 0) refuses a handle with the Gumbel rule on in turn: both own the root's pick)
 *   games of an earlier dbaz_selfplay_start still being played                                                  -> DBAZ_ESTATE
 * A failed call changes nothing.
 * dbaz_get_gumbel: the setting, and the Gumbel searches the driver has started and the Gumbel rows written since the last
 * dbaz_selfplay_start, which zeroes both.  Any output pointer may be NULL.
 * dbaz_gumbel_considered, dbaz_gumbel_target: the rule on the host -- no handle, no device -- from the very code the kernels
 * run.  out[t] = considered(m_eff, R, t) for t < R.  dbaz_gumbel_target: the row's visits of a root given its P, W,
 * n_and_sign[i] = n | (sgn > 0 ? 0x40000000 : 0) and valid[i] != 0 for a valid child.  Arguments out of the ranges above,
 * n_actions outside 1 .. DBAZ_MAX_A or a NULL pointer -> DBAZ_EINVAL. */
int dbaz_selfplay_set_gumbel(dbaz_engine *e, int32_t m, double c_visit, double c_scale);
int dbaz_get_gumbel(dbaz_engine *e, int32_t *m, double *c_visit, double *c_scale, int64_t *searches, int64_t *rows);
int dbaz_gumbel_considered(int32_t m_eff, int32_t R, int32_t *out /*[R]*/);
int dbaz_gumbel_target(int32_t n_actions, double c_visit, double c_scale, const double *P, const float *W,
                       const uint32_t *n_and_sign, const uint8_t *valid, int32_t *out);
/* The full mode of the Gumbel search (the paper's "Full Gumbel"): the rule below the root too, and the paper's whole mixed value.
 * dbaz_selfplay_set_gumbel_mode(e, mode) is a setting of the handle like m: mode 0 (the state after dbaz_create) is the rule at the
 * root as stated above, mode 1 is full.  It is only looked at while m > 0; with m = 0 every row is what it was, and with mode 0
 * every kernel, row and counter of a Gumbel handle is what it was.
 * Same arithmetic as above: float64, every operation rounded on its own, in the order written; the sums in the sum order above.
 *
 * At an inner node s of a search of such a handle, the root included -- with the children's n(a), W(a), sgn(a), valid(a) and P(a) as
 * the simulation reads them; P(a) is the float64 root prior at the root and (double) of the child's float32 prior below it:
 *   v^(s) = (double) of the float32 value the node received when it was expanded: the network's value, a table's or the leaf
 *     solver's exact value, or the twin's on a transposition hit -- the value of the player to move at s, as the backup takes it.
 *   q(a) = ((double)W / (double)(1 + n)) * sgn  for n(a) > 0, as above.
 *   S = sum_a n(a), an integer, over the children's rows (not the root's own visit count).
 *   num = sum_{n>0} P(a) q(a),  den = sum_{n>0} P(a).
 *   v_mix = den != 0 ? (v^ + (double)S * (num / den)) / (1.0 + (double)S) : v^.
 *   cq(a) = q(a) for n(a) > 0, else v_mix.   n_max = the maximum of n over the valid children.
 *   sigma(a) = ((c_visit + (double)n_max) * c_scale) * cq(a).
 *   C(s) = the valid children with P(a) > 0; if there are none, all valid children.  logit(a) = log(P(a)) for P(a) > 0, else -1e30.
 *   x(a) = logit(a) + sigma(a) over C(s),  M = max x,  e(a) = exp(x(a) - M),  pi'(a) = e(a) / sum e.
 * Below the root the simulation takes the first maximum over C(s) of  pi'(a) - (double)n(a) / (1.0 + (double)S).  There is no pb_c,
 * no sqrt, no noise and no g: the pick is deterministic and needs neither c_puct nor the log / sqrt tables.
 * At the root, selection, the move and the row's target are exactly those stated above with this v_mix in place of the root-only
 * one; g, n0, considered() and the halving do not change.
 * Values are not rescaled to [0, 1] by the minimum and maximum of the tree, as mctx does it: q stays in [-1, 1] as in the root rule,
 * so that (c_visit, c_scale) mean the same in both modes.
 * The rows of such searches carry bit 3 of the flag word (ROW_FLAG_GUMBEL_FULL, value 8) beside bit 2.
 * A root made by tree reuse was expanded earlier in the same game under the same setting (both setters are refused while games
 * are being played), so its v^ is always there.
 *
 *   mode other than 0 or 1                                               -> DBAZ_EINVAL
 *   games of an earlier dbaz_selfplay_start still being played           -> DBAZ_ESTATE
 * A failed call changes nothing.  The refusals of dbaz_selfplay_set_gumbel are unchanged, so this call never brings the full mode
 * to match play (dbaz_match_set_search does, per model), to self-play in waves or beside forced playouts; explicit searches never
 * see the rule in either mode.
 * dbaz_get_gumbel_mode: the setting (mode may be NULL).
 * The rule on the host -- no handle, no device -- from the very code the kernels run, for one node with value v, priors P, W,
 * n_and_sign and valid as for dbaz_gumbel_target:  dbaz_gumbel_improved_policy: pi_out[i] = pi'(i), 0.0 for a non-candidate;
 * dbaz_gumbel_nonroot_pick: *out = the child a simulation takes below the root (-1 if no child is valid);
 * dbaz_gumbel_target_full: the row's visits with the full v_mix.  Argument checks: those of dbaz_gumbel_target, and a v that is NaN
 * or infinite -> DBAZ_EINVAL. */
int dbaz_selfplay_set_gumbel_mode(dbaz_engine *e, int32_t mode);
int dbaz_get_gumbel_mode(dbaz_engine *e, int32_t *mode);
int dbaz_gumbel_improved_policy(int32_t n_actions, double c_visit, double c_scale, double v, const double *P, const float *W,
                                const uint32_t *n_and_sign, const uint8_t *valid, double *pi_out);
int dbaz_gumbel_nonroot_pick(int32_t n_actions, double c_visit, double c_scale, double v, const double *P, const float *W,
                             const uint32_t *n_and_sign, const uint8_t *valid, int32_t *out);
int dbaz_gumbel_target_full(int32_t n_actions, double c_visit, double c_scale, double v, const double *P, const float *W,
                            const uint32_t *n_and_sign, const uint8_t *valid, int32_t *out);
/* The search of each model of a match.  On a match_play handle the model of a move is root.to_play XOR (game_idx & 1), as ever;
 * dbaz_match_set_search(e, model, reads, m, c_visit, c_scale, mode, g_scale) gives that model its own read budget, its own rule (PUCT
 * or Gumbel), Gumbel constants, mode and a scale on the Gumbel noise.  It is a setting of the handle for every later
 * dbaz_selfplay_start; after dbaz_create both models have (0, 0, 0, 0, 0, 0), and a handle in that state plays every row it played
 * before, bit for bit.  The other model's rows, moves and random streams are untouched by one model's setting.
 *
 * reads: 0 = the handle's mcts_num_read, as today.  Otherwise a search by this model runs min(rule, reads) reads, rule being the
 *   driver's count min(4 * nb_valid_moves!, mcts_num_read).  The cap is applied where solver_reads and endgame_reads are, and before
 *   them; R of the halving is still the reads the search was started with, after every cap.  Range 0 .. mcts_num_read: the node pool
 *   and the reserve of a re-root stay sized by mcts_num_read.  reads holds for a PUCT model (m = 0) too.
 * m = 0: this model's searches are what they are today except for the read count: Dirichlet noise, temperature, the move-draw
 *   stream, visit counts as the row.  c_visit, c_scale, mode and g_scale are then ignored and read back 0.
 * m > 0: every search by this model is a Gumbel search exactly as stated for dbaz_selfplay_set_gumbel, with this model's m, c_visit
 *   and c_scale: no Dirichlet noise, no temperature, the move-draw stream not consumed, the row's visits the target pi' in units of
 *   2^-24, flag bit 2 set (and bit 3 when mode = 1).
 * g_scale: gl(a) = (g_scale * g(a)) + logit(a) -- one product, then one sum, each rounded on its own.  Range 0 .. 1e3.  1.0 gives
 *   the bits of the self-play rule (the product is exact).  A scripted vector is scaled the same way.  0 is the paper's
 *   deterministic evaluation search: the m' candidates are the top m' by logit, the candidates that survive each halving are decided
 *   by logit + sigma alone, and the move is the argmax of logit + sigma(q) among the most visited; exact ties go to the first index
 *   as everywhere else.
 * mode: 0 = the rule at the root, 1 = full (dbaz_selfplay_set_gumbel_mode's rule), per model.  If either model is full, every node
 *   any search of the handle expands keeps its v^, whichever model expanded it, so a full search always finds the v^ of a root and
 *   of inner nodes that the other model's search made.  A root-only search on such a handle is root-only in everything: the
 *   root-only v_mix, the UCB below the root, bit 3 clear.
 * Tree reuse: n0 already covers a root that the other model's search has visited; the root prior is whatever the tree holds, the
 *   existing semantics of match play.
 *
 *   a handle without match_play; model outside {0, 1}; reads outside 0 .. mcts_num_read;
 *   m < 0 or m > DBAZ_MAX_A; for m > 0: c_visit NaN, negative or above 1e6, c_scale NaN, <= 0 or above 1e3, mode other than 0 or 1,
 *   g_scale NaN, negative or above 1e3                                                               -> DBAZ_EINVAL
 *   games of an earlier dbaz_selfplay_start still being played                                       -> DBAZ_ESTATE
 * A failed call changes nothing.  (Self-play in waves needs no refusal here: dbaz_create refuses max_pending_evals > 1, which
 * selfplay_pending requires, on a match_play handle.)
 * The row's visits of a Gumbel model are the rule's arithmetic; an implementation whose log and exp are within 1 ulp reproduces
 * them to the count wherever no decision and no rounding of pi' * 2^24 + 0.5 lies within that error of a tie.
 * dbaz_selfplay_set_gumbel goes on refusing a match handle; the playout cap and forced playouts stay refused in match play.
 * dbaz_get_gumbel's searches and rows count the Gumbel searches and rows of either model; its setting is the self-play
 * one and reads 0 on a match handle.  Explicit searches (dbaz_search*, dbaz_select) and self-play in waves still
 * never see the rule.
 * dbaz_match_get_search: the model's setting; any output pointer may be NULL.  A handle without match_play or a model outside
 * {0, 1} -> DBAZ_EINVAL. */
int dbaz_match_set_search(dbaz_engine *e, int32_t model, int32_t reads, int32_t m, double c_visit, double c_scale, int32_t mode,
                          double g_scale);
int dbaz_match_get_search(dbaz_engine *e, int32_t model, int32_t *reads, int32_t *m, double *c_visit, double *c_scale, int32_t *mode,
                          double *g_scale);
int dbaz_step(dbaz_engine *e, int32_t k);             /* k simulation steps, asynchronous */
/* until all games are finished, max_steps (if > 0) are done, or every remaining slot is
 * blocked on a full output buffer (counters.blocked_slots == active_slots: fetch and call again) */
int dbaz_run(dbaz_engine *e, int64_t max_steps);
int dbaz_get_counters(dbaz_engine *e, dbaz_counters *out);
int dbaz_timing_begin(dbaz_engine *e);
int dbaz_timing_end(dbaz_engine *e);
/* SelfPlay.get_datasets rows of finished games (self_play.py:95-156), sorted by
 * (game_idx, move_idx).  Drains the output buffer. */
int dbaz_fetch_samples(dbaz_engine *e, int32_t max_rows, int32_t *n_rows,
                       int32_t *game_idx, int16_t *move_idx, int16_t *move, int8_t *player,
                       int16_t *x /*[rows*3HW]*/, int32_t *visits /*[rows*A]*/, double *pi /*[rows*A]*/,
                       int8_t *z, int16_t *max_deepness, int32_t *tree_size, int32_t *terminal_count,
                       float *q_value, int16_t *played);
/* The flag words (the int16 at byte 26 of a packed row: bit 0 = row of a fast search, bit 1 = pruned visits, bit 2 = row of a Gumbel search, bit 3 = in the full mode) of the rows
 * dbaz_fetch_samples would hand out now, in its order.  Drains nothing: call it first.  max_rows = 0: the count alone. */
int dbaz_fetch_row_flags(dbaz_engine *e, int32_t max_rows, int32_t *n_rows, int16_t *flags);
/* device-resident replay rows for the RCCL all-gather (multi-GPU iteration end):
 * fixed-stride packed rows, see DESIGN.md "replay row".  Returns a DEVICE pointer. */
int dbaz_replay_rows_dev(dbaz_engine *e, void **rows_dev, int32_t *n_rows, int32_t *row_bytes);
/* empties the finished-row buffer without a host copy (the caller took the rows on the device) */
int dbaz_replay_rows_clear(dbaz_engine *e);

/* ---- training data path: replay rows in HBM -> dataset -> batches in HBM --------
 * Replaces utils.HDFStoreDataset's array build (utils/utils.py:61-80), torch's DataLoader gather
 * and SymmetriesGenerator (dots_boxes/dots_boxes_nn.py:11-58) of the reference's train loop
 * (nn.py:186-216).  Rows are the packed replay rows of dbaz_replay_rows_dev (this engine's, or
 * the RCCL all-gathered ones of all ranks); they never leave HBM. */
#define DBAZ_MAX_DATASETS 4
/* a handle keeps up to DBAZ_MAX_DATASETS datasets resident (train + validation of the reference's
 * loop); the dataset calls below address the selected one (default 0) */
int dbaz_dataset_select(dbaz_engine *e, int32_t which);
int dbaz_dataset_begin(dbaz_engine *e);
/* append rows sel[0..n_sel) of the packed device rows (sel = HOST int32 indices in the order
 * the reference's DataFrame would have: where-clause, training flag, df.sample; NULL = all) */
int dbaz_dataset_add_rows(dbaz_engine *e, const void *rows_dev, int64_t n_rows, int32_t row_bytes,
                          const int32_t *sel, int64_t n_sel);
/* order: dataset order as a HOST permutation of the staged rows (NULL = staging order), for
 * selections that interleave several row buffers.  pos_average != 0: merge rows with identical
 * features (groupby(x).mean(): Kahan float64 means of pi and z in dataset order; groups in
 * ascending lexicographic order of the feature columns) */
int dbaz_dataset_finish(dbaz_engine *e, int32_t pos_average, const int32_t *order, int64_t *n_out);
/* host copies of the dataset arrays (features int16 [n,3HW], policy float32 [n,A], value [n]) */
int dbaz_dataset_fetch(dbaz_engine *e, int16_t *x, float *pi, float *z);
/* one batch: rows idx[0..n) (HOST indices) under symmetry sym (0..7 = SymmetriesGenerator.IDXS)
 * into caller-owned DEVICE buffers boards float32 [n,3,H,W], pi [n,A], z [n,1]; complete on return */
int dbaz_dataset_batch(dbaz_engine *e, const int32_t *idx, int32_t n, int32_t sym, float *boards_dev,
                       float *pi_dev, float *z_dev);
/* the same QUEUED on the caller's own stream (a hipStream_t; e.g. torch's current stream) and returning at once: the indices are
 * validated on the host, nothing is synchronised.  Use this form when the output buffers come from a stream-ordered caching
 * allocator: dbaz_dataset_batch writes them from the handle's stream, i.e. possibly while work the caller has queued on the
 * buffers' previous owner is still pending. */
int dbaz_dataset_batch_on(dbaz_engine *e, const int32_t *idx, int32_t n, int32_t sym, float *boards_dev, float *pi_dev,
                          float *z_dev, void *stream);
/* SymmetriesGenerator.forward on DEVICE tensors boards [n,3,H,W] / policies [n,A] (either may be
 * NULL); out-of-place */
int dbaz_symmetry_apply(dbaz_engine *e, int32_t sym, const float *boards_in_dev, const float *pol_in_dev,
                        int64_t n, float *boards_out_dev, float *pol_out_dev);
/* host only (no handle, no GPU): src[a'] with out[a'] = in[src[a']] over the two edge planes */
int dbaz_symmetry_table(int32_t rows, int32_t cols, int32_t sym, int32_t *lut_out);

/* ---- training-mode tower: forward and backward of ResNetZero's residual blocks under model.train(True) ----
 * Replaces, inside NeuralNetWrapper.train's step (nn.py:203-221: p, v = self.model(boards); loss.backward()), the
 * ResBlock stack of ResNet.forward (nn.py:23-28,48-57) with BatchNorm2d in training mode (batch statistics, running-stat
 * update, gradient through the statistics) -- 98 % of the step's FLOPs.  bn_input, conv0, the heads, AlphaZeroLoss and
 * torch.optim.SGD stay with the caller.  All tensor arguments are DEVICE pointers; calls are asynchronous on `stream`
 * (a hipStream_t, NULL = the default stream).  One handle holds the activations of ONE forward pass for its backward. */
typedef struct dbaz_trainer dbaz_trainer;
const char *dbaz_trainer_last_error(const dbaz_trainer *t); /* t == NULL: why dbaz_trainer_create failed */
/* 1 where dbaz_trainer_create accepts a rows x cols board, 0 where it refuses it (more than 196 positions, or a long thin board
 * whose weight-gradient images exceed a workgroup's LDS); the reason: dbaz_trainer_last_error(NULL).  Host arithmetic, no device. */
int dbaz_trainer_board_supported(int32_t rows, int32_t cols);
int dbaz_trainer_create(int32_t rows, int32_t cols, int32_t channels /* 64 */, int32_t blocks, int32_t max_batch,
                        int32_t device, dbaz_trainer **out);
void dbaz_trainer_destroy(dbaz_trainer *t);
/* x / out: float32 [n][64][H][W] (torch NCHW).  conv_w[l] [64][64][3][3], conv_b[l], bn_w[l], bn_b[l], run_mean[l],
 * run_var[l] [64]: HOST arrays of DEVICE pointers, layer l = 2*block + (0: conv1/bn1, 1: conv2/bn2); run_mean / run_var
 * are updated in place (momentum 0.1, unbiased variance), NULL skips that. */
int dbaz_trainer_forward(dbaz_trainer *t, int32_t n, const float *x, const float *const *conv_w, const float *const *conv_b,
                         const float *const *bn_w, const float *const *bn_b, float *const *run_mean, float *const *run_var,
                         float *out, void *stream);
/* backward of the forward pass the handle holds: grad_out / grad_x [n][64][H][W]; parameter gradients are WRITTEN to
 * g_conv_w[l], g_conv_b[l], g_bn_w[l], g_bn_b[l] (shapes of the parameters); bn_w as in the forward call */
int dbaz_trainer_backward(dbaz_trainer *t, const float *grad_out, const float *const *bn_w, float *grad_x,
                          float *const *g_conv_w, float *const *g_conv_b, float *const *g_bn_w, float *const *g_bn_b,
                          void *stream);

/* ---- the whole network of the optimizer step: `p, v = self.model(boards)` and `loss.backward()` of
 * NeuralNetWrapper.train (nn.py:203-221) for a ResNetZero under model.train(True) -- bn_input, conv0 + bn0 (nn.py:19-21,48-50), the
 * residual tower, both heads (nn.py:74-105: conv 1x1 + bn + ReLU + fc (+ ReLU + fc1) -> log_softmax / tanh) -- on one
 * dbaz_trainer handle.  A dbaz_net_tensors holds DEVICE pointers to the parameters (or, in the backward call, to where their
 * gradients are WRITTEN), shapes as torch's; blk_* are HOST arrays [2*blocks] as in dbaz_trainer_forward.  Head channels: 16. */
typedef struct dbaz_net_tensors {
    float *bn_input_w, *bn_input_b;                                    /* [3] */
    float *conv0_w, *conv0_b;                                          /* [64][3][3][3], [64] */
    float *bn0_w, *bn0_b;                                              /* [64] */
    float *const *blk_conv_w, *const *blk_conv_b, *const *blk_bn_w, *const *blk_bn_b;
    float *ph_conv_w, *ph_conv_b, *ph_bn_w, *ph_bn_b;                  /* [16][64][1][1], [16], [16], [16] */
    float *ph_fc_w, *ph_fc_b;                                          /* [A][16*H*W], [A] */
    float *vh_conv_w, *vh_conv_b, *vh_bn_w, *vh_bn_b;
    float *vh_fc0_w, *vh_fc0_b;                                        /* [value_fc][16*H*W], [value_fc] */
    float *vh_fc1_w, *vh_fc1_b;                                        /* [1][value_fc], [1] */
} dbaz_net_tensors;
typedef struct dbaz_net_running { /* BatchNorm running statistics, updated in place (any pointer may be NULL) */
    float *bn_input_mean, *bn_input_var, *bn0_mean, *bn0_var;
    float *const *blk_mean, *const *blk_var;                           /* HOST arrays [2*blocks] or NULL */
    float *ph_mean, *ph_var, *vh_mean, *vh_var;
} dbaz_net_running;
/* x float32 [n][3][H][W] -> logp [n][n_actions] (log_softmax), v [n] (tanh).  `running` may be NULL. */
int dbaz_trainer_net_forward(dbaz_trainer *t, int32_t n, const float *x, const dbaz_net_tensors *params, const dbaz_net_running *running,
                             int32_t head_channels, int32_t n_actions, int32_t value_fc, float *logp, float *v, void *stream);
/* backward of the net_forward pass the handle holds; x and params as in that call; d_logp [n][n_actions], d_v [n] */
int dbaz_trainer_net_backward(dbaz_trainer *t, const float *x, const float *d_logp, const float *d_v, const dbaz_net_tensors *params,
                              const dbaz_net_tensors *grads, void *stream);

/* ---- training-mode BatchNorm2d (+ ReLU) on NCHW tensors of any channel count: bn_input, bn0 and the heads' bn0
 * of ResNetZero under model.train(True) (nn.py:19-21,81-83,98-100,114; torch.nn.BatchNorm2d: batch statistics, biased variance,
 * running-stat update with momentum, gradient through the statistics).  Stateless: all pointers DEVICE memory, `workspace` of
 * dbaz_bn2d_workspace_bytes(channels) bytes owned by the caller (the backward call may reuse the forward call's), asynchronous
 * on `stream`; errors: dbaz_trainer_last_error(NULL). */
int64_t dbaz_bn2d_workspace_bytes(int32_t channels);
int dbaz_bn2d_forward(const float *x /*[n][C][H*W]*/, int32_t n, int32_t channels, int32_t hw, const float *gamma, const float *beta,
                      float *run_mean, float *run_var, float eps, float momentum, int32_t relu, float *out, float *save_mean /*[C]*/,
                      float *save_invstd /*[C]*/, void *workspace, void *stream);
int dbaz_bn2d_backward(const float *dout, const float *out, const float *x, int32_t n, int32_t channels, int32_t hw, const float *gamma,
                       const float *save_mean, const float *save_invstd, int32_t relu, float *dx, float *dgamma, float *dbeta,
                       void *workspace, void *stream);

/* ---- AlphaZeroLoss and the SGD update of the optimizer step (nn.py:131-138,179,203-221) --------------------
 * Stateless, all pointers DEVICE memory, asynchronous on `stream`; errors: dbaz_trainer_last_error(NULL).
 * dbaz_az_loss: loss_v = mean((z - v)^2), loss_pi = -mean_n(sum_a pi * logp) (nn.py:133-135); loss3 = {loss_v + loss_pi,
 * loss_pi, loss_v}; d_logp [n][A] / d_v [n] (either may be NULL) receive grad_scale * d(loss_v + loss_pi)/d(.).
 * workspace: dbaz_az_loss_workspace_bytes() bytes. */
int64_t dbaz_az_loss_workspace_bytes(void);
int dbaz_az_loss(const float *logp /*[n][A]*/, const float *v /*[n]*/, const float *pi /*[n][A]*/, const float *z /*[n]*/, int32_t n,
                 int32_t n_actions, float grad_scale, float *loss3, float *d_logp, float *d_v, void *workspace, void *stream);
/* torch.optim.SGD.step (dampening 0, no nesterov) for ALL parameter tensors at once: d = g + weight_decay * p;
 * buf = momentum * buf + d; p -= lr * buf (momentum = 0: p -= lr * d, bufs may be NULL).  params / grads / bufs: HOST arrays of
 * n_tensors DEVICE pointers (float32, contiguous), numels their element counts; the pointers reach the device as kernel arguments
 * (no host -> device copy on the stream).  table_dev: n_tensors * 32 bytes of device scratch; chunk c (2048 elements) belongs to
 * tensor chunk_tensor_dev[c] at chunk index chunk_off_dev[c] within it (device arrays the caller builds once per parameter set).
 * A zero-initialised buf equals torch's first step. */
int dbaz_sgd_step(int32_t n_tensors, const void *const *params, const void *const *grads, const void *const *bufs, const int64_t *numels,
                  void *table_dev, const int32_t *chunk_tensor_dev, const int32_t *chunk_off_dev, int32_t n_chunks, float lr,
                  float momentum, float weight_decay, void *stream);

/* ---- exact solver for small boards: true values and optimal moves from a solved table -------------------
 * The reference has no counterpart.  For a board with E = 2*rows*cols + rows + cols <= 31 real edges the table int8 D[2^E]
 * lives in HBM: D[mask] = best achievable (mover's boxes) - (opponent's boxes) over the boxes still open under optimal play
 * by both sides.  Bit i of a mask is the i-th real edge in ascending order of its action index p*H*W + l*W + c (the sentinel
 * slots of the action space are not edges).  The solver needs no dbaz_engine; one handle per board size and GPU. */
typedef struct dbaz_solver dbaz_solver;
const char *dbaz_solver_last_error(const dbaz_solver *s); /* s == NULL: why dbaz_solver_create failed */
/* E > 31 or rows, cols < 1 -> DBAZ_EINVAL before the device is touched; the table is allocated by the first solve */
int dbaz_solver_create(int32_t rows, int32_t cols, int32_t device, dbaz_solver **out);
void dbaz_solver_destroy(dbaz_solver *s);
/* Retrograde analysis on the GPU; returns when the table is complete.  low_bits: 0 = default; L = a workgroup solves the
 * 2^L subcube of the low L mask bits in LDS (max(4, E - 20) <= L <= min(E, 16)); -1 = the plain kernel, one launch per
 * popcount layer of all 2^E masks (A/B partner).  Every form writes the same bytes.  A table that cannot be allocated is
 * DBAZ_EDEVICE; the handle stays usable. */
int dbaz_solver_solve(dbaz_solver *s, int32_t low_bits);
/* any pointer may be NULL.  solve_ms: HIP-event time of the last solve's kernels (-1 before); d0 = D[0], the empty board's
 * score difference for the first player (-128 before the first solve) */
int dbaz_solver_info(const dbaz_solver *s, int32_t *n_edges, int64_t *table_bytes, double *solve_ms, int32_t *d0);
/* host copy of D[first .. first + count) */
int dbaz_solver_table(dbaz_solver *s, int8_t *host_dst, int64_t first, int64_t count);
/* Scores n feature rows x int16 [n][3*H*W] as datasets and replay rows hold them (get_features, dots_boxes_game.py:96-100:
 * planes 0, 1 = edges, plane 2 = the mover's doubled boxes_to_close); pi float32 [n][A] may be NULL (then policy_mass too).
 * All DEVICE pointers, QUEUED on the caller's stream (a hipStream_t) like dbaz_dataset_batch_on.
 *   value [n]        true result for the mover under optimal play: sign(margin + D[mask]), margin = mover's - opponent's boxes
 *   diff  [n]        D[mask]
 *   q     [n][A]     c + D[next] / -D[next] of every legal action; -128 for drawn edges and sentinel slots
 *   policy_mass [n]  sum of pi[a], ascending a in float32, over the legal a with sign(margin + q[a]) == value
 * A finished game (early end included) gets value = get_result, q all -128 and policy_mass 0. */
int dbaz_solver_score(dbaz_solver *s, int32_t n, const int16_t *x_dev, const float *pi_dev, int8_t *value_dev, int8_t *diff_dev,
                      int8_t *q_dev, float *policy_mass_dev, void *stream);

/* The table as a policy/value evaluator: for n feature rows (as above) a ONE-HOT policy p float32 [n][A] on an optimal move
 * and v float32 [n] = sign(margin + D[mask]), the true result for the mover.  Among the n_opt moves whose q is the maximum the
 * pick is the k-th in ascending action order: k = 0 for pick_seed = 0, otherwise k = mix(mask, pick_seed) mod n_opt with the
 * splitmix64 finaliser  x = mask ^ pick_seed * 0x9E3779B97F4A7C15;  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
 * x *= 0x94D049BB133111EB; x ^= x >> 31  (64-bit, wrapping) -- a pure function of position and seed.  A finished game gets
 * p = 0 and v = get_result.  DEVICE pointers, QUEUED on the caller's stream like dbaz_solver_score; DBAZ_ESTATE before a solve. */
int dbaz_perfect_policy(dbaz_solver *s, int32_t n, const int16_t *x_dev, uint64_t pick_seed, float *p_dev /*[n][A]*/, float *v_dev,
                       void *stream);
/* The same evaluator behind the engine's evaluator boundary: model (0, or 1 = dbaz_config.evaluator2 in match play) of a handle
 * created with DBAZ_EVAL_SOLVER for that model answers its leaves from s's table -- searches, self-play and match play against a
 * network or formula evaluator run unchanged, with perfect priors and values.  The engine BORROWS the table: s must outlive the
 * engine's use of it, dbaz_destroy does not free it.  The transposition cache and the full-rounds cut stay off for this kind.
 * solver_reads > 0: searches served by this model under the driver's rule (num_reads == NULL, self-play) run
 * min(rule, solver_reads) reads -- one read already finds the move; 0 = the rule; explicit num_reads are never touched.
 *   s not solved                                              -> DBAZ_ESTATE
 *   s of another board size or device, model not 0 / 1, the model's evaluator not DBAZ_EVAL_SOLVER, solver_reads < 0
 *                                                             -> DBAZ_EINVAL
 * dbaz_search / dbaz_search_timed / dbaz_selfplay_start before the attach -> DBAZ_ESTATE. */
int dbaz_attach_solver(dbaz_engine *e, int32_t model, dbaz_solver *s, uint64_t pick_seed, int32_t solver_reads);

/* ---- exact endgame solver for any board: true values of positions with few free edges ---------------------
 * The reference has no counterpart.  D of the solver above depends only on which edges are still free, so a position with F free
 * edges on ANY board with A <= DBAZ_MAX_A is a game over the 2^F subsets of those edges; for F <= max_free <= 16 one workgroup
 * solves it in LDS.  No table, no solve step, no dbaz_engine; one handle per board size and GPU. */
typedef struct dbaz_endgame dbaz_endgame;
const char *dbaz_endgame_last_error(const dbaz_endgame *g); /* g == NULL: why dbaz_endgame_create failed */
/* max_free: 0 = 16.  rows, cols < 1, A > DBAZ_MAX_A or max_free outside 0 .. 16 -> DBAZ_EINVAL before the device is touched */
int dbaz_endgame_create(int32_t rows, int32_t cols, int32_t device, int32_t max_free, dbaz_endgame **out);
void dbaz_endgame_destroy(dbaz_endgame *g);
/* Scores n feature rows (x, pi as for dbaz_solver_score); DEVICE pointers, QUEUED on the caller's stream; the grid is n.
 *   n_free [n]       F, the number of free real edges of the row
 *   value, diff, q, policy_mass as dbaz_solver_score writes them, diff = D[0] of the subgame (the same number as the table's
 *   D[mask]); a finished game (early end included) gets value = get_result, q all -128 and policy_mass 0.
 * A row with F > max_free is NOT solved: value 0, diff -128, q all -128, policy_mass 0.  pi_dev == NULL: mass_dev is not written.
 * n == 0 is a no-op. */
int dbaz_endgame_score(dbaz_endgame *g, int32_t n, const int16_t *x_dev, const float *pi_dev, int8_t *value_dev, int8_t *diff_dev,
                       int8_t *q_dev /*[n][A]*/, float *mass_dev, int16_t *n_free_dev, void *stream);
/* The endgame solver as a policy/value evaluator, the counterpart of dbaz_perfect_policy on any board: every row is solved from
 * scratch (the solve of dbaz_endgame_score), then p float32 [n][A] is ONE-HOT on an optimal move and v float32 [n] =
 * sign(margin + D[0]).  Among the n_opt moves whose q is the maximum the pick is the k-th in ascending action order: k = 0 for
 * pick_seed = 0, otherwise k = mix(key, pick_seed) mod n_opt with dbaz_perfect_policy's finaliser and key = the XOR over the
 * row's free real edges a of 1 << (a & 63) (64-bit) -- a function of the position alone, so every path to a position picks the
 * same move.  With pick_seed = 0 the outputs equal dbaz_perfect_policy's wherever both apply.
 *   solved [n]       1, or 0 for a row with F > max_free, which gets p = 0 and v = 0
 * A finished game (early end included) with F <= max_free gets p = 0, v = get_result and solved = 1.
 * DEVICE pointers, QUEUED on the caller's stream; the grid is n; n == 0 is a no-op.  (Not named dbaz_endgame_*: that family is
 * the scorer's and stays as it is.) */
int dbaz_exact_policy(dbaz_endgame *g, int32_t n, const int16_t *x_dev, uint64_t pick_seed, float *p_dev /*[n][A]*/, float *v_dev,
                      uint8_t *solved_dev, void *stream);
/* The same (p, v) through the TABLE path the search uses (below), on its own: root i's subgame is solved once into a scratch table
 * (k_endgame_table), then the rows x[i * per_root .. (i + 1) * per_root) int16 -- positions that draw further edges of root i, the
 * root itself included; the caller's duty, another row gets a meaningless but harmless answer -- are answered from it by lookup
 * (k_endgame_eval).  p [n_roots * per_root][A], v [n_roots * per_root] equal dbaz_exact_policy's on those rows bit for bit; the
 * rows of a root with F > max_free get p = 0, v = 0.  ms_out (host, may be NULL): HIP-event milliseconds of the table kernel [0]
 * and of the lookup kernel [1].  DEVICE pointers; queued on the caller's stream, but the call allocates n_roots x max(16,
 * 2^max_free) bytes of scratch and returns only when the kernels are done (DBAZ_EDEVICE when the scratch cannot be had). */
int dbaz_exact_policy_from(dbaz_endgame *g, int32_t n_roots, const int16_t *roots_dev, int32_t per_root, const int16_t *x_dev,
                           uint64_t pick_seed, float *p_dev, float *v_dev, float *ms_out /*[2]*/, void *stream);
/* Exact training targets: the solved result and the result-preserving moves written over the z and pi of late rows.
 * One row: x int16 [3*H*W], pi float32 [A], z float32.  F = its free real edges; margin, the finished-game test, D and q[a] as
 * dbaz_endgame_score has them.  The row is left untouched, bit for bit, if F > max_free or the game is over (early end included).
 * Otherwise v = sign(margin + D[0]) and O = { free real edges a : sign(margin + q[a]) == v }, never empty, and
 *   z_mode 1: z = (float)v                          z_mode 0: z stays
 *   pi_mode 0: pi stays
 *   pi_mode 1 (uniform): pi[a] = 1.0f / |O| on O and 0.0f in every other of the A slots
 *   pi_mode 2 (restrict): S = the float32 sum of pi[a] over O in ascending a (dbaz_endgame_score's policy_mass);
 *                         S > 0: pi[a] = pi[a] / S on O and 0.0f elsewhere; otherwise the uniform form
 * Side outputs per row, each pointer may be NULL: n_free = F (every row); mass = S before the relabel (0 for an untouched row
 * and without pi_dev); relabelled = 1 for a row the rule applies to, whatever the modes.
 * Dense rows, DEVICE pointers, QUEUED on the caller's stream; the list of rows to solve and its counters are scratch of the
 * handle that grows on demand, so one call at a time per handle.  n == 0 is a no-op.
 *   a mode out of range, pi_mode != 0 with pi_dev == NULL, z_mode != 0 with z_dev == NULL -> DBAZ_EINVAL
 * (Not named dbaz_endgame_*, like dbaz_exact_policy.) */
int dbaz_exact_targets(dbaz_endgame *g, int32_t n, const int16_t *x_dev, int32_t pi_mode, int32_t z_mode, float *pi_dev /*in/out [n][A]*/,
                       float *z_dev /*in/out [n]*/, int16_t *n_free_dev, float *mass_dev, uint8_t *relabelled_dev, void *stream);
/* The same rule over the selected resident dataset (dbaz_dataset_select / dbaz_dataset_finish), in place, on the handle's stream;
 * returns when done.  Later dbaz_dataset_fetch / dbaz_dataset_batch calls read the relabelled arrays; with pos_average the merged
 * rows are relabelled (the targets are a function of the features alone).  stats_host (may be NULL) int64 [4 + 17]: rows in the
 * dataset, rows relabelled, rows with F <= max_free left alone because the game was over, relabelled rows whose z before
 * differed from v, then the relabelled rows per F = 0 .. 16.
 *   no finished dataset in the slot -> DBAZ_ESTATE;  g of another board size or device, a mode out of range -> DBAZ_EINVAL */
int dbaz_dataset_exact_targets(dbaz_engine *e, dbaz_endgame *g, int32_t pi_mode, int32_t z_mode, int64_t *stats_host);
/* The endgame solver inside the search: once a search ROOT of a slot has F0 <= max_free free edges, every later
 * position of that game is a subset of those edges.  The engine solves the root's subgame once, keeps the 2^F0-byte table in the
 * slot's region in HBM (n_slots x max(16, 2^max_free) bytes, allocated by the first attach: 8 192 slots x 64 KB = 512 MiB) and
 * answers every later leaf of that game -- this search's and those of the game's later moves -- by lookup with dbaz_exact_policy's
 * (p, v), bit for bit.  Such a leaf never reaches the model's own evaluator, network or formula: it is not on the evaluation lists,
 * not counted in or deferred by the full-rounds cut, skips the transposition probe and is not counted in dbaz_counters.nn_evals.
 * Every other leaf is handled as without the attach; in particular a leaf with F <= max_free under a root with F > max_free still
 * goes to the model's evaluator (the table is rooted at search roots only; dbaz_attach_leaf_solver below solves such leaves).  A table is valid for the slot's current game only.
 * model: 0, or 1 = the second model in match play.  The engine BORROWS g: it must outlive the engine's use of it.
 * endgame_reads > 0: a search under the driver's rule (num_reads == NULL, self-play) whose root has F <= max_free runs
 * min(rule, endgame_reads) reads; 0 = the rule; explicit num_reads are never touched.
 * With reuse_tree = 0 and no noise a game ends with the theoretical result of the first root that had a table, from that move on
 * (4.6's one-hot argument with its fresh-root condition); with tree reuse or noise only the served leaves' (p, v) are exact.
 *   the model's evaluator DBAZ_EVAL_EXTERNAL or DBAZ_EVAL_SOLVER, model not 0 / 1 (1 without match play), g of another board size
 *   or device, endgame_reads < 0                                  -> DBAZ_EINVAL
 *   a max_free other than that of the handle's FIRST attach (either model; the slot regions are sized once) -> DBAZ_EINVAL
 *   a handle whose slot tables belong to a dbaz_tables (dbaz_attach_tables below: one kind of attach per handle) -> DBAZ_EINVAL
 * A later attach with the same max_free replaces the model's solver, seed and endgame_reads and drops every slot's table.
 *   the slot tables cannot be allocated                           -> DBAZ_EDEVICE; the engine stays usable without the attach */
int dbaz_attach_endgame(dbaz_engine *e, int32_t model, dbaz_endgame *g, uint64_t pick_seed, int32_t endgame_reads);
/* cumulative since the first attach: tables solved (one per game and model side that reaches F <= max_free), leaves answered from
 * them; waits for the engine's queued work.  Either pointer may be NULL.  (Not named dbaz_endgame_*, like dbaz_exact_policy.) */
void dbaz_get_endgame_stats(const dbaz_engine *e, int64_t *tables_solved, int64_t *leaves_served);

/* ---- deep endgames: one solved table per position, up to 31 free edges, on any board ---------------------------
 * The reference has no counterpart.  A position with F free edges is a game over the 2^F subsets of those edges, and every
 * position that can follow it is an entry of the same table.  The handle solves ONE root position into int8 T[2^F] in HBM with the
 * small-board solver's kernels (compact edge j = the root's j-th free real edge in ascending action order; bit j of an index =
 * that edge has been drawn since) and answers feature rows from it.  A row is SERVED when its free real edges are a subset of the
 * root's: the root, and every position reached from it.  One table per handle; no dbaz_engine. */
typedef struct dbaz_deep dbaz_deep;
const char *dbaz_deep_last_error(const dbaz_deep *d); /* d == NULL: why dbaz_deep_create failed */
/* max_free: 1 .. 31, 0 = 24 (16 MiB).  rows, cols < 1, A > DBAZ_MAX_A or max_free outside 0 .. 31 -> DBAZ_EINVAL before the device
 * is touched; the table of 2^max_free bytes is allocated by the first solve and reused by every later one */
int dbaz_deep_create(int32_t rows, int32_t cols, int32_t device, int32_t max_free, dbaz_deep **out);
void dbaz_deep_destroy(dbaz_deep *d);
/* Solves the subgame of root_row, a HOST feature row int16 [3*H*W] (planes 0, 1: edges; sentinel slots are never edges), into
 * the first 2^F bytes of the table; returns when it is complete.  It replaces the previous root's table, after the
 * dbaz_deep_score / dbaz_deep_policy calls queued so far have read it.  low_bits as for dbaz_solver_solve with E = F (0 = default,
 * -1 = the plain kernel; F < 4 always takes the plain kernel); every form writes the same bytes.  The work lists of the subcube
 * kernel depend on (F, low_bits) only and stay on the handle between solves.
 *   F > max_free, low_bits out of range -> DBAZ_EINVAL;  a table that cannot be allocated -> DBAZ_EDEVICE.  After either the
 *   handle has no valid table (DBAZ_ESTATE from the calls below) and stays usable: the next solve starts afresh. */
int dbaz_deep_solve(dbaz_deep *d, const int16_t *root_row_host, int32_t low_bits);
/* any pointer may be NULL.  n_free: F of the solved root (-1 without a valid table); table_bytes = 2^max_free; solve_ms: HIP-event
 * time of the last solve's kernels (-1 before); d0 = T[0], the root's score difference for its mover (-128 without a table) */
int dbaz_deep_info(const dbaz_deep *d, int32_t *n_free, int64_t *table_bytes, double *solve_ms, int32_t *d0);
/* host copy of T[first .. first + count) of the 2^F entries */
int dbaz_deep_table(dbaz_deep *d, int8_t *host_dst, int64_t first, int64_t count);
/* dbaz_endgame_score's outputs from the table: n feature rows (x, pi as for dbaz_solver_score), DEVICE pointers, QUEUED on the
 * caller's stream, one wavefront per row.
 *   n_free [n]       the row's own number of free real edges, served or not
 *   served [n]       1 when the row's free real edges are a subset of the root's, else 0
 * A served row: diff = T[mask], value = sign(margin + diff), q[a] of every free edge (-128 for drawn edges and sentinel slots),
 * policy_mass summed in ascending a in float32 -- bit for bit what dbaz_endgame_score writes where it solves the row.  A finished
 * game (early end included) gets value = get_result, q all -128 and policy_mass 0.  A row that is not served: value 0, diff -128,
 * q all -128, policy_mass 0.  pi_dev == NULL: mass_dev is not written.  n == 0 is a no-op; DBAZ_ESTATE without a valid table. */
int dbaz_deep_score(dbaz_deep *d, int32_t n, const int16_t *x_dev, const float *pi_dev, int8_t *value_dev, int8_t *diff_dev,
                    int8_t *q_dev /*[n][A]*/, float *mass_dev, int16_t *n_free_dev, uint8_t *served_dev, void *stream);
/* dbaz_exact_policy's outputs from the table: p float32 [n][A] ONE-HOT on the k-th optimal move in ascending action order with
 * dbaz_exact_policy's k (pick_seed and the position's key), v float32 [n] the true result for the mover; the same pick as
 * dbaz_exact_policy and dbaz_perfect_policy wherever they apply.  A finished game: p = 0, v = get_result, served = 1; a row that
 * is not served: p = 0, v = 0, served = 0.  DEVICE pointers, QUEUED on the caller's stream; DBAZ_ESTATE without a valid table. */
int dbaz_deep_policy(dbaz_deep *d, int32_t n, const int16_t *x_dev, uint64_t pick_seed, float *p_dev /*[n][A]*/, float *v_dev,
                     uint8_t *served_dev, void *stream);

/* ---- deep endgames in batches: a pool of tables, many roots solved side by side ----------------------------------
 * The reference has no counterpart.  dbaz_deep above holds one table; this handle owns a pool of n_tables slots of 2^max_free
 * bytes each.  One solve takes up to n_tables root positions and solves root i into slot i, the roots of equal F sharing their
 * launches; rows of many games are then answered in one launch, row r from the table table_dev[r] names -- the root's index in
 * the last solve.  Tables, served rule and outputs are dbaz_deep's, bit for bit.  No dbaz_engine. */
typedef struct dbaz_tables dbaz_tables;
const char *dbaz_tables_last_error(const dbaz_tables *t); /* t == NULL: why dbaz_tables_create failed */
/* max_free: 1 .. 31, 0 = 24 (16 MiB per table).  n_tables: 1 .. 65535, 0 = 64 (1 GiB at the default max_free).  rows, cols < 1,
 * A > DBAZ_MAX_A, max_free or n_tables out of range -> DBAZ_EINVAL before the device is touched; the pool of
 * n_tables * 2^max_free bytes is allocated by the first solve and reused by every later one */
int dbaz_tables_create(int32_t rows, int32_t cols, int32_t device, int32_t max_free, int32_t n_tables, dbaz_tables **out);
void dbaz_tables_destroy(dbaz_tables *t);
/* Solves the subgames of n_roots HOST feature rows int16 [n_roots][3*H*W], root i into the first 2^F_i bytes of slot i; returns
 * when every table is complete.  It replaces all tables of the previous solve, after the dbaz_tables_score / dbaz_tables_targets
 * calls queued so far have read them.  low_bits as for dbaz_deep_solve, applied to every root (0 = each root's default, -1 = the
 * plain kernel; F < 4 always takes the plain kernel); every form writes the same bytes.  The work lists of the subcube kernel are
 * kept per (F, low_bits) on the handle.
 *   n_roots < 1 or > n_tables, a root with F > max_free, low_bits out of range for a root's F (the message names the root)
 *                                        -> DBAZ_EINVAL;  a pool that cannot be allocated -> DBAZ_EDEVICE.
 *   After either the handle has no valid table (n_solved = 0, DBAZ_ESTATE from the calls below) and stays usable. */
int dbaz_tables_solve(dbaz_tables *t, int32_t n_roots, const int16_t *roots_host /*int16 [n_roots][3*H*W]*/, int32_t low_bits);
/* any pointer may be NULL.  n_solved: roots of the last successful solve (0 without one); table_bytes = 2^max_free; pool_bytes =
 * n_tables * 2^max_free; solve_ms: HIP-event time of the last solve's kernels, all roots together (-1 before) */
int dbaz_tables_info(const dbaz_tables *t, int32_t *n_solved, int64_t *table_bytes, int64_t *pool_bytes, double *solve_ms);
/* per solved root i < n_solved, HOST arrays (either may be NULL): its free edges F_i, and d0 = T_i[0], its score difference */
int dbaz_tables_roots(const dbaz_tables *t, int32_t *n_free_out /*int32 [n_solved]*/, int32_t *d0_out /*int32 [n_solved]*/);
/* host copy of T_i[first .. first + count) of root i's 2^F_i entries */
int dbaz_tables_table(dbaz_tables *t, int32_t i, int8_t *host_dst, int64_t first, int64_t count);
/* dbaz_deep_score for rows of many games: table_dev int32 [n] names the table of each row.  A row is SERVED when table_dev[r] is
 * in [0, n_solved) and the row's free real edges are a subset of that root's; its outputs are bit for bit those of
 * dbaz_deep_score with that root's table.  Every other row -- an index outside [0, n_solved) is never used to form an address --
 * gets value 0, diff -128, q all -128, policy_mass 0, served 0; n_free is the row's own count either way.  DEVICE pointers,
 * QUEUED on the caller's stream; n == 0 is a no-op; DBAZ_ESTATE without a valid solve. */
int dbaz_tables_score(dbaz_tables *t, int32_t n, const int16_t *x_dev, const float *pi_dev, const int32_t *table_dev /*int32 [n]*/,
                      int8_t *value_dev, int8_t *diff_dev, int8_t *q_dev /*[n][A]*/, float *mass_dev, int16_t *n_free_dev,
                      uint8_t *served_dev, void *stream);
/* dbaz_exact_targets' rule, in place, with v and q from the row's table instead of a solve from scratch: a row that is not served
 * (as above) or belongs to a finished game is left untouched, bit for bit; every other row is relabelled as dbaz_exact_targets
 * relabels a row it solves -- the same O, the same float32 sum S in ascending a, one correctly rounded float32 division per
 * entry -- so the two agree bit for bit wherever both apply.  Modes, side outputs (each may be NULL; n_free of every row, mass and
 * relabelled 0 for an untouched row) and argument checks as for dbaz_exact_targets.  DEVICE pointers, QUEUED on the caller's
 * stream; DBAZ_ESTATE without a valid solve. */
int dbaz_tables_targets(dbaz_tables *t, int32_t n, const int16_t *x_dev, const int32_t *table_dev /*int32 [n]*/, int32_t pi_mode,
                        int32_t z_mode, float *pi_dev /*in/out [n][A]*/, float *z_dev /*in/out [n]*/, int16_t *n_free_dev,
                        float *mass_dev, uint8_t *relabelled_dev, void *stream);

/* ---- deep exact targets on packed replay rows: one table per game, rows relabelled where they lie -----------------
 * The reference has no counterpart.  rows_dev: n_rows packed replay rows (RowMeta | x int16[3*H*W] | visits int32[A], row_bytes
 * apart and 8-byte aligned: what dbaz_replay_rows_dev hands out) on t's DEVICE, in any order.  A GAME is the rows of one game_idx;
 * its ROOT is its first row by move_idx with at most max_free free real edges (none: the game's rows come back byte for byte).
 * The root and every later row of the game are CANDIDATES.  The roots are solved through t's pool n_tables at a time, in the
 * order (F descending, game_idx ascending), the geometries built on the device from the root rows; per candidate, in place:
 *   its free real edges are no subset of its root's (dbaz_tables_score's served rule)  -> untouched, counted `unserved`
 *   its game is over (early end included)                                             -> untouched, counted `finished`
 *   otherwise RELABELLED: v = sign(margin + T[mask]), O = the free edges a with sign(margin + q[a]) == v, dbaz_tables_targets' set;
 *     z_mode 1: RowMeta.z <- v;  pi_mode 2 (restrict): visits[a] <- 0 for every a outside O, sentinel slots included, and 1 on O
 *     if the visits on O sum to 0;  pi_mode 1 (uniform): 1 on O, 0 elsewhere;  pi_mode 0: visits as they are.  Integers only.
 * No other byte of any row changes.  The handle's stream waits for `stream`; the call returns when the rows are final.
 * root_of_dev (may be NULL): int32 [n_rows] on the device, per row the row index of its game's root if the row is a candidate, else -1.
 * stats_host (may be NULL): int64 [8 + 32 + 5] = rows, games, roots (tables solved), chunks, relabelled, finished, unserved,
 *   z_changed (relabelled rows whose z was not v, whatever z_mode says); by_free[32]: relabelled rows by their own free edges;
 *   nanoseconds of HIP-event time of the call's kernels: scan, sort + segment pass, geometry, solve, relabel.
 * Afterwards t holds the LAST chunk's tables as after a dbaz_tables_solve of those roots (n_solved = 0 if no game has a root,
 * and after any failure past the argument checks); solve_ms of dbaz_tables_info is then the solve time of all chunks together.
 * One call at a time per handle; its scratch stays on the handle.
 *   pi_mode / z_mode out of range, row_bytes not the board's, rows_dev NULL with n_rows > 0, misaligned rows, n_rows < 0
 *                                      -> DBAZ_EINVAL before the device is touched;  n_rows == 0: DBAZ_OK, zero stats
 *   two rows with the same (game_idx, move_idx) -> DBAZ_EINVAL, found on the device before any row is written
 *   (Not named dbaz_tables_*: that family is the pool's own.) */
int dbaz_replay_exact_targets(dbaz_tables *t, void *rows_dev, int64_t n_rows, int32_t row_bytes, int32_t pi_mode, int32_t z_mode,
                              int32_t *root_of_dev /*int32 [n_rows]*/, int64_t *stats_host /*int64 [45]*/, void *stream);

/* ---- deep tables inside the search: dbaz_attach_endgame's meaning for up to 31 free edges ------------------------
 * The counterpart of dbaz_attach_endgame with a dbaz_tables: once a search root of a slot has F0 <= max_free free edges, the
 * engine solves that root's subgame once per game into the slot's region in HBM and answers every later leaf and root of the game
 * from it, exactly as described there -- the same (p, v), bit for bit, the same routing, counters and endgame_reads.  t supplies
 * the board and max_free; its own pool is not touched and need not be allocated, and the engine keeps nothing of t's on the device
 * (the work lists of every F <= max_free are built into the engine's own memory at the first attach), so a handle that a later
 * attach has replaced may be destroyed.  The
 * engine allocates n_slots << max_free bytes of slot tables (64-bit sizes: 8 192 slots x 1 MiB = 8 GiB at max_free = 20), a region
 * of 2^max_free bytes per slot whatever a root's F, plus headers, requests and the list of roots of a pass.  The tables are solved
 * on the device from requests that exist only there: every pass over the slots is one fixed launch sequence, a function of
 * max_free alone, and no request waits for a later pass, however many arrive at once.  The engine BORROWS t.
 *   the refusals of dbaz_attach_endgame (evaluator, model, board or device, endgame_reads < 0)          -> DBAZ_EINVAL
 *   a handle's attaches are all of ONE kind and one max_free: a dbaz_tables after a dbaz_endgame, a dbaz_endgame after a
 *   dbaz_tables, or another max_free than the first dbaz_attach_tables   -> DBAZ_EINVAL, nothing changes
 *   the slot tables cannot be allocated   -> DBAZ_EDEVICE, the byte count in the message; the handle stays as it was
 * A later attach with the same max_free replaces the model's handle, seed and endgame_reads and drops every slot's table.
 * dbaz_get_endgame_stats counts these tables and leaves too. */
int dbaz_attach_tables(dbaz_engine *e, int32_t model, dbaz_tables *t, uint64_t pick_seed, int32_t endgame_reads);
/* A slot's table as the search sees it, after waiting for the engine's queued work; for either kind of attach.  valid: the slot
 * has a table (of game `game`, n_free = F0 free edges at its root, free_edges [4] = those edges by action index; compact edge j is
 * the j-th of them, bit j of a table index = that edge has been drawn since).  host_dst (may be NULL with count = 0) receives
 * bytes [first, first + count) of the slot's region, whose first 2^F0 bytes are the table.  Any output pointer may be NULL.
 *   no attach on this handle, slot outside 0 .. n_slots - 1, a range outside the slot's region -> DBAZ_EINVAL */
int dbaz_get_slot_table(dbaz_engine *e, int32_t slot, int32_t *valid, int32_t *n_free, int64_t *game, uint64_t free_edges[4],
                        int8_t *host_dst, int64_t first, int64_t count);

/* ---- deep tables from a pool that the slots share ----------------------------------------------------------------
 * dbaz_attach_tables with n_tables regions of 2^max_free bytes instead of one per slot: n_tables << max_free bytes (64-bit sizes),
 * 1 <= n_tables <= n_slots.  A slot needs a table only while its game is in its last max_free moves; a region is handed to the slot
 * on the device when its search root first has F0 <= max_free free edges and goes back to the pool when the slot's game ends,
 * whether or not the slot starts another.  Every pass runs where dbaz_attach_tables' passes run, and still no request waits for a
 * later pass:
 *   - all regions given back in a pass (a game that ended, a root past max_free) are free before any is granted in that pass;
 *   - the slots that ask are granted in ASCENDING SLOT ORDER as long as free regions last; which region a slot receives is
 *     unspecified and changes no result;
 *   - a slot that asks and gets nothing is DENIED: it has no table, the leaves of THIS search go to the model's own evaluator, and
 *     the slot asks again when its next search starts.  Denials are counted (dbaz_get_table_pool) and change results, as
 *     dbaz_counters.pool_resets do: two runs of one configuration give the same rows and counters, but runs with different slot
 *     counts may differ once something is denied.  With no denial the rows are those of dbaz_attach_tables, bit for bit.
 * dbaz_set_positions, dbaz_selfplay_start and a later attach free every region.  Both models of a match draw on the one pool.
 *   every refusal of dbaz_attach_tables; n_tables outside 1 .. n_slots; endgame_reads > 0 (the reads of a search are capped before
 *   the pass knows whether the slot gets a region); a pooled attach on a handle with one region per slot or the reverse; another
 *   n_tables than the first pooled attach                                  -> DBAZ_EINVAL, nothing changes
 *   the regions cannot be allocated   -> DBAZ_EDEVICE, the byte count in the message; the handle stays as it was */
int dbaz_attach_tables_pool(dbaz_engine *e, int32_t model, dbaz_tables *t, int32_t n_tables, uint64_t pick_seed, int32_t endgame_reads);
/* The pool's figures after waiting for the engine's queued work: its regions (0: no pooled attach on this handle, and the other
 * figures are 0), the regions held now, the most held at once and the denials, the last two counted since the first attach.  Any
 * output pointer may be NULL. */
int dbaz_get_table_pool(dbaz_engine *e, int32_t *n_tables, int32_t *in_use, int32_t *high_water, int64_t *denied);
/* The region that a slot's header names, after waiting for the queued work: the slot's own index for dbaz_attach_endgame and
 * dbaz_attach_tables, a region of the pool or -1 (the slot holds none) for dbaz_attach_tables_pool.  dbaz_get_slot_table reads the
 * bytes of that region; with count > 0 for a slot that holds none it is DBAZ_EINVAL.
 *   no attach on this handle, slot outside 0 .. n_slots - 1 -> DBAZ_EINVAL */
int dbaz_get_slot_table_index(dbaz_engine *e, int32_t slot, int32_t *table);

/* ---- the pool in WAIT MODE: a slot that finds the pool dry waits for a region --------------------------------------
 * dbaz_attach_tables_pool, except that no search is ever denied, so that the rows no longer depend on the slot count, the pool
 * size or the schedule: for every n_tables >= 1 they are the rows of dbaz_attach_tables, bit for bit.  endgame_reads means what
 * it means for dbaz_attach_tables (every search under a root with F <= max_free free edges has a table, so the cap is right).
 * The rule:
 *   - the requests of a pass are handled as in dbaz_attach_tables_pool: all regions given back in the pass are free first, then
 *     the slots that ask take the free regions in ASCENDING SLOT ORDER as long as they last;
 *   - a slot that asks and gets nothing keeps its request standing and is WAITING: it selects no leaf and evaluates nothing, it
 *     consumes none of its reads, and its tree stays as the start of its search left it;
 *   - every later pass ranks the waiting slots together with that pass's new askers, by slot index, under the same rule.  (Any
 *     work-conserving order gives the same rows and the same number of regions held at every pass -- a slot's rows are a function
 *     of (seed, game, ply) alone, and a free region never stays free while a slot asks; ascending slot order is the order the
 *     deny mode already has.  It is no FIFO: a low slot that asks late overtakes a high slot that has waited.)
 *   - the pass that grants a waiting slot a region solves its table in that pass, and the slot's search proceeds as if it had
 *     started then; in the one-simulation step, where the pass runs next to the step's selection, the slot takes its first
 *     selection in the following step;
 *   - `denied` (dbaz_get_table_pool) stays 0; the slot-passes spent waiting are counted instead (dbaz_get_table_pool_waits).
 * A wait ends: regions come back whenever a holder's game ends, and a holder never waits.  A waiting slot is an active slot
 * (dbaz_counters.active_slots), never a blocked one.  dbaz_set_positions, dbaz_selfplay_start and a later attach clear every
 * wait along with the regions.
 * Scope: the self-play driver only (dbaz_run, dbaz_step; one simulation per step and selfplay_pending waves alike, match play
 * included).  Nothing gives a region back during an explicit search, so on a handle in wait mode dbaz_search, dbaz_search_timed,
 * dbaz_search_begin and dbaz_select return DBAZ_ESTATE.
 *   every refusal of dbaz_attach_tables_pool except endgame_reads > 0 (endgame_reads < 0 is refused); a handle's pooled attaches
 *   are all of ONE mode: a wait attach on a handle whose pool denies, or the reverse   -> DBAZ_EINVAL, nothing changes */
int dbaz_attach_tables_pool_wait(dbaz_engine *e, int32_t model, dbaz_tables *t, int32_t n_tables, uint64_t pick_seed, int32_t endgame_reads);
/* After waiting for the engine's queued work: wait_mode (1: the handle's pool is in wait mode), the slots waiting now, and the
 * slot-passes spent waiting -- what `denied` would have counted -- cumulative since the first attach.  All 0 without a pooled
 * attach.  Any output pointer may be NULL. */
int dbaz_get_table_pool_waits(dbaz_engine *e, int32_t *wait_mode, int32_t *waiting, int64_t *waited);

/* ---- exact endgames at the LEAVES: a leaf with few free edges is solved from scratch ------------------------------
 * The attaches above answer leaves from a table rooted at a search root; this one needs no root and no HBM.  With a leaf solver
 * attached to the searching model with threshold L (1 <= L <= g's max_free <= 16), a non-terminal leaf -- the root expansion of a
 * search counts as a leaf -- is treated as follows:
 *   - the slot's table serves the game (any attach above): the leaf is answered from the table, as without this attach -- the
 *     table wins because it is a lookup;
 *   - otherwise, the leaf's own number of free real edges is F <= L: the leaf is SOLVED from scratch.  Its (p, v) is
 *     dbaz_exact_policy's for that position and this attach's pick_seed, bit for bit.  Such a leaf is not on the evaluation lists,
 *     is not counted in or deferred by the full-rounds cut, skips the transposition probe and insert, is not counted in
 *     dbaz_counters.nn_evals, and is counted by dbaz_get_leaf_solves;
 *   - otherwise the leaf goes to the model's evaluator, as without this attach.
 * The rule depends on the leaf's position and the model only: not on the root, the slot, the step or the batch.  It applies to
 * dbaz_search / dbaz_search_timed, self-play, match play and selfplay_pending waves (there a terminal or duplicate leaf of a wave
 * is not solved, as it is not evaluated), alone or next to dbaz_attach_endgame, dbaz_attach_tables and the pool in either mode: a
 * slot that a dry pool denied, or whose table is not valid yet, gets exact leaves a few moves earlier.  endgame_reads stays a
 * property of table-served searches.  The solves run between selection and expansion in one launch per class of F that L reaches
 * (16 / 14-15 / 11-13 / 0-10; 2^F bytes of LDS per leaf), a sequence fixed by the attach: nothing is read back inside a step.
 * The engine BORROWS g and writes nothing to it: the same handle may be attached as dbaz_attach_endgame's or used for
 * dbaz_exact_targets meanwhile.  model: 0, or 1 = the second model in match play.  leaf_free: L, 0 = g's max_free.
 * g == NULL detaches the model (its leaves go to its evaluator again; the counters stay).
 *   the model's evaluator DBAZ_EVAL_EXTERNAL or DBAZ_EVAL_SOLVER, model not 0 / 1 (1 without match play), g of another board size
 *   or device, leaf_free < 0 or > g's max_free                                          -> DBAZ_EINVAL
 *   between dbaz_search_begin and the end of that search, or while games of a dbaz_selfplay_start are being played -> DBAZ_ESTATE
 * A refused call changes nothing.  (Not named dbaz_endgame_*, like dbaz_exact_policy.) */
int dbaz_attach_leaf_solver(dbaz_engine *e, int32_t model, dbaz_endgame *g, int32_t leaf_free, uint64_t pick_seed);
/* by_free int64 [17]: the leaves solved per F = 0 .. 16 (F = 0 never occurs: such a position is finished), cumulative since the
 * first attach, both models together; waits for the engine's queued work.  All 0 without an attach. */
int dbaz_get_leaf_solves(dbaz_engine *e, int64_t *by_free /*[17]*/);

#ifdef __cplusplus
}
#endif
#endif
