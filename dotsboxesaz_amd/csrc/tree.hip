// tree.hip -- per-simulation MCTS kernels, one 64-lane wavefront per game.
//
// Restates the reference's sequential PUCT search (mcts.py, max_pending_evals = 1):
//   k_select          select_leaf      mcts.py:105-114  (+ children_ucb_score/best_child :91-103,
//                                                           lazy child creation utils/utils.py:51-58)
//   k_expand_backup   _search tail     mcts.py:186-199  (prior masking, expand :116-119, backup :121-132)
//   root_prep         UCT_search       mcts.py:211-226  (root renormalisation + Dirichlet mix)
//   k_search_begin    UCT_search       mcts.py:205-208
//   k_advance         init_mcts_tree   mcts.py:163-180  + SelfPlay.play_game / get_next_move /
//                                      get_datasets rows (self_play.py:27-35, 51-74, 95-156)
//
// Numerics follow numpy (NEP 50) exactly: UCB in float64, statistics in float32/int32,
// float32 prior sums with numpy's pairwise summation.  This TU is compiled with
// -ffp-contract=off: a fused multiply-add would change the roundings.
#include "endgame.h"
#include "replay_row.h"
#include "rules.h"
#include "tree.h"

static_assert(FORCED_VISITS_MASK == NS_MASK && FORCED_SAME_BIT == NS_SAME, "forced_playouts.h restates a child's visits | same-player word");

// ------------------------------------------------------------------------------------
// node access
// ------------------------------------------------------------------------------------
struct NodeMeta {
    GState st;
    int parent, move, flags, result, deepness;
    float vhat; // load_meta<true> only (the full Gumbel mode's descent): dword 12, the value the node got at its expansion
};

__device__ __forceinline__ uint32_t *node_ptr(uint32_t *pool, const Geo &g, int idx)
{
    return pool + (size_t)idx * g.node_dw;
}

template <bool VHAT = false>
__device__ __forceinline__ NodeMeta load_meta(uint32_t *pool, const Geo &g, int idx)
{
    const uint32_t *nd = node_ptr(pool, g, idx);
    const uint4 a = *reinterpret_cast<const uint4 *>(nd);
    const uint4 b = *reinterpret_cast<const uint4 *>(nd + 4);
    const uint4 c = *reinterpret_cast<const uint4 *>(nd + 8);
    NodeMeta m;
    m.vhat = VHAT ? __uint_as_float(nd[12]) : 0.0f;
    m.st.e0 = (uint64_t)a.x | ((uint64_t)a.y << 32);
    m.st.e1 = (uint64_t)a.z | ((uint64_t)a.w << 32);
    m.st.e2 = (uint64_t)b.x | ((uint64_t)b.y << 32);
    m.st.e3 = (uint64_t)b.z | ((uint64_t)b.w << 32);
    m.parent = (int)c.x;
    m.move = (int)(int16_t)(c.y & 0xFFFFu);
    m.st.to_play = (int)((c.y >> 16) & 0xFFu);
    m.st.just_played = (int)((c.y >> 24) & 0xFFu) - 1;
    m.st.b2c0 = (int)(int16_t)(c.z & 0xFFFFu);
    m.st.b2c1 = (int)(int16_t)(c.z >> 16);
    m.flags = (int)(c.w & 0xFFu);
    m.result = (int)((c.w >> 8) & 0xFFu) - 1;
    m.deepness = (int)(c.w >> 16);
    return m;
}

// expanded and not terminal: a node select_leaf descends through (`while current.is_expanded`, mcts.py:107)
__device__ __forceinline__ bool is_inner(int flags) { return (flags & NF_EXPANDED) && !(flags & NF_TERMINAL); }

__device__ __forceinline__ uint32_t pack_dw9(int move, int to_play, int just_played)
{
    return ((uint32_t)(uint16_t)(int16_t)move) | ((uint32_t)(to_play & 0xFF) << 16) |
           ((uint32_t)((just_played + 1) & 0xFF) << 24);
}
__device__ __forceinline__ uint32_t pack_dw10(int b0, int b1)
{
    return ((uint32_t)(uint16_t)(int16_t)b0) | ((uint32_t)(uint16_t)(int16_t)b1 << 16);
}
__device__ __forceinline__ uint32_t pack_dw11(int flags, int result, int deepness)
{
    return (uint32_t)(flags & 0xFF) | ((uint32_t)((result + 1) & 0xFF) << 8) | ((uint32_t)deepness << 16);
}

// UCTNode.__init__ (mcts.py:47-65): zeroed W / visits, no children; P is written at expand.
__device__ void init_node(uint32_t *pool, const Geo &g, int idx, const GState &st, int parent, int move,
                          int deepness, int lane)
{
    uint32_t *nd = node_ptr(pool, g, idx);
    int res = gs_result(st);
    int flags = (res != DBAZ_RESULT_NONE) ? NF_TERMINAL : 0;
    if (lane < META_DW) {
        uint32_t v = 0;
        switch (lane) {
        case 0: v = (uint32_t)st.e0; break;
        case 1: v = (uint32_t)(st.e0 >> 32); break;
        case 2: v = (uint32_t)st.e1; break;
        case 3: v = (uint32_t)(st.e1 >> 32); break;
        case 4: v = (uint32_t)st.e2; break;
        case 5: v = (uint32_t)(st.e2 >> 32); break;
        case 6: v = (uint32_t)st.e3; break;
        case 7: v = (uint32_t)(st.e3 >> 32); break;
        case 8: v = (uint32_t)parent; break;
        case 9: v = pack_dw9(move, st.to_play, st.just_played); break;
        case 10: v = pack_dw10(st.b2c0, st.b2c1); break;
        case 11: v = pack_dw11(flags, res, deepness); break;
        default: v = 0; break;
        }
        nd[lane] = v;
    }
    uint32_t *rows = nd + META_DW;
    for (int i = lane; i < g.AS; i += WAVE) {
        rows[g.AS + i] = 0u;             // W = 0.0f
        rows[2 * g.AS + i] = 0u;         // visits = 0
        rows[3 * g.AS + i] = 0xFFFFFFFFu; // child = -1
    }
}

// ------------------------------------------------------------------------------------
// Node pool of one game.  Re-rooting (init_mcts_tree, mcts.py:163-180) moves nothing: the chosen child
// simply becomes the root, and the old root -- its link to the kept child cut -- is handed to a
// collector that enumerates the dropped part of the tree a few nodes per simulation (ring `pend`:
// dropped nodes whose child row is still needed; stack `freel`: indices ready for reuse).  In steady state
// one node is created per simulation and GC_PER_STEP are recycled, so the pool never grows past
// the tree plus one move's worth of garbage.  (Round 1 compacted the kept subtree in place: 2.5-4 MB
// moved by one wave for 0.4-2 ms per move, on a CU the network's workgroups then could not use.)
// ------------------------------------------------------------------------------------
#ifndef GC_PER_STEP
#define GC_PER_STEP 2
#endif
struct PoolState { int n_nodes, n_free, head, tail; };

__device__ __forceinline__ PoolState pool_load(const Slot *S)
{
    PoolState q;
    q.n_nodes = S->n_nodes; q.n_free = S->n_free; q.head = S->pend_head; q.tail = S->pend_tail;
    return q;
}
__device__ __forceinline__ void pool_store(const PoolState &q, Slot *S)
{
    S->n_nodes = q.n_nodes; S->n_free = q.n_free; S->pend_head = q.head; S->pend_tail = q.tail;
}
__device__ __forceinline__ int ring_at(int i, int cap) { return i >= cap ? i - cap : i; }

// Takes up to NB (<= 4) nodes off the pending ring: their children join the ring, the nodes themselves the free
// stack.  Wave-cooperative, wave-uniform state.  Two halves so that the row loads of the batch (all in flight
// together) can overlap other work of the wave: gc_issue reserves the entries and requests their child rows,
// gc_finish consumes them.  Only entries that were on the ring at gc_issue are read.
// NJ: the child rows' words per lane that can hold a child (ceil(A / 64) where the caller knows it, else all four)
template <int NB, int NJ = 4>
struct GcBatch {
    int k;
    int node[NB];
    int32_t c[NB][NJ];
};

template <int NB, int NJ>
__device__ __forceinline__ void gc_issue(GcBatch<NB, NJ> &b, const Geo &g, const TreeBufs &B, int slot, uint32_t *pool, PoolState &q, int lane)
{
    const int avail = q.tail - q.head;
    b.k = avail < NB ? (avail > 0 ? avail : 0) : NB;
    if (b.k == 0) return;
    const int32_t *pend = B.pend + (size_t)slot * g.cap;
    const int h0 = q.head; // head stays in [0, cap), tail in [head, head + cap]
#pragma unroll
    for (int t = 0; t < NB; t++) b.node[t] = t < b.k ? pend[ring_at(h0 + t, g.cap)] : 0;
#pragma unroll
    for (int t = 0; t < NB; t++) {
        const int32_t *Crow = reinterpret_cast<const int32_t *>(node_ptr(pool, g, b.node[t]) + META_DW + 3 * g.AS);
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int i = lane + WAVE * j;
            b.c[t][j] = (t < b.k && i < g.A) ? Crow[i] : -1;
        }
    }
    q.head += b.k;
}

template <int NB, int NJ>
__device__ __forceinline__ void gc_finish(const GcBatch<NB, NJ> &b, const Geo &g, const TreeBufs &B, int slot, PoolState &q, int lane)
{
    if (b.k == 0) return;
    int32_t *pend = B.pend + (size_t)slot * g.cap, *fl = B.freel + (size_t)slot * g.cap;
    int tl = ring_at(q.tail, g.cap);
#pragma unroll
    for (int t = 0; t < NB; t++) {
        if (t < b.k) {
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                if (WAVE * j < g.A) {
                    const bool has = b.c[t][j] >= 0;
                    const unsigned long long m = __ballot(has);
                    if (has) pend[ring_at(tl + (int)__popcll(m & ((1ull << lane) - 1ull)), g.cap)] = b.c[t][j];
                    const int n = (int)__popcll(m);
                    tl = ring_at(tl + n, g.cap);
                    q.tail += n;
                }
            }
            if (lane == 0) fl[q.n_free] = b.node[t];
            q.n_free++;
        }
    }
    if (q.head >= g.cap) { q.head -= g.cap; q.tail -= g.cap; } // keep the counters small (tail - head <= cap always)
}

template <int NB>
__device__ __forceinline__ void pool_collect(const Geo &g, const TreeBufs &B, int slot, uint32_t *pool, PoolState &q, int lane)
{
    GcBatch<NB> b;
    gc_issue(b, g, B, slot, pool, q, lane);
    gc_finish(b, g, B, slot, q, lane);
}

// UCTNode creation needs an index: recycled first, then fresh, then whatever the collector can still find
__device__ __forceinline__ int pool_alloc(const Geo &g, const TreeBufs &B, int slot, uint32_t *pool, PoolState &q, int lane)
{
    if (q.n_free == 0 && q.n_nodes >= g.cap) {
        while (q.n_free == 0 && q.tail > q.head) {
            pool_collect<4>(g, B, slot, pool, q, lane);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the next batch reads ring entries this one pushed
        }
    }
    if (q.n_free > 0) {
        q.n_free--;
        return (B.freel + (size_t)slot * g.cap)[q.n_free]; // wave-uniform load
    }
    if (q.n_nodes < g.cap) return q.n_nodes++;
    return -1;
}

// ------------------------------------------------------------------------------------
// numpy pairwise summation on LDS data (<= 256 elements), result broadcast to the wave.
// Mirrors @TYPE@_pairwise_sum (numpy loops_utils.h.src): 8 strided accumulators per
// block of <= 128, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), tail added in order.
// ------------------------------------------------------------------------------------
template <typename T>
__device__ T np_pairwise_sum(const T *a, int n, int lane)
{
    int grp = lane >> 3, j = lane & 7;
    int s = 0, L = n;
    int n2 = 0;
    if (n > 128) {
        n2 = n / 2;
        n2 -= n2 % 8;
        if (grp == 0) { s = 0; L = n2; } else { s = n2; L = n - n2; }
    }
    T res;
    if (L < 8) {
        res = (T)(-0.0);
        for (int i = 0; i < L; i++)
            res += a[s + i];
    } else {
        T r = a[s + j];
        int lim = L - (L % 8);
        for (int i = 8; i < lim; i += 8)
            r += a[s + i + j];
        T t = r + __shfl_down(r, 1);
        T u = t + __shfl_down(t, 2);
        res = u + __shfl_down(u, 4);
        for (int i = lim; i < L; i++)
            res += a[s + i];
    }
    T b0 = __shfl(res, 0);
    if (n > 128) {
        T b1 = __shfl(res, 8);
        return b0 + b1;
    }
    return b0;
}

// ------------------------------------------------------------------------------------
// formula evaluators (restated from oracle ob_eval_formula; a pure function of the hash)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t fmix64(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

__device__ __forceinline__ uint64_t formula_hash(const GState &st)
{
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    h = fmix64(h ^ st.e0);
    h = fmix64(h ^ st.e1);
    h = fmix64(h ^ st.e2);
    h = fmix64(h ^ st.e3);
    int b = st.to_play == 0 ? st.b2c0 : st.b2c1;
    h = fmix64(h ^ (uint64_t)(int64_t)(b + 512));
    return h;
}
__device__ __forceinline__ float formula_p(uint64_t h, int i, int kind)
{
    if (kind == DBAZ_EVAL_FORMULA_UNIFORM)
        return 1.0f;
    uint64_t t = fmix64(h + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ULL);
    uint32_t u = (uint32_t)(t >> 20) & 0xFFFFu;
    return (float)((u & 0xFFu) + 1u) * (float)(((u >> 8) & 0xFFu) + 1u);
}
__device__ __forceinline__ float formula_v(uint64_t h, int kind)
{
    if (kind == DBAZ_EVAL_FORMULA_UNIFORM)
        return 0.0f;
    uint64_t t = fmix64(h ^ 0xD6E8FEB86659FD93ULL);
    uint32_t u = (uint32_t)(t >> 17) & 0xFFFFu;
    return ((float)u - 32768.0f) / 32768.0f;
}

// ---- per-game transposition table (the reference's (p, v) cache by position hash, utils/proxies.py:35-43) ----
// Entry = tag24 | epoch8 | node index.  A hit is only taken after the candidate node of the LIVE tree has been
// checked: same network input (edges and the mover's boxes_to_close, exactly the reference's hash) and already
// expanded -- so stale entries (old epochs, renumbered nodes) can never return a wrong result, and (p, v) need not
// be stored: the twin's prior row IS masked(p) normalised for the same valid moves, its value sits in meta dword 12.
#define TT_PROBES 4
__device__ __forceinline__ int tt_mover_b2c(const GState &st) { return st.to_play == 0 ? st.b2c0 : st.b2c1; }
__device__ __forceinline__ unsigned tt_epoch_byte(int epoch) { return (unsigned)(epoch % 255) + 1u; }
__device__ __forceinline__ unsigned long long tt_entry(uint64_t h, unsigned ep, int idx)
{
    return ((h >> 40) << 40) | ((unsigned long long)ep << 32) | (unsigned long long)(unsigned)idx;
}

// ------------------------------------------------------------------------------------
// Philox4x32-10 counter RNG (production move sampling / Dirichlet noise; the reference
// uses numpy's global MT19937, which parity tests replace by injected draws)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox(uint4 c, uint2 k)
{
    for (int r = 0; r < 10; r++) {
        uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}
__device__ __forceinline__ double u01(uint32_t a, uint32_t b)
{
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}
// stream: (game, ply, element, purpose)
__device__ __forceinline__ double rng_gamma(uint64_t seed, uint64_t game, uint32_t ply, uint32_t elem, double a)
{
    uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    double boost = 1.0;
    uint32_t ctr = 0;
    if (a < 1.0) {
        uint4 r = philox(make_uint4((uint32_t)game, (uint32_t)(game >> 32) ^ (ply << 8), elem, 0x40000000u), key);
        double u = u01(r.x, r.y);
        if (u < 1e-300) u = 1e-300;
        boost = pow(u, 1.0 / a);
        a += 1.0;
    }
    double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    for (;; ctr++) {
        uint4 r = philox(make_uint4((uint32_t)game, (uint32_t)(game >> 32) ^ (ply << 8), elem, 0x80000000u + ctr), key);
        double u1 = u01(r.x, r.y), u2 = u01(r.z, r.w);
        if (u1 < 1e-300) u1 = 1e-300;
        double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        uint4 r2 = philox(make_uint4((uint32_t)game, (uint32_t)(game >> 32) ^ (ply << 8), elem, 0xC0000000u + ctr), key);
        double u = u01(r2.x, r2.y);
        if (u < 1.0 - 0.0331 * x * x * x * x || (u > 0 && log(u) < 0.5 * x * x + d * (1.0 - v + log(v))))
            return d * v * boost;
        if (ctr > 64) return d * boost; // unreachable in practice; bounded loop
    }
}

// to_play of a node alone (dword 9 of its meta block, common.h)
__device__ __forceinline__ int node_to_play(uint32_t *pool, const Geo &g, int idx) { return (int)((node_ptr(pool, g, idx)[9] >> 16) & 0xffu); }

// Match play (self_play.py:59,237-239): the player to move at the ROOT selects the model for the whole search of this move; odd
// games swap the seats (the reference shuffles them by worker pid)
__device__ __forceinline__ int search_model(const SearchCfg &cfg, int to_play, int64_t game_idx) { return cfg.match_play ? ((to_play ^ (int)(game_idx & 1)) & 1) : 0; }

// ------------------------------------------------------------------------------------
// Gumbel root search (gumbel.h; the rule is in include/dbaz.h): what a search keeps from its preparation.  Runs at the end of
// root_prep, on the float64 root prior it has just written: the candidates, gl = g + logit (-inf for every other child), the
// children's visits of this moment and m'.  ext: noise_in holds a scripted g for this (game, ply).
// ------------------------------------------------------------------------------------
__device__ void gumbel_prep(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, int slot, Slot *S, uint32_t *pool, const NodeMeta &rm,
                            bool ext, int lane)
{
    const int A = g.A;
    const double *rp = B.root_prior + (size_t)slot * g.AS;
    const double *nin = B.noise_in + (size_t)slot * g.AS;
    const uint32_t *NS0 = node_ptr(pool, g, S->root) + META_DW + 2 * g.AS;
    double *gl = B.gumbel_gl + (size_t)slot * g.AS;
    int32_t *n0 = B.gumbel_n0 + (size_t)slot * g.AS;
    int npos = 0, nval = 0;
    for (int i = lane; i < A; i += WAVE) {
        const bool v = gs_valid(g, rm.st, i);
        nval += v ? 1 : 0;
        npos += (v && rp[i] > 0.0) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        nval += __shfl_xor(nval, o);
        npos += __shfl_xor(npos, o);
    }
    const bool any = npos > 0; // no valid child with a positive prior: every valid child is a candidate
    // the searching model's m and scale on g (one model on a self-play handle; dbaz_match_set_search); wave-uniform
    const int model = __builtin_amdgcn_readfirstlane(search_model(cfg, rm.st.to_play, S->game_idx));
    const double g_scale = cfg.gumbel_g_scale[model];
    const uint2 key = make_uint2((uint32_t)cfg.seed, (uint32_t)(cfg.seed >> 32));
    const uint64_t game = (uint64_t)S->game_idx;
    const uint32_t ply = (uint32_t)S->move_idx;
    for (int i = lane; i < A; i += WAVE) {
        const double P = rp[i];
        const bool cand = gs_valid(g, rm.st, i) && (P > 0.0 || !any);
        double x = -INFINITY;
        if (cand) {
            double gv;
            if (ext) {
                gv = nin[i];
            } else {
                const uint4 r = philox(make_uint4((uint32_t)game, (uint32_t)(game >> 32), ply + 65536u * (uint32_t)i, GUMBEL_TAG), key);
                gv = gumbel_from_u(u01(r.x, r.y));
            }
            x = gumbel_noisy_logit(g_scale, gv, gumbel_logit(P));
        }
        gl[i] = x;
        n0[i] = (int32_t)(NS0[i] & NS_MASK);
    }
    if (lane == 0) B.gumbel_hdr[2 * slot + 1] = min(cfg.gumbel_m[model], any ? npos : nval);
    __syncthreads();
}

// ------------------------------------------------------------------------------------
// root prior renormalisation + Dirichlet mix, mcts.py:211-226 (wave-cooperative)
// ------------------------------------------------------------------------------------
// GUMBEL: the instantiation a handle with the Gumbel rule on launches (gumbel.h); false compiles every trace of the rule out
template <int GUMBEL>
__device__ __forceinline__ void root_prep(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, int slot, Slot *S,
                          uint32_t *pool, float *ldsf, double *ldsd, int lane)
{
    const int root = S->root;
    NodeMeta rm = load_meta(pool, g, root);
    const float *Prow = reinterpret_cast<const float *>(node_ptr(pool, g, root) + META_DW);
    double *rp = B.root_prior + (size_t)slot * g.AS;
    const int A = g.A;
    int prepped = S->root_prepped, isf64 = S->root_prior_f64;
    bool probs_f64;
    __syncthreads();
    if (!prepped || !isf64) {
        for (int i = lane; i < A; i += WAVE)
            ldsf[i] = prepped ? (float)rp[i] : Prow[i];
        __syncthreads();
        float cpsum = np_pairwise_sum(ldsf, A, lane);
        probs_f64 = !(cpsum != 0.0f);
        __syncthreads();
        for (int i = lane; i < A; i += WAVE) {
            if (!probs_f64) ldsf[i] = ldsf[i] / cpsum; else ldsd[i] = 0.0;
        }
    } else {
        for (int i = lane; i < A; i += WAVE)
            ldsd[i] = rp[i];
        __syncthreads();
        double cpsum = np_pairwise_sum(ldsd, A, lane);
        probs_f64 = true;
        __syncthreads();
        for (int i = lane; i < A; i += WAVE)
            ldsd[i] = (cpsum != 0.0) ? ldsd[i] / cpsum : 0.0;
    }
    __syncthreads();
    // a fast search of the playout cap is UCT_search(..., dirichlet=(0.0, 0.0)): no noise, coeff = 0; a vector waiting in noise_in
    // (scripted for this ply, or left by the host) is dropped, not kept for a later search
    // a Gumbel search (gumbel.h) is prepared the same way; a vector waiting for it is its g, read before it is dropped here
    const bool gumbel = GUMBEL && (S->fast_search & SEARCH_GUMBEL) != 0;
    const bool g_ext = gumbel && B.noise_valid[slot] != 0;
    if (GUMBEL) __syncthreads();
    const bool fast = (S->fast_search & SEARCH_FAST) != 0 || gumbel;
    const double coeff = fast ? 0.0 : cfg.coeff;
    const double onemc = 1.0 - coeff;
    if (fast && lane == 0) B.noise_valid[slot] = 0;
    if (cfg.alpha > 0 && !fast) {
        const bool ext = B.noise_valid[slot] != 0;
        const double *nin = B.noise_in + (size_t)slot * g.AS;
        double gsum = 0.0;
        double gam[4] = {0, 0, 0, 0};
        if (!ext) {
            // np.random.dirichlet over ALL A slots (mcts.py:220-222), own Philox stream
            int k = 0;
            for (int i = lane; i < A; i += WAVE, k++) {
                gam[k] = rng_gamma(cfg.seed, (uint64_t)S->game_idx, (uint32_t)S->move_idx, (uint32_t)i, cfg.alpha);
                gsum += gam[k];
            }
            for (int o = 32; o > 0; o >>= 1)
                gsum += __shfl_xor(gsum, o);
        }
        int k = 0;
        for (int i = lane; i < A; i += WAVE, k++) {
            double nz = ext ? nin[i] : gam[k] / gsum;
            nz = nz * (gs_valid(g, rm.st, i) ? 1.0 : 0.0);
            double a = probs_f64 ? onemc * ldsd[i] : (double)((float)onemc * ldsf[i]);
            rp[i] = a + coeff * nz;
        }
        S->root_prior_f64 = 1;
        if (lane == 0) B.noise_valid[slot] = 0;
    } else {
        const double cn = coeff * 0.0;
        for (int i = lane; i < A; i += WAVE)
            rp[i] = probs_f64 ? onemc * ldsd[i] + cn : (double)((float)onemc * ldsf[i] + (float)cn);
        S->root_prior_f64 = probs_f64 ? 1 : 0;
    }
    S->root_prepped = 1;
    __syncthreads();
    if (GUMBEL && gumbel) gumbel_prep(g, cfg, B, slot, S, pool, rm, g_ext, lane);
}

// phase and a step stamp leave in ONE 8-byte store.  The driver pass (move choice, re-root, next search) of step t
// runs on a second stream NEXT TO k_select of step t: a slot whose search it starts carries stamp t, and k_select(t)
// -- which may see the slot's old or new phase word -- leaves slots stamped t alone; from step t+1 on (kernel boundary)
// the slot is a searching slot like any other.
__device__ __forceinline__ void set_phase_stamped(Slot *S, int phase, int step)
{
    *reinterpret_cast<volatile unsigned long long *>(&S->phase) = (unsigned long long)(unsigned)phase | ((unsigned long long)(unsigned)step << 32);
}

__device__ __forceinline__ int rule_num_reads(const Geo &g, const SearchCfg &cfg, const GState &st)
{
    // n_searches = min(4*factorial(nb_valid_moves), mcts_num_read), self_play.py:64-65
    int nb = gs_count_valid(g, st);
    double f = 4.0;
    for (int i = 2; i <= nb; i++) {
        f *= (double)i;
        if (f > (double)cfg.mcts_num_read) break;
    }
    return f < (double)cfg.mcts_num_read ? (int)f : cfg.mcts_num_read;
}

// The slot's game is over.  With a pool of tables shared by the slots (EndgameStart::release) the region it holds goes back in
// the pass that follows on this stream, whether or not the slot starts another game.
__device__ __forceinline__ void endgame_release(const StartArgs &sa, int slot, const Slot *S, int lane)
{
    if (sa.eg.release && lane == 0) {
        sa.eg.req[slot].game = S->game_idx;
        sa.eg.req[slot].want = 2;
    }
}

// UCT_search prologue (mcts.py:205-226) for one slot; num_reads < 0 = driver rule
// kind: SEARCH_FAST = a fast search of the playout cap, SEARCH_FORCED / SEARCH_PRUNE = forced playouts at the root and a pruned
// row (start_move_search decides; explicit searches are of kind 0)
template <int GUMBEL>
__device__ __forceinline__ void begin_search(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, int slot, Slot *S,
                             uint32_t *pool, int num_reads, const StartArgs &sa, float *ldsf, double *ldsd, int lane, int kind = 0)
{
    NodeMeta rm = load_meta(pool, g, S->root);
    const bool fast = (kind & SEARCH_FAST) != 0;
    S->fast_search = kind; // root_prep (here or after the root's expansion), the descents and the row of this search read it
    if (rm.flags & NF_TERMINAL) { // play_game never searches a terminal root
        endgame_release(sa, slot, S, lane);
        S->sims_left = 0;
        set_phase_stamped(S, PH_IDLE, cfg.step);
        return;
    }
    if (num_reads < 0) {
        num_reads = rule_num_reads(g, cfg, rm.st);
        if (fast) num_reads = min(num_reads, sa.pc.fast_reads);
        const int model = search_model(cfg, rm.st.to_play, S->game_idx);
        // match play: the searching model's own read budget (dbaz_match_set_search), ahead of the caps below
        if (GUMBEL && cfg.match_reads[model] > 0) num_reads = min(num_reads, cfg.match_reads[model]);
        // a search that the solved table serves needs no more than a few reads (dbaz_attach_solver's solver_reads)
        if ((model ? cfg.evaluator2 : cfg.evaluator) == DBAZ_EVAL_SOLVER && sa.caps.cap[model] > 0) num_reads = min(num_reads, sa.caps.cap[model]);
        // the same for a search whose leaves the slot's endgame table will answer (dbaz_attach_endgame's endgame_reads)
        if (sa.caps.eg_cap[model] > 0 && gs_count_valid(g, rm.st) <= sa.eg.max_free[model]) num_reads = min(num_reads, sa.caps.eg_cap[model]);
        // benchmark population (dbaz_selfplay_stagger): the slot's first search is cut short so that the slots'
        // move boundaries are spread over a whole search instead of all falling into the same step
        // (dbaz_selfplay_quickplay: the opening plies of the slot's first game are searched with a small budget -- a cheap way
        // to a population of positions that search-based play reaches; the staggered budget applies to the first full search)
        const int qu = S->quick_until;
        if (qu > 0 && S->move_idx < qu) {
            num_reads = min(num_reads, max(cfg.quick_reads, 1));
        } else {
            const int ffr = S->ff_reads;
            if (ffr > 0) {
                num_reads = min(num_reads, ffr);
                S->ff_reads = 0;
            }
        }
    }
    if (sa.eg.req) {
        // a search starts: k_endgame_table (next on this stream) solves or re-checks the slot's table before the first selection
        const int model = search_model(cfg, rm.st.to_play, S->game_idx);
        if (sa.eg.max_free[model] > 0 && lane == 0) {
            EndgameReq rq;
            rq.free_edges[0] = ~(rm.st.e0 | g.sentinel[0]) & g.amask[0];
            rq.free_edges[1] = ~(rm.st.e1 | g.sentinel[1]) & g.amask[1];
            rq.free_edges[2] = ~(rm.st.e2 | g.sentinel[2]) & g.amask[2];
            rq.free_edges[3] = ~(rm.st.e3 | g.sentinel[3]) & g.amask[3];
            rq.game = S->game_idx;
            rq.want = 1;
            rq.model = model;
            sa.eg.req[slot] = rq;
        }
    }
    if (GUMBEL && (kind & SEARCH_GUMBEL) && lane == 0) B.gumbel_hdr[2 * slot] = num_reads; // R of sequential halving (gumbel.h)
    S->sims_left = num_reads;
    S->first_wave = 1;
    S->wave_sims = 0;
    if (rm.flags & NF_EXPANDED) {
        root_prep<GUMBEL>(g, cfg, B, slot, S, pool, ldsf, ldsd, lane);
        set_phase_stamped(S, num_reads > 0 ? PH_SIMS : PH_READY, cfg.step);
    } else {
        set_phase_stamped(S, PH_EXPAND_ROOT, cfg.step);
    }
}

__global__ void __launch_bounds__(WAVE) k_search_begin(Geo g, SearchCfg cfg, TreeBufs B, const int32_t *num_reads, StartArgs sa)
{
    __shared__ float ldsf[DBAZ_MAX_A];
    __shared__ double ldsd[DBAZ_MAX_A];
    int slot = blockIdx.x, lane = threadIdx.x;
    Slot *S = B.slots + slot;
    if (S->phase == PH_ERROR || S->game_idx < 0)
        return;
    uint32_t *pool = B.nodes + (size_t)slot * g.cap * g.node_dw;
    begin_search<false>(g, cfg, B, slot, S, pool, num_reads ? num_reads[slot] : -1, sa, ldsf, ldsd, lane);
}

// ------------------------------------------------------------------------------------
// select_leaf, mcts.py:105-114
// ------------------------------------------------------------------------------------
__device__ __forceinline__ bool cand_beats(double xa, int ia, bool ha, double xb, int ib, bool hb)
{
    // numpy argmax order: first maximum; the first NaN beats everything
    if (!ha) return false;
    if (!hb) return true;
    bool na = xa != xa, nb = xb != xb;
    if (na || nb) {
        if (na && nb) return ia < ib;
        return na;
    }
    return xa > xb || (xa == xb && ia < ib);
}

// pb_c's N-dependent factor  log((N + base + 1) / base) + cpuct  and  sqrt(N)  (mcts.py:92-94) from the
// host-libm tables.  N is wave-uniform: the loads are unconditional scalar loads (clamped index) so that
// they can be in flight together with the node's rows; beyond the table the device computes the terms
// (never reached with the default table sizing).
__device__ __forceinline__ void select_tab(const SearchCfg &cfg, const TreeBufs &B, int N, double &pbc, double &sq)
{
    const int i = min(N, cfg.table_n - 1);
    pbc = B.pbc_table[i];
    sq = B.sqrt_table[i];
}
__device__ __forceinline__ void select_tab_fix(const SearchCfg &cfg, int N, double &pbc, double &sq)
{
    if (N >= cfg.table_n) {
        pbc = log(((double)N + cfg.cpuct_base + 1.0) / cfg.cpuct_base) + cfg.cpuct;
        sq = sqrt((double)N);
    }
}

// The four rows of a node (this lane's children i = lane + 64 j) and its meta block are fetched
// together -- the descent then costs ONE dependent memory round trip per tree level (the next
// node's rows are requested the moment the child index is known, which itself comes out of the
// prefetched C row by shuffle) instead of four (rows in two dependent strides, C[best], meta).
template <int NPL>
struct NodeRows {
    float P[NPL], W[NPL];
    uint32_t NS[NPL];
    int32_t C[NPL];
};

template <int NPL>
__device__ __forceinline__ void load_rows(NodeRows<NPL> &r, uint32_t *pool, const Geo &g, int idx, int lane)
{
    const uint32_t *nd = node_ptr(pool, g, idx) + META_DW;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const int i = lane + WAVE * j;
        const bool ok = i < g.A;
        r.P[j] = ok ? reinterpret_cast<const float *>(nd)[i] : 0.0f;
        r.W[j] = ok ? reinterpret_cast<const float *>(nd + g.AS)[i] : 0.0f;
        r.NS[j] = ok ? nd[2 * g.AS + i] : 0u;
        r.C[j] = ok ? reinterpret_cast<const int32_t *>(nd + 3 * g.AS)[i] : -1;
    }
}

// path[depth] = (node, the move that led into it, its player to move): what backup needs of a path node
__device__ __forceinline__ void path_put(PathEnt *path, int depth, int node, int in_move, const NodeMeta &m, int lane)
{
    if (lane == 0) {
        PathEnt pe;
        pe.node = node; pe.move_in = (int16_t)in_move; pe.to_play = (int16_t)m.st.to_play;
        path[depth] = pe;
    }
}

// get_features of a leaf as float32 planes (nn_batch_builder + nn.py:157)
__device__ __forceinline__ void write_features(const Geo &g, const GState &st, float *dst, int lane)
{
    for (int i = lane; i < 3 * g.HW; i += WAVE) dst[i] = (float)gs_feature(g, st, i);
}

// One descent from the root to a leaf (select_leaf, mcts.py:105-114), shared by the one-leaf-per-game step and by the
// K-pending search: UCB scan, wave argmax in numpy's order, path entry, lazy child creation, VIRTUAL_LOSS on every
// node left, and the one-round-trip prefetch of the next level.  vv = 1 (K-pending search with virtual_visits) counts
// the visit of every edge taken, the root's included, NOW instead of at backup; vv = 0 folds away at the call site.
// The leaf's own path entry, path[depth], is the caller's.
// The root level of a Gumbel search (gumbel.h; the rule is in include/dbaz.h): the child this simulation takes.  R: the root's
// rows as the descent holds them, rp: its float64 priors.  Four butterfly reductions (t, n_max and the two sums of v_mix) and the
// argmax; the sums run in the rule's order -- this lane's children in index order, then o = 32 .. 1.  The child found gets
// FORCED_PRIOR in rp, and the root level's pb_c terms become 1, under which that child's score is beyond every other one.
// FULL, the <2> instantiation, and full, the search's own SEARCH_GUMBEL_FULL (dbaz_selfplay_set_gumbel_mode, or the searching model's
// mode in match play): v_mix is the full one, around the root's own value m.vhat (load_meta<true>) with S, the sum of the children's
// visits, riding in the same butterfly.  c_visit, c_scale: the searching model's.
template <int NPL, bool FULL>
__device__ __forceinline__ void gumbel_root_pick(const Geo &g, double c_visit, double c_scale, bool full, const TreeBufs &B, int slot,
                                                 const NodeMeta &m,
                                                 const NodeRows<NPL> &R, double (&rp)[NPL], double &pbc_cur, double &sq_cur, int lane)
{
    const int A = g.A;
    const double *glrow = B.gumbel_gl + (size_t)slot * g.AS;
    const int32_t *n0row = B.gumbel_n0 + (size_t)slot * g.AS;
    const int reads = B.gumbel_hdr[2 * slot], m_eff = B.gumbel_hdr[2 * slot + 1];
    const uint64_t ew[4] = {m.st.e0, m.st.e1, m.st.e2, m.st.e3};
    double gl[NPL];
    int nsr[NPL]; // n_s, the visits of this search
    int t = 0, n_max = 0, Sn = 0;
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const int i = lane + WAVE * j;
        const bool in = i < A;
        const bool valid = in && !(((ew[j] | g.sentinel[j]) >> lane) & 1ull);
        const int n = (int)(R.NS[j] & NS_MASK);
        gl[j] = in ? glrow[i] : -INFINITY;
        nsr[j] = in ? n - n0row[i] : 0;
        t += nsr[j];
        if (FULL) Sn += n;
        n_max = (valid && n > n_max) ? n : n_max;
        num = num + (n > 0 ? rp[j] * forced_value(R.W[j], n, (R.NS[j] & NS_SAME) != 0) : 0.0);
        den = den + (n > 0 ? rp[j] : 0.0);
    }
    for (int o = 32; o > 0; o >>= 1) {
        t += __shfl_xor(t, o);
        if (FULL) Sn += __shfl_xor(Sn, o);
        n_max = max(n_max, __shfl_xor(n_max, o));
        num = num + __shfl_xor(num, o);
        den = den + __shfl_xor(den, o);
    }
    t = __builtin_amdgcn_readfirstlane(t);
    n_max = __builtin_amdgcn_readfirstlane(n_max);
    const double vmix = (FULL && full) ? gumbel_vmix_full((double)m.vhat, Sn, num, den) : gumbel_vmix(num, den);
    int cv = gumbel_considered(m_eff, reads, t);
    // gl + sigma of the candidates at cv visits of this search, -inf for every other child
    double sc[NPL], mx;
    for (int pass = 0;; pass++) {
        mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int n = (int)(R.NS[j] & NS_MASK);
            const double cq = n > 0 ? forced_value(R.W[j], n, (R.NS[j] & NS_SAME) != 0) : vmix;
            sc[j] = (gl[j] > -INFINITY && nsr[j] == cv) ? gl[j] + gumbel_sigma(c_visit, c_scale, n_max, cq) : -INFINITY;
            mx = fmax(mx, sc[j]);
        }
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
        if (mx > -INFINITY || pass) break;
        // no candidate at cv visits (never while t < R): the candidates with the fewest visits compete
        int mn = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < NPL; j++) mn = (gl[j] > -INFINITY && nsr[j] < mn) ? nsr[j] : mn;
        for (int o = 32; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o));
        cv = __builtin_amdgcn_readfirstlane(mn);
    }
    bool found = false;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const unsigned long long mk = __ballot(sc[j] == mx && sc[j] > -INFINITY);
        if (!found && mk != 0ull) {
            if (lane == __ffsll((long long)mk) - 1) rp[j] = FORCED_PRIOR;
            found = true;
        }
    }
    pbc_cur = 1.0;
    sq_cur = 1.0;
}

// A level below the root in the full mode of a Gumbel search (dbaz_selfplay_set_gumbel_mode; the rule is in include/dbaz.h): the
// score pi'(a) - n(a) / (1 + S) of this lane's children, -inf for every child that is no candidate.  R: the node's rows as the
// descent holds them, m.vhat: its own value (load_meta<true>).  Three butterfly reductions -- S, n_max and the two sums of v_mix
// fused, then M, then the sum of e -- in the rule's order; the descent's first-maximum argmax follows on sc.
template <int NPL>
__device__ __forceinline__ void gumbel_inner_scores(const Geo &g, double c_visit, double c_scale, const NodeMeta &m, const NodeRows<NPL> &R,
                                                    double (&sc)[NPL], int lane)
{
    const int A = g.A;
    const uint64_t ew[4] = {m.st.e0, m.st.e1, m.st.e2, m.st.e3};
    int Sn = 0, n_max = 0;
    double num = 0.0, den = 0.0;
    bool pos = false;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const bool valid = lane + WAVE * j < A && !(((ew[j] | g.sentinel[j]) >> lane) & 1ull);
        const int n = (int)(R.NS[j] & NS_MASK);
        const double P = (double)R.P[j];
        Sn += n;
        n_max = (valid && n > n_max) ? n : n_max;
        num = num + (n > 0 ? P * forced_value(R.W[j], n, (R.NS[j] & NS_SAME) != 0) : 0.0);
        den = den + (n > 0 ? P : 0.0);
        pos = pos || (valid && P > 0.0);
    }
    for (int o = 32; o > 0; o >>= 1) {
        Sn += __shfl_xor(Sn, o);
        n_max = max(n_max, __shfl_xor(n_max, o));
        num = num + __shfl_xor(num, o);
        den = den + __shfl_xor(den, o);
    }
    Sn = __builtin_amdgcn_readfirstlane(Sn);
    n_max = __builtin_amdgcn_readfirstlane(n_max);
    const bool any = __ballot(pos) != 0ull;
    const double vmix = gumbel_vmix_full((double)m.vhat, Sn, num, den);
    double M = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const bool valid = lane + WAVE * j < A && !(((ew[j] | g.sentinel[j]) >> lane) & 1ull);
        const int n = (int)(R.NS[j] & NS_MASK);
        const double P = (double)R.P[j];
        const bool cand = valid && (P > 0.0 || !any);
        const double cq = n > 0 ? forced_value(R.W[j], n, (R.NS[j] & NS_SAME) != 0) : vmix;
        sc[j] = cand ? gumbel_logit(P) + gumbel_sigma(c_visit, c_scale, n_max, cq) : -INFINITY;
        M = fmax(M, sc[j]);
    }
    for (int o = 32; o > 0; o >>= 1) M = fmax(M, __shfl_xor(M, o));
    double se = 0.0;
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        sc[j] = sc[j] > -INFINITY ? exp(sc[j] - M) : 0.0; // e(a); 0 for a non-candidate, told apart again below by its validity
        se = se + sc[j];
    }
    for (int o = 32; o > 0; o >>= 1) se = se + __shfl_xor(se, o);
#pragma unroll
    for (int j = 0; j < NPL; j++) {
        const bool valid = lane + WAVE * j < A && !(((ew[j] | g.sentinel[j]) >> lane) & 1ull);
        const int n = (int)(R.NS[j] & NS_MASK);
        const bool cand = valid && ((double)R.P[j] > 0.0 || !any);
        sc[j] = cand ? gumbel_nonroot_score(sc[j] / se, n, Sn) : -INFINITY;
    }
}

struct Leaf {
    int cur, depth, in_move, err;
    int root_to_play;
    NodeMeta m;
};

// GUMBEL = 0 (a handle with the Gumbel rule off, and the K-pending search, which the rule never reaches) compiles the Gumbel
// pre-pass out: the descent is then the parent's, instruction for instruction.  1: the rule at the root level.  2: the full mode
// (dbaz_selfplay_set_gumbel_mode) -- the root level's v_mix is the full one, and every level below the root scores its children by
// gumbel_inner_scores instead of the UCB; 0 and 1 hold no trace of that.
template <int NPL, int GUMBEL>
__device__ __forceinline__ Leaf descend(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, int slot, Slot *S, uint32_t *pool,
                                        PoolState &q, PathEnt *path, const unsigned vv, int lane)
{
    const double *rprior = B.root_prior + (size_t)slot * g.AS;
    const int A = g.A;
    const int root = S->root;
    int cur = root, depth = 0, err = 0;
    const int root_N = S->root_N;
    const int kind = S->fast_search; // requested beside root_N, looked at once the root's rows are on their way
    // (full mode: the root's own value comes with its meta block.  A root made by tree reuse was expanded earlier in the same game
    // under the same setting -- the setters are refused while games are being played -- so k_expand_backup<2> has left it there)
    NodeMeta m = load_meta<GUMBEL == 2>(pool, g, root);
    NodeRows<NPL> R;
    load_rows<NPL>(R, pool, g, root, lane);
    double pbc_cur, sq_cur;
    select_tab(cfg, B, root_N, pbc_cur, sq_cur);
    select_tab_fix(cfg, root_N, pbc_cur, sq_cur);
    double rp[NPL]; // float64 root priors (root_prep), used for the root level only
#pragma unroll
    for (int j = 0; j < NPL; j++) rp[j] = (lane + WAVE * j < A) ? rprior[lane + WAVE * j] : 0.0;
    int in_move = m.move;
    const int root_to_play = m.st.to_play;
    // Gumbel root search (gumbel.h): on for the searches of the self-play driver, and at the root level only, in the instantiations a
    // handle with the rule on launches.  The pre-pass picks the root's child by sequential halving and hands it to the loop the way
    // the forced pre-pass below does, through rp; it also makes the root level's pb_c a plain 1 / (n + 1) > 0, since a re-used root
    // starts its search at N = 0, where sqrt(N) would wipe FORCED_PRIOR out.  (Such a handle has no forced playouts.)
    // The constants are the searching model's (dbaz_match_set_search; a self-play handle has model 0 alone), and in the <2>
    // instantiation the mode is the search's own bit: a root-only search of a handle whose other model is full stays root-only.
    const int gmodel = GUMBEL ? __builtin_amdgcn_readfirstlane(search_model(cfg, root_to_play, S->game_idx)) : 0;
    const double c_visit = GUMBEL ? cfg.gumbel_c_visit[gmodel] : 0.0, c_scale = GUMBEL ? cfg.gumbel_c_scale[gmodel] : 0.0;
    const bool gfull = GUMBEL == 2 && (__builtin_amdgcn_readfirstlane(kind) & SEARCH_GUMBEL_FULL) != 0;
    if (GUMBEL && (__builtin_amdgcn_readfirstlane(kind) & SEARCH_GUMBEL) && is_inner(m.flags))
        gumbel_root_pick<NPL, GUMBEL == 2>(g, c_visit, c_scale, gfull, B, slot, m, R, rp, pbc_cur, sq_cur, lane);
    // full mode: the levels below the root of such a search take the rule's pick, not the UCB's
    const bool ginner = GUMBEL == 2 && gfull && (__builtin_amdgcn_readfirstlane(kind) & SEARCH_GUMBEL) != 0;
    // forced playouts (forced_playouts.h): on for a full search of the self-play driver, and at the root level only
    const bool forced = !GUMBEL && (__builtin_amdgcn_readfirstlane(kind) & SEARCH_FORCED) != 0;
    if (forced && is_inner(m.flags)) {
        // Root-only pre-pass: a forced child scores FORCED_SCORE, above every other score, and the argmax takes the first maximum,
        // so the root level's choice is the lowest forced index.  That child is found here, from rows the root level reads anyway,
        // and handed to the loop below in the one place that is the root level's alone: its entry of rp becomes FORCED_PRIOR, under
        // which its score (pb_c > 0: a forced child has n > 0, so N > 0) is beyond every other one.  The loop itself is untouched:
        // no register and no instruction more at any level, and nothing at all with the rule off.
        const uint64_t ew[4] = {m.st.e0, m.st.e1, m.st.e2, m.st.e3};
        bool found = false;
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int i = lane + WAVE * j;
            const bool valid = i < A && !(((ew[j] | g.sentinel[j]) >> lane) & 1ull);
            const unsigned long long mk = __ballot(valid && forced_child(cfg.forced_k, rp[j], (int)(R.NS[j] & NS_MASK), root_N));
            if (!found && mk != 0ull) {
                if (lane == __ffsll((long long)mk) - 1) rp[j] = FORCED_PRIOR;
                found = true;
            }
        }
    }
    if (lane == 0) {
        if (vv) S->root_N = root_N + 1;
        if (is_inner(m.flags)) S->root_W = S->root_W - 1.0f; // current.total_value -= VIRTUAL_LOSS (root slot)
    }
    while (is_inner(m.flags)) {
        uint32_t *nd = node_ptr(pool, g, cur);
        float *Wrow = reinterpret_cast<float *>(nd + META_DW + g.AS);
        uint32_t *NSrow = nd + META_DW + 2 * g.AS;
        int32_t *Crow = reinterpret_cast<int32_t *>(nd + META_DW + 3 * g.AS);
        // children_ucb_score, mcts.py:91-99 (float64 throughout); the N-dependent terms were requested
        // together with this node's rows (select_tab)
        const double pbc0 = pbc_cur, sq = sq_cur;
        // Branch-free scan of this lane's children (word j of the played / sentinel masks holds child lane + 64 j)
        const uint64_t ew[4] = {m.st.e0, m.st.e1, m.st.e2, m.st.e3};
        double bx = 0.0;
        int bj = 0;
        float bw = 0.0f;
        uint32_t bns = 0;
        int bc = -1;
        bool have = false;
        double gsc[NPL]; // full Gumbel mode, below the root: the rule's scores in place of the UCB's
        const bool gpick = GUMBEL == 2 && ginner && cur != root;
        if (GUMBEL == 2 && gpick) gumbel_inner_scores<NPL>(g, c_visit, c_scale, m, R, gsc, lane);
#pragma unroll
        for (int j = 0; j < NPL; j++) {
            const int i = lane + WAVE * j;
            const bool in = i < A;
            const double P = (cur == root) ? rp[j] : (double)R.P[j];
            const float w = R.W[j];
            const uint32_t ns = R.NS[j];
            const int n = (int)(ns & NS_MASK);
            const double sgn = (ns & NS_SAME) ? 1.0 : -1.0;
            const double t = sq / (double)(n + 1);
            const double pb_c = pbc0 * t;
            const double prior_score = pb_c * P;
            double value_score = (double)w / (double)(1 + n);
            value_score = value_score * sgn;
            const double score = prior_score + value_score;
            const bool valid = in && !(((ew[j] | g.sentinel[j]) >> lane) & 1ull);
            const double inval = valid ? 0.0 : 1.0;
            const double x = (GUMBEL == 2 && gpick) ? gsc[j] : -1e12 * inval + score; // best_child, mcts.py:101-103
            // numpy argmax order inside the lane: first maximum, a NaN already held wins
            const bool take = in && (!have || (bx == bx && !(x <= bx)));
            bx = take ? x : bx;
            bj = take ? j : bj;
            bw = take ? w : bw;
            bns = take ? ns : bns;
            bc = take ? R.C[j] : bc;
            have = have || take;
        }
        int bi;
        if (__ballot(have && bx != bx) == 0ull) {
            // no NaN anywhere (always, in practice): wave maximum, then the lowest child index that attains it
            double mx = have ? bx : -INFINITY;
            for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
            bi = -1;
#pragma unroll
            for (int j = 0; j < NPL; j++) {
                const unsigned long long mk = __ballot(have && bx == mx && bj == j);
                if (bi < 0 && mk != 0ull) bi = WAVE * j + (__ffsll((long long)mk) - 1);
            }
        } else {
            // numpy's argmax with NaNs (the first NaN wins): generic butterfly
            bi = have ? lane + WAVE * bj : 0x7fffffff;
            double rx = bx;
            bool rh = have;
            for (int o = 32; o > 0; o >>= 1) {
                double ox = __shfl_xor(rx, o);
                int oi = __shfl_xor(bi, o);
                int oh = __shfl_xor((int)rh, o);
                if (cand_beats(ox, oi, oh != 0, rx, bi, rh)) { rx = ox; bi = oi; rh = true; }
            }
        }
        // the lane that owns child bi holds it as ITS running best (lanes scan their children in index order and
        // the wave-wide winner is some lane's own best), so its bw / bns / bc are the winner's W, N|sign and C
        // bi and everything read from its owner lane are wave-uniform: say so (scalar branches and loads below)
        bi = __builtin_amdgcn_readfirstlane(bi);
        const int owner = bi & (WAVE - 1);
        bw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bw), owner));
        bns = (uint32_t)__builtin_amdgcn_readlane((int)bns, owner);
        int child = __builtin_amdgcn_readlane(bc, owner);
        path_put(path, depth, cur, in_move, m, lane);
        depth++;
        if (child < 0) {
            // DictWithDefault.__missing__ -> UCTNode(game_state.play(move)), mcts.py:53-54
            child = pool_alloc(g, B, slot, pool, q, lane);
            if (child < 0) { err = DBAZ_EPOOL; depth--; break; }
            GState st = m.st;
            int r = gs_play(g, st, bi, nullptr);
            if (r < 0) { err = DBAZ_EILLEGAL; depth--; break; }
            bool same = (st.to_play == st.just_played);
            if (lane == 0) {
                Crow[bi] = child;
                NSrow[bi] = (same ? NS_SAME : 0u) | vv; // child_player_changed slot (mcts.py:119); visits = 0, or the pending one
            }
            init_node(pool, g, child, st, cur, bi, m.deepness + 1, lane);
            NodeMeta cm;
            cm.st = st; cm.parent = cur; cm.move = bi; cm.vhat = 0.0f;
            cm.result = gs_result(st);
            cm.flags = (cm.result != DBAZ_RESULT_NONE) ? NF_TERMINAL : 0;
            cm.deepness = m.deepness + 1;
            cur = child; in_move = bi; m = cm;
            break;
        }
        // everything the next level needs is requested at once: the child's pb_c / sqrt terms (its visit count is
        // already known from this node's N row), its meta block and its four rows
        const int nchild = (int)(bns & NS_MASK);
        double pbc_nx = 0.0, sq_nx = 0.0;
        if (!(GUMBEL == 2 && ginner)) select_tab(cfg, B, nchild, pbc_nx, sq_nx); // (the full mode's levels below the root need no pb_c terms)
        NodeMeta cm = load_meta<GUMBEL == 2>(pool, g, child);
        load_rows<NPL>(R, pool, g, child, lane); // rows of an unexpanded node are ignored
        if (!(GUMBEL == 2 && ginner)) select_tab_fix(cfg, nchild, pbc_nx, sq_nx);
        if (lane == owner) {
            if (vv) NSrow[bi] = bns + 1u;                       // the visit of the edge into `child`, counted now
            if (is_inner(cm.flags)) Wrow[bi] = bw - 1.0f;      // VIRTUAL_LOSS on the node being left next iteration
        }
        if (is_inner(cm.flags)) {
            pbc_cur = pbc_nx;
            sq_cur = sq_nx;
        }
        cur = child; in_move = bi; m = cm;
    }
    Leaf lf;
    lf.cur = cur; lf.depth = depth; lf.in_move = in_move; lf.err = err; lf.root_to_play = root_to_play; lf.m = m;
    return lf;
}

#ifndef SELECT_WAVES
#define SELECT_WAVES 16 // games per workgroup (one wave each)
#endif
// full rounds only: k_select's class of each slot's leaf (TreeBufs::ev_class), read by k_order_evals
#define EV_CLASS_DEFERRED (-2) // the leaf of an earlier step whose evaluation was put off: head of the list
#define EV_CLASS_NEW (-3)      // a leaf selected in this step
#define SEL_DEFERRED (-2)      // select_one, beside the routes: the slot's put-off leaf asks again (full rounds only)

// The leaf solver's rule (include/dbaz.h, dbaz_attach_leaf_solver) for a non-terminal leaf that no table serves: a leaf with
// at most ls_free[model] free real edges is solved from scratch.  Returns its class, or -1.  Scalar popcounts: wave-uniform.
__device__ __forceinline__ int leaf_solve_rule(const Geo &g, const EndgameBufs &G, int model, const GState &st)
{
    const int L = G.ls_free[model];
    if (L <= 0) return -1;
    const int F = gs_count_valid(g, st);
    return F <= L ? leaf_solve_class(F) : -1;
}
// does the slot's table serve the leaves of this game's search by `model` (one header read)
__device__ __forceinline__ bool table_serves(const EndgameBufs &G, int slot, int64_t game, int model) { return G.hdr && G.model[model] && endgame_hdr_serves(G.hdr[slot], game); }
// The route (tree.h) of a non-terminal, non-duplicate leaf of a search by `model`; tab = table_serves.  A leaf under a valid table
// of its game is answered from it, whatever the evaluator: it is a lookup, so it wins over the leaf solver.  Either keeps the leaf
// off the evaluation lists (so it is never counted in or deferred by the full-rounds cut) and away from the transposition probe.
__device__ __forceinline__ int leaf_route(const Geo &g, const SearchCfg &cfg, const EndgameBufs &G, int model, const GState &st, bool tab)
{
    if (tab) return ROUTE_TABLE;
    const int c = leaf_solve_rule(g, G, model, st);
    return c >= 0 ? ROUTE_SOLVE + c : (eval_uses_list(model ? cfg.evaluator2 : cfg.evaluator) ? model : ROUTE_NONE);
}
// EndgameBufs::leaf, select to expand: the leaf's route where a table or the leaf solver answers it (its (p, v) are in evalP /
// evalV whatever the evaluator), else 0.  leaf_answered is its only reader.
__device__ __forceinline__ void leaf_note(const EndgameBufs &G, size_t row, int route) { if (G.leaf) G.leaf[row] = route >= ROUTE_TABLE ? route : 0; }
__device__ __forceinline__ int leaf_answered(const EndgameBufs &G, size_t row) { return G.leaf ? G.leaf[row] : 0; }
// The lists of the routes.  route_counter: the length word of route r's list.  route_put: entry (the slot, or slot * K + k in a wave)
// goes to place `at` of it; a wave's leaves for the model are on list_m, a single leaf also leaves its place in Slot::eval_pos.
__device__ __forceinline__ int32_t *route_counter(const TreeBufs &B, const EndgameBufs &G, int r)
{
    return r >= ROUTE_SOLVE ? G.ls_cnt + (r - ROUTE_SOLVE) : B.n_eval + (r == ROUTE_TABLE ? 3 : r); // (n_eval[2] is k_tower's)
}
__device__ __forceinline__ void route_put(const TreeBufs &B, const EndgameBufs &G, int r, int at, int entry, bool wave)
{
    if (r >= ROUTE_SOLVE) G.ls_list[(size_t)(r - ROUTE_SOLVE) * G.ls_cap + at] = entry;
    else if (r == ROUTE_TABLE) G.list[at] = entry;
    else if (wave) B.list_m[at] = entry;
    else {
        (r ? B.eval_list2 : B.eval_list)[at] = entry;
        B.slots[entry].eval_pos = at;
    }
}

// The pool of tables in wait mode (dbaz_attach_tables_pool_wait): a slot whose search found the pool dry selects nothing until a
// pass grants it a region (EndgameSlotHdr::wait == ENDGAME_WAITING) -- its reads and its tree stay as begin_search left them.  The
// pass that wakes it leaves its step there, like set_phase_stamped: where it runs next to this step's selection, the slot -- whose
// table that pass is still solving -- takes its first selection in the next step, behind the join.
__device__ __forceinline__ bool endgame_slot_waits(const SearchCfg &cfg, const EndgameBufs &G, int slot)
{
    if (!G.hdr || !G.wait) return false;
    const int w = __builtin_amdgcn_readfirstlane(*reinterpret_cast<volatile const int32_t *>(&G.hdr[slot].wait));
    return w == ENDGAME_WAITING || (w == cfg.step && cfg.driver_concurrent);
}

// returns the route of this game's leaf (ROUTE_NONE: of no leaf, or of one that goes on no list), or SEL_DEFERRED
template <int NPL, int GUMBEL>
__device__ __forceinline__ int select_one(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, const EndgameBufs &G, int slot, int lane)
{
    Slot *S = B.slots + slot;
    const unsigned long long pw = *reinterpret_cast<volatile const unsigned long long *>(&S->phase); // phase | stamp << 32
    // (one address for the whole wave: say so, and the branches on it are scalar)
    const int phase = __builtin_amdgcn_readfirstlane((int)(unsigned)pw), stamp = __builtin_amdgcn_readfirstlane((int)(unsigned)(pw >> 32));
    if (phase != PH_EXPAND_ROOT && phase != PH_SIMS)
        return ROUTE_NONE;
    if (stamp == cfg.step && cfg.driver_concurrent) // search started by this step's driver pass (see set_phase_stamped)
        return ROUTE_NONE;
    if (endgame_slot_waits(cfg, G, slot))
        return ROUTE_NONE;
    if (cfg.eval_round > 0 && S->pending) {
        // the leaf of an earlier step whose evaluation was put off (full rounds only): path, leaf and features are still in place.
        // k_order_evals puts it at the head of the list.
        if (lane == 0) S->sel_step = cfg.step;
        return SEL_DEFERRED;
    }
    uint32_t *pool = B.nodes + (size_t)slot * g.cap * g.node_dw;
    PathEnt *path = B.path + (size_t)slot * g.dmax;
    PoolState q = pool_load(S);
    GcBatch<GC_PER_STEP, NPL> gcb; // the collector's share of this simulation: rows requested now, consumed after the descent
    gcb.k = 0;
    if (cfg.gc_lazy <= 0 || q.n_free + (g.cap - q.n_nodes) < cfg.gc_lazy) gc_issue(gcb, g, B, slot, pool, q, lane);
    const Leaf lf = descend<NPL, GUMBEL>(g, cfg, B, slot, S, pool, q, path, 0u, lane);
    if (lf.err) {
        if (lane == 0) { S->error = lf.err; S->phase = PH_ERROR; }
        return ROUTE_NONE;
    }
    const NodeMeta &m = lf.m;
    const int cur = lf.cur;
    const int model = search_model(cfg, lf.root_to_play, S->game_idx);
    gc_finish(gcb, g, B, slot, q, lane);
    path_put(path, lf.depth, cur, lf.in_move, m, lane);
    if (lane == 0) {
        S->leaf = cur;
        S->sel_step = cfg.step;
        S->path_len = lf.depth + 1;
        S->leaf_terminal = (m.flags & NF_TERMINAL) ? 1 : 0;
        S->leaf_result = m.result;
        S->leaf_to_play = m.st.to_play;
        pool_store(q, S);
        S->model = model;
        if (q.n_nodes > S->pool_high) S->pool_high = q.n_nodes;
    }
    int route = (m.flags & NF_TERMINAL) ? ROUTE_NONE : leaf_route(g, cfg, G, model, m.st, table_serves(G, slot, S->game_idx, model));
    if (lane == 0) leaf_note(G, slot, route);
    if (!(m.flags & NF_TERMINAL)) {
        write_features(g, m.st, B.feat + (size_t)slot * 3 * g.HW, lane);
        const int ev = model ? cfg.evaluator2 : cfg.evaluator;
        int hit = -1;
        // (the table exists for network evaluators, and for the formula evaluators when forced on -- transposition_cache
        // = 2 -- so that the hit path can be compared with the oracle bit for bit)
        if (B.tt && leaf_uses_transpositions(ev, route >= ROUTE_TABLE)) {
            // lanes 0..TT_PROBES-1 read the probe window; a candidate is verified against the live tree
            const uint64_t h = formula_hash(m.st);
            const unsigned long long *tt = B.tt + (size_t)slot * ((size_t)B.tt_mask + 1);
            unsigned long long *ttw = B.tt + (size_t)slot * ((size_t)B.tt_mask + 1);
            unsigned long long ent = 0;
            if (lane < TT_PROBES) ent = tt[((unsigned)h + (unsigned)lane) & (unsigned)B.tt_mask];
            unsigned long long cand = __ballot(lane < TT_PROBES && ent != 0ull && (ent >> 40) == (h >> 40));
            const int mb = tt_mover_b2c(m.st);
            while (cand && hit < 0) {
                const int pl = __ffsll((long long)cand) - 1;
                cand &= cand - 1;
                const int idx = (int)(unsigned)__shfl(ent, pl);
                if (idx >= 0 && idx < q.n_nodes && idx != cur) {
                    const NodeMeta tm = load_meta(pool, g, idx);
                    if (is_inner(tm.flags) && tm.st.e0 == m.st.e0 && tm.st.e1 == m.st.e1 &&
                        tm.st.e2 == m.st.e2 && tm.st.e3 == m.st.e3 && tt_mover_b2c(tm.st) == mb) {
                        hit = idx;
                        // still in use: stamp the entry with the current epoch (old epochs are the preferred victims)
                        if (lane == 0)
                            ttw[((unsigned)h + (unsigned)pl) & (unsigned)B.tt_mask] = tt_entry(h, tt_epoch_byte(S->tt_epoch), idx);
                    }
                }
            }
            if (hit >= 0) route = ROUTE_NONE;
        }
        if (lane == 0) S->leaf_hit = hit;
    }
    return route;
}

// One wave per game.  Two forms; tree_launch_select picks by cfg.eval_round, and neither form serves the other's path.
//
// Sixteen games (SELECT_WAVES) per workgroup wherever this kernel writes the evaluation lists itself (cfg.eval_round == 0:
// match play, two networks, the manual search calls).  The leaves that need a network evaluation are
// appended to the per-model lists with ONE global atomic per workgroup and model (positions inside
// the workgroup come from an LDS counter): a per-wave atomicAdd on the single list counter serialises
// 8192 same-address atomics per step and was most of this kernel's duration.  The other routes' lists are written the same way.
// A value that a wave without a slot carries around the descent costs a register for its whole length: `route` is the only one.
//
// ONE (full rounds only, cfg.eval_round > 0): one game per workgroup.  There this kernel appends to no network list -- it leaves
// ev_class[slot] for k_order_evals -- so nothing is left to share between the games of a workgroup: no LDS counters, no barrier,
// and a game's registers are free the moment ITS descent ends instead of when the deepest of sixteen does.  The rare leaf of
// ROUTE_TABLE or the leaf solver goes onto its list with the wave's own atomic.
template <int NPL, bool ONE, int GUMBEL>
__global__ void __launch_bounds__(ONE ? WAVE : WAVE * SELECT_WAVES) k_select(Geo g, SearchCfg cfg, TreeBufs B, int n_slots, EndgameBufs G)
{
    if (ONE) {
        const int slot = blockIdx.x, lane = threadIdx.x;
        if (slot >= n_slots) return;
        const int route = select_one<NPL, GUMBEL>(g, cfg, B, G, slot, lane);
        if (lane == 0) {
            B.ev_class[slot] = route == SEL_DEFERRED ? EV_CLASS_DEFERRED : (route == ROUTE_MODEL0 ? EV_CLASS_NEW : -1);
            // (full rounds: one model, so no model bit on a solver entry)
            if (route >= ROUTE_TABLE) route_put(B, G, route, atomicAdd(route_counter(B, G, route), 1), slot, false);
        }
        return;
    }
    __shared__ int s_cnt[N_ROUTES], s_base[N_ROUTES];
    const int slot = blockIdx.x * SELECT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & (WAVE - 1);
    if (threadIdx.x < N_ROUTES) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int route = ROUTE_NONE; // (no put-off leaves here: they are of the full rounds)
    if (slot < n_slots) route = select_one<NPL, GUMBEL>(g, cfg, B, G, slot, lane);
    const bool put = route >= 0 && lane == 0;
    int my = 0;
    if (put) my = atomicAdd(&s_cnt[route], 1);
    __syncthreads();
    // (two statements: one for all routes holds both counters' addresses in scalar registers across the descent, 16 bytes of scratch)
    const int t = threadIdx.x;
    if (t < ROUTE_SOLVE && s_cnt[t] > 0) s_base[t] = atomicAdd(route_counter(B, G, t), s_cnt[t]);
    if (t >= ROUTE_SOLVE && t < N_ROUTES && s_cnt[t] > 0) s_base[t] = atomicAdd(route_counter(B, G, t), s_cnt[t]);
    __syncthreads();
    if (put) // a solver entry carries the model: the model's seed picks
        route_put(B, G, route, s_base[route] + my, route >= ROUTE_SOLVE ? slot | (B.slots[slot].model << LEAF_SOLVE_MODEL_SHIFT) : slot, false);
}

// Full rounds only (SearchCfg.eval_round > 0, one model): which leaves land behind the network's cut depends on their order in
// the list, so the list must not follow the order in which k_select's workgroups finish.  k_select leaves every slot's class in
// ev_class; this one workgroup writes the list in slot order, the put-off leaves first, then the leaves of this step -- the same
// list on every run.  The order starts at slot `rot`, which moves with the step: the leaves behind the cut are spread over the
// slots as the atomic order spread them, instead of the same top slots waiting every other step.
//
// The scan kernels (this one and k_driver_scan) are one workgroup of SCAN_T threads that hands every flagged item its rank in item
// order.  A thread takes item c * SCAN_T + t of each of the NG chunks of a group: the caller issues all NG loads first (they are
// independent, so they cost one memory round trip, not NG), and scan_ranks turns the flags of all chunks and all NCLS classes
// into ranks with ONE exchange through LDS: per-wave popcounts in (class, chunk, wave) order, an exclusive scan of that table by
// the first wave, two barriers.  More items than SCAN_T * NG are taken group after group.
#define SCAN_T 1024
#define SCAN_W (SCAN_T / WAVE)
#define SCAN_NG 8       // chunks per group: the values a thread holds in registers at once ...
#define SCAN_NG_SMALL 2 // ... and the instance for at most SCAN_T * SCAN_NG_SMALL slots, which does not pay for eight

// fl[cls] bit c: this thread's item of chunk c is in class cls.  rank[cls][c]: the number of class-cls items of the group in front
// of it (chunk, then thread order); tot[cls]: all of them.  s_pre: NCLS * NG * SCAN_W + 1 ints, free again after the call only
// behind a barrier.
template <int NCLS, int NG>
__device__ __forceinline__ void scan_ranks(int *s_pre, const unsigned (&fl)[NCLS], int (&rank)[NCLS][NG], int (&tot)[NCLS])
{
    constexpr int E = NCLS * NG * SCAN_W, PER = E / WAVE;
    static_assert(E % WAVE == 0, "the first wave scans E / WAVE table entries per lane");
    const int t = threadIdx.x, lane = t & (WAVE - 1), w = t / WAVE;
#pragma unroll
    for (int cls = 0; cls < NCLS; cls++) {
#pragma unroll
        for (int c = 0; c < NG; c++) {
            const unsigned long long m = __ballot((fl[cls] >> c) & 1u);
            rank[cls][c] = (int)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) s_pre[(cls * NG + c) * SCAN_W + w] = (int)__popcll(m);
        }
    }
    __syncthreads();
    if (w == 0) {
        int v[PER], sum = 0;
#pragma unroll
        for (int k = 0; k < PER; k++) { v[k] = s_pre[lane * PER + k]; sum += v[k]; }
        int inc = sum;
        for (int o = 1; o < WAVE; o <<= 1) {
            const int up = __shfl_up(inc, o);
            inc += lane >= o ? up : 0;
        }
        int ex = inc - sum;
#pragma unroll
        for (int k = 0; k < PER; k++) { s_pre[lane * PER + k] = ex; ex += v[k]; }
        if (lane == WAVE - 1) s_pre[E] = inc;
    }
    __syncthreads();
#pragma unroll
    for (int cls = 0; cls < NCLS; cls++) {
        const int first = s_pre[cls * NG * SCAN_W];
#pragma unroll
        for (int c = 0; c < NG; c++) rank[cls][c] += s_pre[(cls * NG + c) * SCAN_W + w] - first;
        tot[cls] = s_pre[(cls + 1) * NG * SCAN_W] - first; // (the entry behind the last class is the grand total)
    }
}

template <int NG>
__global__ void __launch_bounds__(SCAN_T) k_order_evals(TreeBufs B, int n_slots, int rot)
{
    __shared__ int s_pre[2 * NG * SCAN_W + 1], s_def[SCAN_W];
    const int t = threadIdx.x, lane = t & (WAVE - 1), w = t / WAVE;
    const bool one_group = n_slots <= SCAN_T * NG;
    // this step's leaves start behind ALL put-off leaves: with more than one group these are counted first
    int n_def = 0;
    if (!one_group) {
        int n = 0;
        for (int i = t; i < n_slots; i += SCAN_T) n += B.ev_class[i] == EV_CLASS_DEFERRED ? 1 : 0;
        for (int o = WAVE / 2; o > 0; o >>= 1) n += __shfl_xor(n, o);
        if (lane == 0) s_def[w] = n;
        __syncthreads();
        for (int k = 0; k < SCAN_W; k++) n_def += s_def[k];
    }
    int base_def = 0, base_new = 0;
    for (int g0 = 0; g0 < n_slots; g0 += SCAN_T * NG) {
        int cl[NG];
#pragma unroll
        for (int c = 0; c < NG; c++) {
            const int j = g0 + c * SCAN_T + t, i = j + rot < n_slots ? j + rot : j + rot - n_slots;
            cl[c] = j < n_slots ? B.ev_class[i] : -1;
        }
        unsigned fl[2] = {0u, 0u};
#pragma unroll
        for (int c = 0; c < NG; c++) {
            fl[0] |= (cl[c] == EV_CLASS_DEFERRED ? 1u : 0u) << c;
            fl[1] |= (cl[c] == EV_CLASS_NEW ? 1u : 0u) << c;
        }
        int rank[2][NG], tot[2];
        scan_ranks<2, NG>(s_pre, fl, rank, tot);
        if (one_group) n_def = tot[0];
#pragma unroll
        for (int c = 0; c < NG; c++) {
            if ((fl[0] | fl[1]) >> c & 1u) {
                const int j = g0 + c * SCAN_T + t, i = j + rot < n_slots ? j + rot : j + rot - n_slots;
                const int pos = (fl[0] >> c & 1u) ? base_def + rank[0][c] : n_def + base_new + rank[1][c];
                B.eval_list[pos] = i;
                B.slots[i].eval_pos = pos;
            }
        }
        base_def += tot[0];
        base_new += tot[1];
        if (g0 + SCAN_T * NG < n_slots) __syncthreads(); // s_pre is written again
    }
    if (t == 0) B.n_eval[0] = base_def + base_new;
}

// Full rounds only (SearchCfg.eval_round > 0).  A network launch costs whole rounds of workgroups (nn.hip): 5 306 leaves are four
// rounds of 1 280 and a remainder round that costs 40 % of a round for 3.5 % of the leaves.  When at most eval_defer_max leaves
// would be left behind the last full round, the network kernels take only the full rounds (nn.hip cut_n: every kernel of the step
// applies the same rule to the same count; k_tower leaves the count in n_eval[2]); the slots behind the cut keep their selected
// leaf -- k_expand_backup sets Slot::pending -- and ask again in the next step, at the head of the list (k_order_evals).  Every game
// plays the same moves: only WHEN a slot's simulation completes changes.

// ------------------------------------------------------------------------------------
// UCT_search with K > 1 pending evaluations on ONE tree (mcts.py:228-239; players.AZPlayer).
// A wave of the search = up to K simulations selected ONE AFTER THE OTHER by the tree's wavefront, each leaving a
// virtual loss on its leaf path, then ONE batched evaluation of their leaves, then their expand + backup in the same
// order.  Virtual loss: exactly the reference's `total_value -= VIRTUAL_LOSS` on every node a simulation leaves
// (mcts.py:108-109; restored by backup's `+ VIRTUAL_LOSS`), plus what the reference lacks -- the visit is counted on
// every edge of the path, the leaf's included, at SELECT time instead of at backup time, so that the simulations of a
// wave spread over the tree instead of piling onto one leaf (with K = 64 the reference's in-flight leaves are
// 98 % duplicates).  A leaf that is selected again while its evaluation is pending is not evaluated twice (NF_INFLIGHT).
// With K = 1 every number equals the sequential kernels' (and the oracle's) bit for bit: a simulation never reads a
// count it has itself incremented.
// ------------------------------------------------------------------------------------
template <int NPL>
__device__ __forceinline__ void select_multi_one(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, const EndgameBufs &G, int slot, int lane)
{
    Slot *S = B.slots + slot;
    const int phase = S->phase;
    if (phase != PH_EXPAND_ROOT && phase != PH_SIMS) return;
    if (endgame_slot_waits(cfg, G, slot)) return;
    uint32_t *pool = B.nodes + (size_t)slot * g.cap * g.node_dw;
    const int A = g.A, K = B.kmax;
    int width = min(max(cfg.pending, 1), K);
    if (S->first_wave) width = min(width, A);                 // max_pend = min(max_pending_evals, len(valid_moves))
    int n_sims = phase == PH_EXPAND_ROOT ? 1 : min(width, S->sims_left);
    PoolState q = pool_load(S);
    const unsigned vv = cfg.virtual_visits ? 1u : 0u; // the visit is counted at selection (backup then adds the value only)
    // Model 0 here and below: the waves never run match play (dbaz_create refuses the combination), so k_select_multi's solver
    // entries carry no model bit either.  One header read per slot, not per simulation.
    const bool tab = table_serves(G, slot, S->game_idx, 0);
    int err = 0, done = 0;
    for (int k = 0; k < n_sims && !err; k++) {
        PathEnt *path = B.path_m + ((size_t)slot * K + k) * g.dmax;
        pool_collect<GC_PER_STEP>(g, B, slot, pool, q, lane);
        const Leaf lf = descend<NPL, false>(g, cfg, B, slot, S, pool, q, path, vv, lane);
        err = lf.err;
        if (err) break;
        // leaf bookkeeping of simulation k
        const NodeMeta &m = lf.m;
        const bool term = (m.flags & NF_TERMINAL) != 0;
        const bool dup = !term && (m.flags & NF_INFLIGHT);
        path_put(path, lf.depth, lf.cur, lf.in_move, m, lane);
        if (lane == 0) {
            SimRec sr;
            sr.leaf = lf.cur; sr.path_len = lf.depth + 1; sr.terminal = term ? 1 : 0; sr.result = m.result; sr.to_play = m.st.to_play;
            sr.dup = dup ? 1 : 0;
            if (G.leaf) {
                // leaf_route's first half written out, and only with something attached: the K-loop's descents run in sequence and
                // pay for every register it holds -- calling leaf_route here cost the single tree 1.5 to 3 % (EXPERIMENTS 2)
                const int lsc = tab || term || dup ? -1 : leaf_solve_rule(g, G, 0, m.st);
                G.leaf[(size_t)slot * K + k] = (term || dup) ? 0 : (tab ? ROUTE_TABLE : (lsc >= 0 ? ROUTE_SOLVE + lsc : 0));
            }
            B.simrec[(size_t)slot * K + k] = sr;
            if (!term && !dup)
                node_ptr(pool, g, lf.cur)[11] = pack_dw11(m.flags | NF_INFLIGHT, m.result, m.deepness);
        }
        if (!term && !dup) write_features(g, m.st, B.feat_m + ((size_t)slot * K + k) * 3 * g.HW, lane);
        done = k + 1;
        // the next simulation of this wave reads what this one wrote (same wavefront: program order + a drain)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    if (lane == 0) {
        if (err) { S->error = err; S->phase = PH_ERROR; }
        S->wave_sims = done;
        S->sel_step = cfg.step;
        if (phase == PH_SIMS) S->first_wave = 0; // (the root expansion is not one of the waves)
        pool_store(q, S);
        if (q.n_nodes > S->pool_high) S->pool_high = q.n_nodes;
    }
}

template <int NPL>
__global__ void __launch_bounds__(WAVE) k_select_multi(Geo g, SearchCfg cfg, TreeBufs B, int n_slots, EndgameBufs G)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot >= n_slots) return;
    select_multi_one<NPL>(g, cfg, B, G, slot, lane);
    __syncthreads();
    // the lists: the wave's simulations of each route, in simulation order (one loop over all routes is the slower code: EXPERIMENTS 2)
    const Slot *S = B.slots + slot;
    if (S->phase == PH_ERROR) return;
    const int K = B.kmax, n = S->wave_sims;
    const bool lists = eval_uses_list(cfg.evaluator);
    if ((!lists && !G.leaf) || S->sel_step != cfg.step) return;
    for (int k0 = 0; k0 < n; k0 += WAVE) {
        const int k = k0 + lane;
        int route = ROUTE_NONE;
        if (k < n) {
            const SimRec sr = B.simrec[(size_t)slot * K + k];
            route = leaf_answered(G, (size_t)slot * K + k); // (0 for a terminal or duplicate leaf)
            if (route == 0) route = lists && !sr.terminal && !sr.dup ? ROUTE_MODEL0 : ROUTE_NONE;
        }
        const bool need = route == ROUTE_MODEL0, eg = route == ROUTE_TABLE;
        const int lsc = route >= ROUTE_SOLVE ? route - ROUTE_SOLVE : -1;
        const unsigned long long mk = __ballot(need), me = __ballot(eg);
        int base = 0, ebase = 0;
        if (lane == 0 && mk) base = atomicAdd(route_counter(B, G, ROUTE_MODEL0), (int)__popcll(mk));
        if (lane == 0 && me) ebase = atomicAdd(route_counter(B, G, ROUTE_TABLE), (int)__popcll(me));
        base = __shfl(base, 0), ebase = __shfl(ebase, 0);
        if (need) route_put(B, G, ROUTE_MODEL0, base + (int)__popcll(mk & ((1ull << lane) - 1ull)), slot * K + k, true);
        if (eg) route_put(B, G, ROUTE_TABLE, ebase + (int)__popcll(me & ((1ull << lane) - 1ull)), slot * K + k, true);
        for (int c = 0; G.ls_list && c < LEAF_SOLVE_CLASSES; c++) {
            const unsigned long long ml = __ballot(lsc == c);
            if (!ml) continue;
            int lbase = 0;
            if (lane == 0) lbase = atomicAdd(route_counter(B, G, ROUTE_SOLVE + c), (int)__popcll(ml));
            lbase = __shfl(lbase, 0);
            if (lsc == c) route_put(B, G, ROUTE_SOLVE + c, lbase + (int)__popcll(ml & ((1ull << lane) - 1ull)), slot * K + k, true);
        }
    }
}

// ------------------------------------------------------------------------------------
// _search tail, the pieces both search modes share: prior masking (mcts.py:189-196) + expand (:116-119),
// backup (:121-132), the per-simulation statistics, and the end of a step's work on a slot
// ------------------------------------------------------------------------------------
// P row of the leaf = child_priors * valid, renormalised as the reference does; returns v.  The priors and the value come
// from the formula of evaluator `ev`, or from ep[A] / *evv.  ldsf must be free (wave-cooperative).
__device__ __forceinline__ float expand_priors(const Geo &g, const GState &st, int ev, bool from_table, const float *ep, const float *evv,
                                               float *Prow, float *ldsf, int lane)
{
    const bool formula = !leaf_reads_eval_buffers(ev, from_table);
    uint64_t h = 0;
    if (formula) h = formula_hash(st);
    for (int i = lane; i < g.A; i += WAVE) {
        float p = formula ? formula_p(h, i, ev) : ep[i];
        ldsf[i] = p * (gs_valid(g, st, i) ? 1.0f : 0.0f); // child_priors * valid
    }
    __syncthreads();
    float s = np_pairwise_sum<float>(ldsf, g.A, lane);
    const bool renorm = (s > 0.0f) && (s != 1.0f);
    for (int i = lane; i < g.A; i += WAVE)
        Prow[i] = renorm ? ldsf[i] / s : ldsf[i];
    return formula ? formula_v(h, ev) : *evv;
}

// every path node (root ... leaf) gets W += v_n + VIRTUAL_LOSS, and N += 1 unless the visits were counted at selection
__device__ __forceinline__ void backup_path(const Geo &g, uint32_t *pool, Slot *S, const PathEnt *path, int plen, int leaf_to_play, float v,
                                            bool count_visits, int lane)
{
    for (int d = lane; d < plen; d += WAVE) {
        PathEnt pe = path[d];
        float vn = (pe.to_play == leaf_to_play) ? v : -v;
        float add = vn + 1.0f;
        if (d == 0) {
            S->root_W = S->root_W + add;
            if (count_visits) S->root_N = S->root_N + 1;
        } else {
            uint32_t *pn = node_ptr(pool, g, path[d - 1].node);
            float *Wr = reinterpret_cast<float *>(pn + META_DW + g.AS);
            uint32_t *NSr = pn + META_DW + 2 * g.AS;
            Wr[pe.move_in] = Wr[pe.move_in] + add;
            if (count_visits) NSr[pe.move_in] = NSr[pe.move_in] + 1u;
        }
    }
}

// statistics of one finished simulation; served = its leaf needed no evaluation of its own (transposition hit / duplicate leaf);
// eg = answered from the slot's endgame table: neither an evaluation nor a hit
__device__ __forceinline__ void count_sim(Slot *S, int term, bool served, bool eg, int path_len, int deepness)
{
    S->terminal_count += term;
    if (deepness > S->max_deepness) S->max_deepness = deepness;
    S->n_search += 1;
    S->sum_path += path_len;
    S->n_term += term;
    S->n_eval += (term || served || eg) ? 0 : 1;
    S->n_hit += served ? 1 : 0;
}

// a slot's step ends: the root expansion (uncounted, mcts.py:207-208) hands over to the simulations, `sims` of which are done otherwise
template <int GUMBEL>
__device__ __forceinline__ void end_step(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, int slot, Slot *S, uint32_t *pool, int phase,
                                         int sims, float *ldsf, double *ldsd, int lane)
{
    if (phase == PH_EXPAND_ROOT) {
        root_prep<GUMBEL>(g, cfg, B, slot, S, pool, ldsf, ldsd, lane);
        if (lane == 0) set_phase_stamped(S, S->sims_left > 0 ? PH_SIMS : PH_READY, cfg.step);
    } else if (lane == 0) {
        int left = S->sims_left - sims;
        S->sims_left = left;
        if (left <= 0) set_phase_stamped(S, PH_READY, cfg.step);
    }
}

// The step's last kernel resets the per-step counters (the routes' lists and the driver list are consumed by then): no memset launches.
__device__ __forceinline__ void reset_step_counters(const TreeBufs &B, const EndgameBufs &G, int slot, int lane)
{
    if (slot == 0 && lane < N_ROUTES && (lane < ROUTE_SOLVE || G.ls_cnt)) *route_counter(B, G, lane) = 0;
    if (slot == 0 && lane == 0) B.drv_count[0] = 0;
}

__global__ void __launch_bounds__(WAVE) k_expand_backup_multi(Geo g, SearchCfg cfg, TreeBufs B, EndgameBufs G)
{
    __shared__ float ldsf[DBAZ_MAX_A];
    __shared__ double ldsd[DBAZ_MAX_A];
    const int slot = blockIdx.x, lane = threadIdx.x;
    reset_step_counters(B, G, slot, lane);
    Slot *S = B.slots + slot;
    const int phase = S->phase;
    if (phase != PH_EXPAND_ROOT && phase != PH_SIMS) return;
    if (S->sel_step != cfg.step) return;
    uint32_t *pool = B.nodes + (size_t)slot * g.cap * g.node_dw;
    const int K = B.kmax, n = S->wave_sims;
    for (int k = 0; k < n; k++) {
        const SimRec sr = B.simrec[(size_t)slot * K + k];
        const bool eg = !sr.terminal && !sr.dup && leaf_answered(G, (size_t)slot * K + k) != 0;
        const PathEnt *path = B.path_m + ((size_t)slot * K + k) * g.dmax;
        NodeMeta lm = load_meta(pool, g, sr.leaf);
        uint32_t *nd = node_ptr(pool, g, sr.leaf);
        float v;
        if (sr.terminal) {
            v = (float)lm.result;
        } else if (lm.flags & NF_EXPANDED) {
            v = __uint_as_float(nd[12]); // expanded by an earlier simulation of this wave (sr.dup): same (p, v)
        } else {
            __syncthreads(); // ldsf is reused from the simulation before
            v = expand_priors(g, lm.st, cfg.evaluator, eg, B.evalP_m + ((size_t)slot * K + k) * g.AS, B.evalV_m + (size_t)slot * K + k,
                              reinterpret_cast<float *>(nd + META_DW), ldsf, lane);
            if (lane == 0) nd[12] = __float_as_uint(v);
        }
        if (lane == 0) nd[11] = pack_dw11((lm.flags | NF_EXPANDED) & ~NF_INFLIGHT, lm.result, lm.deepness);
        // N += 1 here (the reference) or already at selection (virtual_visits)
        backup_path(g, pool, S, path, sr.path_len, lm.st.to_play, v, !cfg.virtual_visits, lane);
        if (lane == 0) count_sim(S, sr.terminal, sr.dup != 0, eg, sr.path_len, lm.deepness);
        // the next simulation's path shares nodes with this one (same wavefront: program order + a drain)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    __syncthreads();
    end_step<false>(g, cfg, B, slot, S, pool, phase, n, ldsf, ldsd, lane);
    if (lane == 0) S->wave_sims = 0;
}

// ------------------------------------------------------------------------------------
// _search tail: prior masking (mcts.py:189-196), expand (:116-119), backup (:121-132)
// ------------------------------------------------------------------------------------
// Four waves per SIMD (second launch bound: at most 128 registers), so that 8 192 slots are two rounds of one-wave workgroups
// instead of 2.67.  What does not fit is the float64 pow / log / cos of the Dirichlet sampler inlined through end_step ->
// root_prep -> rng_gamma: the allocator spills there, once per move, and nowhere on the path of an ordinary simulation.
template <int GUMBEL>
__global__ void __launch_bounds__(WAVE, 4) k_expand_backup(Geo g, SearchCfg cfg, TreeBufs B, EndgameBufs G)
{
    __shared__ float ldsf[DBAZ_MAX_A];
    __shared__ double ldsd[DBAZ_MAX_A];
    const int slot = blockIdx.x, lane = threadIdx.x;
    reset_step_counters(B, G, slot, lane);
    Slot *S = B.slots + slot;
    const int phase = S->phase;
    if (phase != PH_EXPAND_ROOT && phase != PH_SIMS)
        return;
    // only slots for which THIS step's k_select left a leaf: the driver kernel (second stream) may have started a new
    // search in a slot while this step's network was running
    if (S->sel_step != cfg.step)
        return;
    uint32_t *pool = B.nodes + (size_t)slot * g.cap * g.node_dw;
    const PathEnt *path = B.path + (size_t)slot * g.dmax;
    const int A = g.A;
    const int leaf = S->leaf, plen = S->path_len;
    NodeMeta lm = load_meta(pool, g, leaf);
    uint32_t *nd = node_ptr(pool, g, leaf);
    float v;
    int hit = -1;
    const bool eg = !(lm.flags & NF_TERMINAL) && leaf_answered(G, slot) != 0; // (p, v) came from the slot's endgame table or the leaf solver
    if (!(lm.flags & NF_TERMINAL)) {
        float *Prow = reinterpret_cast<float *>(nd + META_DW);
        const int ev = (cfg.match_play && S->model) ? cfg.evaluator2 : cfg.evaluator;
        if (B.tt) hit = S->leaf_hit;
        if (cfg.eval_round > 0 && hit < 0 && !eval_is_formula(ev) && !eg) {
            // behind this step's cut: the network has not seen the leaf; keep it and ask again next step
            const bool late = S->eval_pos >= B.n_eval[2];
            if (lane == 0) S->pending = late ? 1 : 0;
            if (late) return;
        }
        if (hit >= 0) {
            // transposition: the twin's row is masked(p) / sum for the same valid moves, its v the same network output
            const uint32_t *tw = node_ptr(pool, g, hit);
            const float *Psrc = reinterpret_cast<const float *>(tw + META_DW);
            for (int i = lane; i < A; i += WAVE) Prow[i] = Psrc[i];
            v = __uint_as_float(tw[12]);
        } else {
            v = expand_priors(g, lm.st, ev, eg, B.evalP + (size_t)slot * g.AS, B.evalV + slot, Prow, ldsf, lane);
        }
        // full Gumbel mode: every expanded node keeps its value there, with or without a table -- the descent's v_mix reads it
        if (GUMBEL == 2 && !B.tt && lane == 0) nd[12] = __float_as_uint(v);
        if (B.tt && lane == 0) {
            nd[12] = __float_as_uint(v); // a later twin reads the value here
            if (hit < 0 && !eg) {
                // insert: first empty / stale-epoch / same-tag entry of the probe window, else a hash-chosen victim
                const uint64_t h = formula_hash(lm.st);
                unsigned long long *tt = B.tt + (size_t)slot * ((size_t)B.tt_mask + 1);
                const unsigned ep = tt_epoch_byte(S->tt_epoch);
                int victim = (int)((h >> 20) & (TT_PROBES - 1));
                for (int q = TT_PROBES - 1; q >= 0; q--) {
                    const unsigned long long e0 = tt[((unsigned)h + (unsigned)q) & (unsigned)B.tt_mask];
                    if (e0 == 0ull || ((unsigned)(e0 >> 32) & 0xFFu) != ep || (e0 >> 40) == (h >> 40)) victim = q;
                }
                tt[((unsigned)h + (unsigned)victim) & (unsigned)B.tt_mask] = tt_entry(h, ep, leaf);
            }
        }
    } else {
        v = (float)lm.result; // get_result(), python int
    }
    if (lane == 0)
        nd[11] = pack_dw11(lm.flags | NF_EXPANDED, lm.result, lm.deepness);
    backup_path(g, pool, S, path, plen, lm.st.to_play, v, true, lane);
    __syncthreads();
    if (lane == 0) count_sim(S, (lm.flags & NF_TERMINAL) ? 1 : 0, hit >= 0, eg, plen, lm.deepness);
    end_step<GUMBEL>(g, cfg, B, slot, S, pool, phase, 1, ldsf, ldsd, lane);
}

// ------------------------------------------------------------------------------------
// init_mcts_tree (mcts.py:163-180): O(1) re-root.  reuse_tree: the chosen child becomes the root where it
// lies (its subtree keeps its node indices, so transposition entries stay valid), the old root -- link to
// the kept child cut -- goes onto the collector's ring.  Otherwise the whole pool is dropped.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void pool_reset(Slot *S)
{
    S->root = 0;
    S->n_nodes = 1;
    S->n_free = 0;
    S->pend_head = 0;
    S->pend_tail = 0;
}

// re-root slot on `move`; returns 0 or an error code.  wave-uniform.
// need_free > 0 (the self-play driver): the kept subtree holds at most min(`carried`, nodes of the whole tree - 1) nodes (every
// node below the chosen child was created by a distinct simulation through it); if that plus need_free exceeds the pool, the next
// search could run out of nodes half-way.  The reference's trees are unbounded Python objects; here such a move starts from a fresh root instead (as with
// reuse_tree = 0, counted in Slot::pool_resets) -- a trained network that puts nearly all visits on one move for many plies in a
// row (a chain) keeps nearly everything, move after move.  need_free = 0 (dbaz_advance): no check, exhaustion stays an error.
__device__ int reroot(const Geo &g, const TreeBufs &B, int slot, Slot *S, uint32_t *pool, int move,
                      int reuse, int lane, int need_free = 0)
{
    const int root = S->root;
    NodeMeta rm = load_meta(pool, g, root);
    uint32_t *nd0 = node_ptr(pool, g, root);
    if (move < 0 || move >= g.A)
        return DBAZ_EILLEGAL;
    int child = (int)nd0[META_DW + 3 * g.AS + move];
    int carried = (int)(nd0[META_DW + 2 * g.AS + move] & NS_MASK);
    GState st;
    int child_deep;
    if (child >= 0) {
        NodeMeta cm = load_meta(pool, g, child);
        st = cm.st;
        child_deep = cm.deepness;
    } else {
        st = rm.st;
        if (gs_play(g, st, move, nullptr) < 0)
            return DBAZ_EILLEGAL;
        child_deep = rm.deepness + 1;
        carried = 0;
    }
    __syncthreads();
    if (reuse && child >= 0 && need_free > 0 && carried + need_free > g.cap) {
        // visits over-count nodes (a revisit of a terminal leaf creates none: end games carry thousands of visits on a few
        // hundred nodes), so take the exact count before giving the subtree up: with the collector drained, the nodes in use
        // are those of the current tree (root, kept child and siblings)
        PoolState q = pool_load(S);
        while (q.tail > q.head) {
            pool_collect<4>(g, B, slot, pool, q, lane);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the next batch reads ring entries this one pushed
        }
        if (lane == 0) pool_store(q, S);
        const int live = q.n_nodes - q.n_free - 1;
        if ((carried < live ? carried : live) + need_free > g.cap) {
            reuse = 0;
            if (lane == 0) S->pool_resets++;
        }
        __syncthreads();
    }
    if (reuse && child >= 0) {
        const int tail = S->pend_tail;
        if (lane == 0) {
            nd0[META_DW + 3 * g.AS + move] = 0xFFFFFFFFu;           // the kept subtree is no child of the dropped root
            node_ptr(pool, g, child)[8] = 0xFFFFFFFFu;               // new root: parent = None
            (B.pend + (size_t)slot * g.cap)[ring_at(tail, g.cap)] = root;
        }
        S->pend_tail = tail + 1;
        S->root = child;
        S->deepness_correction = child_deep;
        S->tree_size = carried;
    } else if (reuse) {
        // children[move] did not exist: a fresh, unexpanded node becomes the root; nothing else survives
        pool_reset(S);
        init_node(pool, g, 0, st, -1, move, child_deep, lane);
        S->deepness_correction = child_deep;
        S->tree_size = carried;
    } else {
        // create_root_uct_node(child.game_state); next_node.move = move
        pool_reset(S);
        init_node(pool, g, 0, st, -1, move, 1, lane);
        S->deepness_correction = 0;
        S->tree_size = 0;
    }
    // new TreeRoot: fresh defaultdict slots and statistics (mcts.py:22-31)
    S->root_N = 0;
    S->root_W = 0.0f;
    S->root_prepped = 0;
    S->root_prior_f64 = 0;
    S->max_deepness = 0;
    S->terminal_count = 0;
    S->tt_epoch = S->tt_epoch + 1; // entries of older moves become the preferred victims (they stay valid while their node lives)
    __syncthreads();
    return 0;
}

// reset slot to a fresh game from the empty board (create_root_uct_node(BoxesState())) or from its entry of the start table
__device__ void fresh_game(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, int slot, Slot *S,
                           uint32_t *pool, long long game_idx, int lane)
{
    GState st;
    gs_init(g, st);
    int ff = S->ff_plies;
    int plies = 0;
    if (B.n_starts > 0) {
        // play_games(game_state, idxs): the start table's entry of this game (uniform over the lanes; never combined with ff_plies)
        st = B.start_states[(game_idx / B.games_per_start) % B.n_starts];
    } else if (ff > 0) {
        // synthetic mid-game population (benchmark only): uniformly random legal plies
        uint2 key = make_uint2((uint32_t)cfg.seed ^ 0xA5A5A5A5u, (uint32_t)(cfg.seed >> 32));
        for (int t = 0; t < ff; t++) {
            int nb = gs_count_valid(g, st);
            if (nb <= 1) break;
            uint4 r = philox(make_uint4((uint32_t)game_idx, (uint32_t)(game_idx >> 32), (uint32_t)t, 0x11111111u), key);
            int pick = (int)(r.x % (uint32_t)nb);
            int mv = -1;
            for (int i = 0; i < g.A; i++) {
                if (gs_valid(g, st, i)) {
                    if (pick == 0) { mv = i; break; }
                    pick--;
                }
            }
            GState trial = st;
            gs_play(g, trial, mv, nullptr);
            if (gs_result(trial) != DBAZ_RESULT_NONE) break;
            st = trial;
            plies++;
        }
        S->ff_plies = 0;
    }
    init_node(pool, g, 0, st, -1, -1, 1, lane);
    pool_reset(S);
    S->root_N = 0;
    S->root_W = 0.0f;
    S->root_prepped = 0;
    S->root_prior_f64 = 0;
    S->deepness_correction = 0;
    S->max_deepness = 0;
    S->terminal_count = 0;
    S->tree_size = 0;
    S->move_idx = 0;
    S->n_rows = 0;
    S->game_idx = game_idx;
    S->temperature = 1.0;
    S->phase = PH_IDLE;
    S->sel_step = 0; // no leaf pending (step numbers start at 1)
    S->tt_epoch = S->tt_epoch + 1;
    (void)plies;
    __syncthreads();
}

__global__ void __launch_bounds__(WAVE) k_set_positions(Geo g, SearchCfg cfg, TreeBufs B, const int16_t *moves,
                                                        const int32_t *offsets)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    Slot *S = B.slots + slot;
    uint32_t *pool = B.nodes + (size_t)slot * g.cap * g.node_dw;
    GState st;
    gs_init(g, st);
    int err = 0;
    if (moves && offsets) {
        for (int i = offsets[slot]; i < offsets[slot + 1]; i++)
            if (gs_play(g, st, moves[i], nullptr) < 0) { err = DBAZ_EILLEGAL; break; }
    }
    S->ff_plies = 0;
    S->ff_reads = 0;
    S->quick_until = 0;
    fresh_game(g, cfg, B, slot, S, pool, slot, lane);
    init_node(pool, g, 0, st, -1, -1, 1, lane);
    if (lane == 0) {
        S->error = err;
        S->phase = err ? PH_ERROR : PH_IDLE;
        S->n_search = S->sum_path = S->n_eval = S->n_term = S->n_hit = 0;
        S->pool_high = 1;
        S->pool_resets = 0;
        S->pending = 0;
    }
}

// manual init_mcts_tree on every slot with moves[slot] >= 0
__global__ void __launch_bounds__(WAVE) k_advance_manual(Geo g, SearchCfg cfg, TreeBufs B, const int32_t *moves,
                                                         int reuse)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    Slot *S = B.slots + slot;
    if (S->phase == PH_ERROR || S->game_idx < 0)
        return;
    int mv = moves[slot];
    if (mv < 0)
        return;
    uint32_t *pool = B.nodes + (size_t)slot * g.cap * g.node_dw;
    int err = reroot(g, B, slot, S, pool, mv, reuse, lane);
    if (lane == 0) {
        if (err) { S->error = err; S->phase = PH_ERROR; }
        else { S->phase = PH_IDLE; S->move_idx += 1; }
    }
}

// ------------------------------------------------------------------------------------
// self-play driver: SelfPlay.play_game / get_next_move / get_datasets (self_play.py)
// ------------------------------------------------------------------------------------
__device__ bool try_emit(const Geo &g, const TreeBufs &B, int slot, Slot *S, uint32_t *pool, int lane)
{
    // rows of the finished game -> output buffer, z per row (self_play.py:105-112)
    NodeMeta rm = load_meta(pool, g, S->root); // terminal root
    const int n = S->n_rows;
    int base = 0;
    if (lane == 0) {
        base = atomicAdd(B.out_count, n);
        if (base + n > B.max_out) {
            atomicSub(B.out_count, n);
            base = -1;
        }
    }
    base = __shfl(base, 0);
    if (base < 0)
        return false;
    const int F = 3 * g.HW, A = g.A, rcap = g.E + 1;
    const int winner = rm.st.just_played;
    const int zt = rm.result;
    for (int r = 0; r < n; r++) {
        const int16_t *sx = B.row_x + ((size_t)slot * rcap + r) * F;
        int16_t *dx = B.out_x + (size_t)(base + r) * F;
        for (int i = lane; i < F; i += WAVE) dx[i] = sx[i];
        const int32_t *sv = B.row_vis + ((size_t)slot * rcap + r) * A;
        int32_t *dv = B.out_vis + (size_t)(base + r) * A;
        for (int i = lane; i < A; i += WAVE) dv[i] = sv[i];
        if (lane == 0) {
            RowMeta mm = B.row_meta[(size_t)slot * rcap + r];
            mm.z = (int8_t)((mm.player == winner) ? zt : -zt);
            B.out_meta[base + r] = mm;
        }
    }
    if (lane == 0) {
        atomicAdd((unsigned long long *)B.games_finished, 1ull);
    }
    return true;
}

template <int GUMBEL>
__device__ __forceinline__ void start_move_search(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, int slot, Slot *S,
                                  uint32_t *pool, const StartArgs &sa, float *ldsf, double *ldsd, int lane)
{
    // play_game loop head (self_play.py:57-66): temperature schedule, sims budget, search
    const int i = S->move_idx;
    for (int k = 0; k < cfg.n_temp; k++)
        if (cfg.temp_idx[k] == i) S->temperature = cfg.temp_val[k];
    // teacher-forced Dirichlet vector for this (game, ply), if scripted
    long long gi = S->game_idx - B.first_game;
    // playout cap: full or fast is a function of (seed, game, ply) alone
    const bool fast = !playout_is_full(sa.pc, cfg.seed, S->game_idx, (uint32_t)i);
    if (lane == 0) atomicAdd((unsigned long long *)B.moves_played + (fast ? 2 : 1), 1ull);
    // (with the Gumbel rule on, a scripted vector is the search's g, whatever the noise setting, and for fast searches too)
    // (the rule is the searching model's: dbaz_match_set_search gives each model of a match its own; wave-uniform)
    const int model = GUMBEL ? __builtin_amdgcn_readfirstlane(search_model(cfg, node_to_play(pool, g, S->root), S->game_idx)) : 0;
    const bool gumbel = GUMBEL && cfg.gumbel_m[model] > 0;
    if ((gumbel || (cfg.alpha > 0 && !fast)) && B.script_noise && gi >= 0 && gi < B.n_script && B.script_has_noise[gi] && i <= g.E) {
        const double *src = B.script_noise + ((size_t)gi * (g.E + 1) + i) * g.A;
        double *dst = B.noise_in + (size_t)slot * g.AS;
        for (int k = lane; k < g.A; k += WAVE) dst[k] = src[k];
        if (lane == 0) B.noise_valid[slot] = 1;
        __syncthreads();
        __threadfence_block();
    } else if (GUMBEL && gumbel && lane == 0) {
        B.noise_valid[slot] = 0; // only a scripted vector is a search's g: one that the host left in noise_in is dropped
    }
    if (GUMBEL && gumbel && lane == 0) atomicAdd((unsigned long long *)B.moves_played + 5, 1ull); // Gumbel searches started
    // forced playouts belong to the driver's full searches (with the cap off every search is one)
    // (the Gumbel rule belongs to every search of the driver, full or fast; a handle has it or forced playouts, never both)
    const int kind = (fast ? SEARCH_FAST : (cfg.forced_k > 0.0 ? SEARCH_FORCED | (cfg.forced_prune ? SEARCH_PRUNE : 0) : 0)) | (gumbel ? SEARCH_GUMBEL | (cfg.gumbel_mode[model] ? SEARCH_GUMBEL_FULL : 0) : 0);
    begin_search<GUMBEL>(g, cfg, B, slot, S, pool, -1, sa, ldsf, ldsd, lane, kind);
}


template <int GUMBEL>
__global__ void __launch_bounds__(WAVE) k_selfplay_start(Geo g, SearchCfg cfg, TreeBufs B, StartArgs sa)
{
    __shared__ float ldsf[DBAZ_MAX_A];
    __shared__ double ldsd[DBAZ_MAX_A];
    const int slot = blockIdx.x, lane = threadIdx.x;
    Slot *S = B.slots + slot;
    uint32_t *pool = B.nodes + (size_t)slot * g.cap * g.node_dw;
    if (lane == 0) {
        S->error = 0;
        S->n_search = S->sum_path = S->n_eval = S->n_term = S->n_hit = 0;
        S->pool_high = 1;
        S->pool_resets = 0;
        S->pending = 0;
    }
    // deterministic initial assignment: slot i takes game first+i (the dispenser starts behind them)
    long long gidx = B.first_game + slot;
    if (gidx >= B.last_game) {
        S->game_idx = -1;
        S->phase = PH_IDLE;
        return;
    }
    fresh_game(g, cfg, B, slot, S, pool, gidx, lane);
    start_move_search<GUMBEL>(g, cfg, B, slot, S, pool, sa, ldsf, ldsd, lane);
}

// The end of a Gumbel search (gumbel.h; the rule is in include/dbaz.h), everything read after the search: the move -- the first
// maximum of gl + sigma over the candidates with the most visits of this search -- is returned, and rv (if not null) gets the
// row's visits, softmax(logit + sigma) over the candidates in units of 2^-24.  One wave; the sums run in the rule's order.
// FULL (the <2> instantiation) and full (the search's SEARCH_GUMBEL_FULL): v_mix is the full one around the root's own value,
// dword 12 of its meta block.  It is always there: the root was expanded by k_expand_backup<2> in this game, whichever model
// searched then, as a root or -- under tree reuse -- as an inner node earlier on, since the setters are refused while games
// are being played.
template <bool FULL>
__device__ int gumbel_finish(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, int slot, uint32_t *pool, int root, const NodeMeta &rm,
                             bool full, int32_t *rv, double *ldsd, int lane)
{
    const int A = g.A;
    const int model = __builtin_amdgcn_readfirstlane(search_model(cfg, rm.st.to_play, B.slots[slot].game_idx)); // whose constants
    const double c_visit = cfg.gumbel_c_visit[model], c_scale = cfg.gumbel_c_scale[model];
    const uint32_t *NS0 = node_ptr(pool, g, root) + META_DW + 2 * g.AS;
    const float *W0 = reinterpret_cast<const float *>(node_ptr(pool, g, root) + META_DW + g.AS);
    const double *rprior = B.root_prior + (size_t)slot * g.AS;
    const double *gl = B.gumbel_gl + (size_t)slot * g.AS;
    const int32_t *n0 = B.gumbel_n0 + (size_t)slot * g.AS;
    int n_max = 0, ns_max = -1, Sn = 0;
    double num = 0.0, den = 0.0;
    for (int i = lane; i < A; i += WAVE) {
        const uint32_t ns = NS0[i];
        const int n = (int)(ns & NS_MASK);
        if (FULL) Sn += n;
        if (gs_valid(g, rm.st, i) && n > n_max) n_max = n;
        if (gl[i] > -INFINITY && n - n0[i] > ns_max) ns_max = n - n0[i];
        num = num + (n > 0 ? rprior[i] * forced_value(W0[i], n, (ns & NS_SAME) != 0) : 0.0);
        den = den + (n > 0 ? rprior[i] : 0.0);
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_max = max(n_max, __shfl_xor(n_max, o));
        ns_max = max(ns_max, __shfl_xor(ns_max, o));
        if (FULL) Sn += __shfl_xor(Sn, o);
        num = num + __shfl_xor(num, o);
        den = den + __shfl_xor(den, o);
    }
    const double vmix = (FULL && full) ? gumbel_vmix_full((double)__uint_as_float(node_ptr(pool, g, root)[12]), Sn, num, den) : gumbel_vmix(num, den);
    // the move, and x = logit + sigma with its maximum
    double bs = -INFINITY, M = -INFINITY;
    int bi = 0x7fffffff;
    __syncthreads();
    for (int i = lane; i < A; i += WAVE) {
        const bool cand = gl[i] > -INFINITY;
        double x = -INFINITY;
        if (cand) {
            const uint32_t ns = NS0[i];
            const int n = (int)(ns & NS_MASK);
            const double sg = gumbel_sigma(c_visit, c_scale, n_max, n > 0 ? forced_value(W0[i], n, (ns & NS_SAME) != 0) : vmix);
            const double s = gl[i] + sg;
            if (n - n0[i] == ns_max && s > bs) { bs = s; bi = i; }
            x = gumbel_logit(rprior[i]) + sg;
            if (x > M) M = x;
        }
        ldsd[i] = x;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(bs, o);
        const int oi = __shfl_xor(bi, o);
        if (os > bs || (os == bs && oi < bi)) { bs = os; bi = oi; }
        M = fmax(M, __shfl_xor(M, o));
    }
    if (rv) {
        double se = 0.0;
        for (int i = lane; i < A; i += WAVE) {
            const double e = ldsd[i] > -INFINITY ? exp(ldsd[i] - M) : 0.0;
            ldsd[i] = e;
            se = se + e;
        }
        for (int o = 32; o > 0; o >>= 1) se = se + __shfl_xor(se, o);
        for (int i = lane; i < A; i += WAVE) rv[i] = gl[i] > -INFINITY ? gumbel_count(ldsd[i] / se) : 0;
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(bi);
}

// One pass of the driver for every slot whose reads are done (PH_READY), whose finished game still waits for output space
// (PH_EMIT) or whose game ended in an earlier pass (PH_NEWGAME: it starts the game k_driver_scan gave it).  A game that ends
// here leaves the slot in PH_NEWGAME until the next pass.
// (the slots come from k_driver_scan's list: a step in which no slot needs the driver costs two tiny launches instead
// of one workgroup per game squeezing in between the network's workgroups)
template <int GUMBEL>
__device__ __forceinline__ void advance_one(const Geo &g, const SearchCfg &cfg, const TreeBufs &B, int slot, const StartArgs &sa, float *ldsf,
                            double *ldsd, int lane)
{
    Slot *S = B.slots + slot;
    const int phase = S->phase;
    if (phase != PH_READY && phase != PH_EMIT && phase != PH_NEWGAME)
        return;
    uint32_t *pool = B.nodes + (size_t)slot * g.cap * g.node_dw;
    const int A = g.A, F = 3 * g.HW, rcap = g.E + 1;
    if (phase == PH_NEWGAME) {
        // the game index k_driver_scan handed out in this pass
        const long long gidx = S->game_idx;
        S->quick_until = 0; // only a slot's first game has quick plies
        fresh_game(g, cfg, B, slot, S, pool, gidx, lane);
        start_move_search<GUMBEL>(g, cfg, B, slot, S, pool, sa, ldsf, ldsd, lane);
        return;
    }
    if (phase == PH_EMIT) {
        if (try_emit(g, B, slot, S, pool, lane) && lane == 0)
            S->phase = PH_NEWGAME;
        return;
    }
    const int root = S->root;
    NodeMeta rm = load_meta(pool, g, root);
    const uint32_t *NS0 = node_ptr(pool, g, root) + META_DW + 2 * g.AS;
    // ---- get_next_move (self_play.py:27-35) ----
    int vmax = 0;
    long long vsum = 0;
    for (int i = lane; i < A; i += WAVE) {
        int vc = (int)(NS0[i] & NS_MASK);
        vmax = vc > vmax ? vc : vmax;
        vsum += vc;
    }
    for (int o = 32; o > 0; o >>= 1) {
        int ov = __shfl_xor(vmax, o);
        vmax = ov > vmax ? ov : vmax;
        vsum += __shfl_xor(vsum, o);
    }
    int mv = -1;
    const int ply = S->move_idx;
    long long gi = S->game_idx - B.first_game;
    if (B.script_moves && gi >= 0 && gi < B.n_script && ply <= g.E)
        mv = B.script_moves[(size_t)gi * (g.E + 1) + ply];
    const int r = S->n_rows;
    const int kind = S->fast_search;
    const bool gumbel = GUMBEL && (kind & SEARCH_GUMBEL) != 0;
    if (GUMBEL && gumbel) {
        // Gumbel root search (gumbel.h): the move by the rule -- no temperature, the move-draw stream is not consumed -- unless a
        // scripted one wins, and the row's visits, which are the target pi'
        const int gmv = gumbel_finish<GUMBEL == 2>(g, cfg, B, slot, pool, root, rm, (kind & SEARCH_GUMBEL_FULL) != 0, r < rcap ? B.row_vis + ((size_t)slot * rcap + r) * A : nullptr, ldsd, lane);
        if (mv < 0) mv = gmv;
    }
    if (mv < 0) {
        // probs = (vc/vc.max())**(1/T); probs /= probs.sum(); np.random.choice(A, p=probs)
        const double invT = 1.0 / S->temperature;
        for (int i = lane; i < A; i += WAVE) {
            int vc = (int)(NS0[i] & NS_MASK);
            ldsd[i] = pow((double)vc / (double)vmax, invT);
        }
        __syncthreads();
        double ps = np_pairwise_sum<double>(ldsd, A, lane);
        __syncthreads();
        if (lane == 0) {
            double c = 0.0;
            for (int i = 0; i < A; i++) { c += ldsd[i] / ps; ldsd[i] = c; } // cumsum
        }
        __syncthreads();
        const double last = ldsd[A - 1];
        uint2 key = make_uint2((uint32_t)cfg.seed, (uint32_t)(cfg.seed >> 32));
        uint4 r = philox(make_uint4((uint32_t)S->game_idx, (uint32_t)(S->game_idx >> 32), (uint32_t)ply, 0x22222222u), key);
        const double u = u01(r.x, r.y);
        int cnt = 0;
        for (int i = lane; i < A; i += WAVE)
            cnt += (ldsd[i] / last <= u) ? 1 : 0; // searchsorted(side='right')
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        mv = cnt;
        if (mv >= A) { // unreachable (cdf[-1]/last == 1 > u); fall back to the most visited move
            int bv = -1, bidx = 0;
            for (int i = 0; i < A; i++) { int vc = (int)(NS0[i] & NS_MASK); if (vc > bv) { bv = vc; bidx = i; } }
            mv = bidx;
        }
        __syncthreads();
    }
    // ---- row of get_datasets for this root (self_play.py:107-117) ----
    const bool prune = (kind & SEARCH_PRUNE) != 0;
    if (r < rcap) {
        int16_t *rx = B.row_x + ((size_t)slot * rcap + r) * F;
        for (int i = lane; i < F; i += WAVE) rx[i] = (int16_t)gs_feature(g, rm.st, i);
        int32_t *rv = B.row_vis + ((size_t)slot * rcap + r) * A;
        if (prune) {
            // policy target pruning (forced_playouts.h; the rule is in include/dbaz.h): the move above came from the raw visits, the
            // tree keeps them, the row gets n'.  c* = the first valid child with the most visits
            int bn = -1, bi = 0x7fffffff;
            for (int i = lane; i < A; i += WAVE) {
                const int vc = (int)(NS0[i] & NS_MASK);
                if (gs_valid(g, rm.st, i) && vc > bn) { bn = vc; bi = i; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const int on = __shfl_xor(bn, o), oi = __shfl_xor(bi, o);
                if (on > bn || (on == bn && oi < bi)) { bn = on; bi = oi; }
            }
            const int cs = __builtin_amdgcn_readfirstlane(bi);
            const int root_N = S->root_N;
            double pbc, sq; // what the next simulation of this root would read
            select_tab(cfg, B, root_N, pbc, sq);
            select_tab_fix(cfg, root_N, pbc, sq);
            const double *rprior = B.root_prior + (size_t)slot * g.AS;
            const float *W0 = reinterpret_cast<const float *>(node_ptr(pool, g, root) + META_DW + g.AS);
            long long cut = 0;
            if (bn >= 0) { // (a root without a valid child is terminal and never gets here)
                const double ustar = forced_ustar(pbc, sq, rprior[cs], W0[cs], NS0[cs]); // one address for the wave
                for (int i = lane; i < A; i += WAVE) {
                    const uint32_t ns = NS0[i];
                    const int vc = (int)(ns & NS_MASK);
                    int np = vc;
                    if (i != cs && vc > 0 && gs_valid(g, rm.st, i)) np = forced_pruned(cfg.forced_k, pbc, sq, root_N, rprior[i], W0[i], ns, ustar);
                    rv[i] = np;
                    cut += vc - np;
                }
            } else {
                for (int i = lane; i < A; i += WAVE) rv[i] = (int32_t)(NS0[i] & NS_MASK);
            }
            for (int o = 32; o > 0; o >>= 1) cut += __shfl_xor(cut, o);
            if (lane == 0) {
                atomicAdd((unsigned long long *)B.moves_played + 3, 1ull);
                atomicAdd((unsigned long long *)B.moves_played + 4, (unsigned long long)cut);
            }
        } else if (gumbel) {
            if (lane == 0) atomicAdd((unsigned long long *)B.moves_played + 6, 1ull); // (gumbel_finish wrote the visits)
        } else {
            for (int i = lane; i < A; i += WAVE) rv[i] = (int32_t)(NS0[i] & NS_MASK);
        }
        if (lane == 0) {
            RowMeta mm;
            mm.game_idx = (int32_t)S->game_idx;
            mm.move_idx = (int16_t)ply;
            mm.move = (int16_t)rm.move;
            mm.played = (int16_t)mv;
            mm.max_deepness = (int16_t)(S->max_deepness - S->deepness_correction);
            mm.tree_size = S->tree_size;
            mm.terminal_count = S->terminal_count;
            mm.q_value = S->root_W / (float)(1 + S->root_N); // TreeRoot.get_tree_stats, mcts.py:33-36
            mm.player = (int8_t)rm.st.to_play;
            mm.z = 0;
            mm.flags = ((kind & SEARCH_FAST) ? ROW_FLAG_FAST : 0) | (prune ? ROW_FLAG_PRUNED : 0) | (gumbel ? ROW_FLAG_GUMBEL | ((GUMBEL == 2 && (kind & SEARCH_GUMBEL_FULL)) ? ROW_FLAG_GUMBEL_FULL : 0) : 0);
            B.row_meta[(size_t)slot * rcap + r] = mm;
        }
        S->n_rows = r + 1;
    }
    __syncthreads();
    // ---- init_mcts_tree ----
    int err = reroot(g, B, slot, S, pool, mv, cfg.reuse_tree, lane, cfg.mcts_num_read + 2);
    if (err) {
        if (lane == 0) { S->error = err; S->phase = PH_ERROR; }
        return;
    }
    S->move_idx = ply + 1;
    if (lane == 0) atomicAdd((unsigned long long *)B.moves_played, 1ull);
    NodeMeta nm = load_meta(pool, g, S->root);
    if (nm.flags & NF_TERMINAL) { // (the self-play driver never reaches begin_search's terminal branch: the game ends here)
        endgame_release(sa, slot, S, lane);
        const bool emitted = try_emit(g, B, slot, S, pool, lane);
        if (lane == 0)
            S->phase = emitted ? PH_NEWGAME : PH_EMIT;
        return;
    }
    start_move_search<GUMBEL>(g, cfg, B, slot, S, pool, sa, ldsf, ldsd, lane);
}

// which slots need the driver: finished reads, a blocked emit or a finished game (the pass runs after the previous step's
// expand/backup).  One workgroup walks the slots in order: the list is in slot order, and the slots whose game ended take the
// next game indices (generate_games' chunking, self_play.py:291-306) in slot order, so that the same slot plays the same game on
// every run; a slot left without a game goes idle.
//
// The phase words lie one to a Slot, a cache line each: 8 192 of them through ONE compute unit cost more than the scan (31 us,
// all loads in flight, against 27 us for eight round trips).  So many small workgroups read them first -- k_driver_flags leaves
// every slot's class in drv_list[i], densely -- and the scan reads that.  Its compacted list goes into the same array: an
// entry's position is never behind its slot index, and a group's flags are all read before its first store.
#define DRV_NEEDS 1 // the slot needs the driver
#define DRV_FRESH 2 // ... and waits for a game index
__global__ void __launch_bounds__(WAVE) k_driver_flags(TreeBufs B, int n_slots)
{
    const int i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n_slots) return;
    const int phase = B.slots[i].phase;
    const bool fresh = phase == PH_NEWGAME;
    B.drv_list[i] = (phase == PH_EMIT || phase == PH_READY || fresh ? DRV_NEEDS : 0) | (fresh ? DRV_FRESH : 0);
}

template <int NG>
__global__ void __launch_bounds__(SCAN_T) k_driver_scan(SearchCfg cfg, TreeBufs B, int n_slots)
{
    __shared__ int s_pre[2 * NG * SCAN_W + 1];
    const int t = threadIdx.x;
    const long long next = *B.next_game;
    long long taken = 0;
    int base = 0;
    for (int g0 = 0; g0 < n_slots; g0 += SCAN_T * NG) {
        int cl[NG];
#pragma unroll
        for (int c = 0; c < NG; c++) {
            const int i = g0 + c * SCAN_T + t;
            cl[c] = i < n_slots ? B.drv_list[i] : 0;
        }
        unsigned fl[2] = {0u, 0u}; // needs the driver; of those, waits for a game
#pragma unroll
        for (int c = 0; c < NG; c++) {
            fl[0] |= (cl[c] & DRV_NEEDS ? 1u : 0u) << c;
            fl[1] |= (cl[c] & DRV_FRESH ? 1u : 0u) << c;
        }
        int rank[2][NG], tot[2];
        scan_ranks<2, NG>(s_pre, fl, rank, tot);
#pragma unroll
        for (int c = 0; c < NG; c++) {
            const int i = g0 + c * SCAN_T + t;
            if (fl[0] >> c & 1u) B.drv_list[base + rank[0][c]] = i;
            if (fl[1] >> c & 1u) {
                const long long gidx = next + taken + (long long)rank[1][c];
                Slot *S = B.slots + i;
                if (gidx < B.last_game) {
                    S->game_idx = gidx;
                } else {
                    S->game_idx = -1;
                    S->phase = PH_IDLE;
                }
            }
        }
        base += tot[0];
        taken += tot[1];
        if (g0 + SCAN_T * NG < n_slots) __syncthreads(); // s_pre is written again
    }
    if (t == 0) {
        B.drv_count[0] = base;
        *B.next_game = next + taken;
    }
}

template <int GUMBEL>
__global__ void __launch_bounds__(WAVE) k_advance_auto(Geo g, SearchCfg cfg, TreeBufs B, StartArgs sa)
{
    __shared__ float ldsf[DBAZ_MAX_A];
    __shared__ double ldsd[DBAZ_MAX_A];
    const int lane = threadIdx.x;
    const int n = *B.drv_count;
    for (int li = blockIdx.x; li < n; li += gridDim.x) {
        advance_one<GUMBEL>(g, cfg, B, B.drv_list[li], sa, ldsf, ldsd, lane);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------
// readback helpers + batched rules kernels (one thread per state)
// ------------------------------------------------------------------------------------
__global__ void k_get_roots(Geo g, TreeBufs B, int n_slots, double *priors, float *tv, int32_t *nv, int32_t *changed,
                            int32_t *stats, float *q, float *root_tv, int32_t *root_nv, uint64_t *edges,
                            int16_t *b2c2, int8_t *to_play, int8_t *just_played, int8_t *result, int8_t *expanded)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot >= n_slots) return;
    Slot *S = B.slots + slot;
    uint32_t *pool = B.nodes + (size_t)slot * g.cap * g.node_dw;
    NodeMeta rm = load_meta(pool, g, S->root);
    const uint32_t *nd = node_ptr(pool, g, S->root);
    const int A = g.A;
    for (int i = lane; i < A; i += WAVE) {
        uint32_t ns = nd[META_DW + 2 * g.AS + i];
        int c = (int)nd[META_DW + 3 * g.AS + i];
        if (priors) {
            double p;
            if (S->root_prepped) p = B.root_prior[(size_t)slot * g.AS + i];
            else p = is_inner(rm.flags)
                         ? (double)reinterpret_cast<const float *>(nd + META_DW)[i] : 0.0;
            priors[(size_t)slot * A + i] = p;
        }
        if (tv) tv[(size_t)slot * A + i] = reinterpret_cast<const float *>(nd + META_DW + g.AS)[i];
        if (nv) nv[(size_t)slot * A + i] = (int32_t)(ns & NS_MASK);
        if (changed) {
            // child_player_changed: 1 until the child is expanded, then +/-1 (mcts.py:61-62,119)
            int ch = 1;
            if (c >= 0) {
                NodeMeta cm = load_meta(pool, g, c);
                if (cm.flags & NF_EXPANDED) ch = (ns & NS_SAME) ? 1 : -1;
            }
            changed[(size_t)slot * A + i] = ch;
        }
    }
    if (lane == 0) {
        if (stats) {
            stats[slot * 3 + 0] = S->max_deepness - S->deepness_correction;
            stats[slot * 3 + 1] = S->tree_size;
            stats[slot * 3 + 2] = S->terminal_count;
        }
        if (q) q[slot] = S->root_W / (float)(1 + S->root_N);
        if (root_tv) root_tv[slot] = S->root_W;
        if (root_nv) root_nv[slot] = S->root_N;
        if (edges) {
            edges[slot * 4 + 0] = rm.st.e0; edges[slot * 4 + 1] = rm.st.e1;
            edges[slot * 4 + 2] = rm.st.e2; edges[slot * 4 + 3] = rm.st.e3;
        }
        if (b2c2) { b2c2[slot * 2] = (int16_t)rm.st.b2c0; b2c2[slot * 2 + 1] = (int16_t)rm.st.b2c1; }
        if (to_play) to_play[slot] = (int8_t)rm.st.to_play;
        if (just_played) just_played[slot] = (int8_t)rm.st.just_played;
        if (result) result[slot] = (int8_t)gs_result(rm.st);
        if (expanded) expanded[slot] = (rm.flags & NF_EXPANDED) ? 1 : 0;
    }
}

__global__ void k_get_leaves(Geo g, TreeBufs B, int n_slots, int16_t *leaf_x, uint8_t *need_eval, int32_t *n_active)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    Slot *S = B.slots + slot;
    const bool active = S->phase == PH_EXPAND_ROOT || S->phase == PH_SIMS;
    const bool need = active && !S->leaf_terminal;
    const int F = 3 * g.HW;
    const float *f = B.feat + (size_t)slot * F;
    for (int i = lane; i < F; i += WAVE)
        leaf_x[(size_t)slot * F + i] = need ? (int16_t)f[i] : (int16_t)0;
    if (lane == 0) {
        need_eval[slot] = need ? 1 : 0;
        if (active) atomicAdd(n_active, 1);
    }
}

// Slot array -> SlotSummary (out must be zeroed except first_error_slot = 0x7fffffff)
__global__ void __launch_bounds__(256) k_slot_summary(TreeBufs B, int n_slots, SlotSummary *out)
{
    unsigned long long ns = 0, ne = 0, nh = 0, nt = 0, sp = 0, nr = 0;
    int active = 0, error = 0, blocked = 0, high = 0, ferr = 0x7fffffff;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += gridDim.x * blockDim.x) {
        const Slot &S = B.slots[i];
        ns += (unsigned long long)S.n_search; ne += (unsigned long long)S.n_eval; nh += (unsigned long long)S.n_hit;
        nt += (unsigned long long)S.n_term; sp += (unsigned long long)S.sum_path; nr += (unsigned long long)S.pool_resets;
        const int ph = S.phase;
        if (ph == PH_ERROR) { error++; ferr = min(ferr, i); }
        else if (S.game_idx >= 0 && ph != PH_IDLE) active++;
        if (ph == PH_EMIT) blocked++;
        high = max(high, S.pool_high);
    }
    for (int o = 32; o > 0; o >>= 1) {
        ns += __shfl_xor(ns, o); ne += __shfl_xor(ne, o); nh += __shfl_xor(nh, o); nt += __shfl_xor(nt, o); sp += __shfl_xor(sp, o);
        nr += __shfl_xor(nr, o);
        active += __shfl_xor(active, o); error += __shfl_xor(error, o); blocked += __shfl_xor(blocked, o);
        high = max(high, __shfl_xor(high, o)); ferr = min(ferr, __shfl_xor(ferr, o));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        atomicAdd(&out->n_search, ns); atomicAdd(&out->n_eval, ne); atomicAdd(&out->n_hit, nh); atomicAdd(&out->n_term, nt);
        atomicAdd(&out->sum_path, sp); atomicAdd(&out->n_reset, nr);
        atomicAdd(&out->active, active); atomicAdd(&out->error, error); atomicAdd(&out->blocked, blocked);
        atomicMax(&out->pool_high, high);
        if (ferr != 0x7fffffff) atomicMin(&out->first_error_slot, ferr);
    }
}
// second pass (only when an error was seen): the code of the lowest failing slot
__global__ void k_slot_error_code(TreeBufs B, SlotSummary *out)
{
    if (out->first_error_slot != 0x7fffffff) out->first_error_code = B.slots[out->first_error_slot].error;
}

// wall-clock cut-off of UCT_search (mcts.py:232-233): the reads that were not started are dropped
__global__ void k_stop_search(TreeBufs B, int n_slots)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    Slot *S = B.slots + i;
    if (S->phase == PH_SIMS) { S->sims_left = 0; S->phase = PH_READY; }
}

__global__ void k_count_active(TreeBufs B, int n_slots, int32_t *out /*[3]: searching, ready, error*/)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ph = i < n_slots ? B.slots[i].phase : PH_IDLE;
    // one atomic per wave and class (same-address atomics serialise)
    const unsigned long long m0 = __ballot(ph == PH_EXPAND_ROOT || ph == PH_SIMS);
    const unsigned long long m1 = __ballot(ph == PH_READY || ph == PH_EMIT);
    const unsigned long long m2 = __ballot(ph == PH_ERROR);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (m0) atomicAdd(out + 0, (int)__popcll(m0));
        if (m1) atomicAdd(out + 1, (int)__popcll(m1));
        if (m2) atomicAdd(out + 2, (int)__popcll(m2));
    }
}

__global__ void k_rules(Geo g, int op, int n, uint64_t *edges, int16_t *b2c2, int8_t *to_play, int8_t *just_played,
                        const int32_t *moves, int8_t *n_closed, int8_t *closed_lc, uint8_t *valid, int8_t *result,
                        int16_t *x)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    GState s;
    gs_init(g, s);
    if (op != 0) {
        if (edges) { s.e0 = edges[4 * i]; s.e1 = edges[4 * i + 1]; s.e2 = edges[4 * i + 2]; s.e3 = edges[4 * i + 3]; }
        if (b2c2) { s.b2c0 = b2c2[2 * i]; s.b2c1 = b2c2[2 * i + 1]; }
        if (to_play) s.to_play = to_play[i];
        if (just_played) s.just_played = just_played[i];
    }
    bool wb = false;
    switch (op) {
    case 0: wb = true; break;                                  // __init__
    case 1:                                                    // get_valid_moves
        for (int k = 0; k < g.A; k++) valid[(size_t)i * g.A + k] = gs_valid(g, s, k) ? 1 : 0;
        break;
    case 2: {                                                  // play_
        int cl[4] = {-1, -1, -1, -1};
        int r = gs_play(g, s, moves[i], cl);
        n_closed[i] = (int8_t)r;
        if (closed_lc) for (int k = 0; k < 4; k++) closed_lc[4 * i + k] = (int8_t)((r > 0 && k < 2 * r) ? cl[k] : -1);
        wb = r >= 0;
        break;
    }
    case 3: result[i] = (int8_t)gs_result(s); break;           // get_result
    case 4:                                                    // get_features
        for (int k = 0; k < 3 * g.HW; k++) x[(size_t)i * 3 * g.HW + k] = (int16_t)gs_feature(g, s, k);
        break;
    }
    if (wb) {
        edges[4 * i] = s.e0; edges[4 * i + 1] = s.e1; edges[4 * i + 2] = s.e2; edges[4 * i + 3] = s.e3;
        b2c2[2 * i] = (int16_t)s.b2c0; b2c2[2 * i + 1] = (int16_t)s.b2c1;
        to_play[i] = (int8_t)s.to_play;
        just_played[i] = (int8_t)s.just_played;
    }
}

// ------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------
void tree_launch_search_begin(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots,
                              const int32_t *num_reads_dev, StartArgs sa)
{
    hipLaunchKernelGGL(k_search_begin, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, num_reads_dev, sa);
}
template <int GUMBEL>
static void launch_select(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, const EndgameBufs &G)
{
    const int npl = (g.A + WAVE - 1) / WAVE;
    if (c.eval_round > 0) { // k_order_evals writes the network's list: one game per workgroup
        switch (npl) {
        case 1: hipLaunchKernelGGL((k_select<1, true, GUMBEL>), dim3(n_slots), dim3(WAVE), 0, s, g, c, B, n_slots, G); break;
        case 2: hipLaunchKernelGGL((k_select<2, true, GUMBEL>), dim3(n_slots), dim3(WAVE), 0, s, g, c, B, n_slots, G); break;
        case 3: hipLaunchKernelGGL((k_select<3, true, GUMBEL>), dim3(n_slots), dim3(WAVE), 0, s, g, c, B, n_slots, G); break;
        default: hipLaunchKernelGGL((k_select<4, true, GUMBEL>), dim3(n_slots), dim3(WAVE), 0, s, g, c, B, n_slots, G); break;
        }
        return;
    }
    const dim3 grid((n_slots + SELECT_WAVES - 1) / SELECT_WAVES), block(WAVE * SELECT_WAVES);
    switch (npl) {
    case 1: hipLaunchKernelGGL((k_select<1, false, GUMBEL>), grid, block, 0, s, g, c, B, n_slots, G); break;
    case 2: hipLaunchKernelGGL((k_select<2, false, GUMBEL>), grid, block, 0, s, g, c, B, n_slots, G); break;
    case 3: hipLaunchKernelGGL((k_select<3, false, GUMBEL>), grid, block, 0, s, g, c, B, n_slots, G); break;
    default: hipLaunchKernelGGL((k_select<4, false, GUMBEL>), grid, block, 0, s, g, c, B, n_slots, G); break;
    }
}
void tree_launch_select(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, const EndgameBufs &G)
{
    // a handle with the Gumbel rule on launches the instantiations that hold its root pre-pass (in the full mode, those that hold the
    // rule below the root too); every other handle the ones without
    if (gumbel_level(c) == 2) launch_select<2>(s, g, c, B, n_slots, G);
    else if (gumbel_level(c) == 1) launch_select<1>(s, g, c, B, n_slots, G);
    else launch_select<0>(s, g, c, B, n_slots, G);
}
void tree_launch_select_multi(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, const EndgameBufs &G)
{
    switch ((g.A + WAVE - 1) / WAVE) {
    case 1: hipLaunchKernelGGL(k_select_multi<1>, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, n_slots, G); break;
    case 2: hipLaunchKernelGGL(k_select_multi<2>, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, n_slots, G); break;
    case 3: hipLaunchKernelGGL(k_select_multi<3>, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, n_slots, G); break;
    default: hipLaunchKernelGGL(k_select_multi<4>, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, n_slots, G); break;
    }
}
void tree_launch_expand_backup_multi(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, const EndgameBufs &G)
{
    hipLaunchKernelGGL(k_expand_backup_multi, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, G);
}
void tree_launch_expand_backup(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, const EndgameBufs &G)
{
    // (a handle with the Gumbel rule on launches the instantiations that hold it; every other handle the ones without a trace of it)
    if (gumbel_level(c) == 2) hipLaunchKernelGGL(k_expand_backup<2>, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, G);
    else if (gumbel_level(c) == 1) hipLaunchKernelGGL(k_expand_backup<1>, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, G);
    else hipLaunchKernelGGL(k_expand_backup<0>, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, G);
}
void tree_launch_set_positions(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots,
                               const int16_t *moves_dev, const int32_t *offsets_dev)
{
    hipLaunchKernelGGL(k_set_positions, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, moves_dev, offsets_dev);
}
void tree_launch_advance_manual(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots,
                                const int32_t *moves_dev, int reuse)
{
    hipLaunchKernelGGL(k_advance_manual, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, moves_dev, reuse);
}
void tree_launch_selfplay_start(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, StartArgs sa)
{
    // (the start of a search is the same in both modes of the rule)
    if (gumbel_level(c) > 0) hipLaunchKernelGGL(k_selfplay_start<1>, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, sa);
    else hipLaunchKernelGGL(k_selfplay_start<0>, dim3(n_slots), dim3(WAVE), 0, s, g, c, B, sa);
}
void tree_launch_order_evals(hipStream_t s, const TreeBufs &B, int n_slots, int step)
{
    const int rot = (int)(((unsigned long long)(unsigned)step * 2654435761ull) % (unsigned long long)n_slots);
    if (n_slots <= SCAN_T * SCAN_NG_SMALL) hipLaunchKernelGGL(k_order_evals<SCAN_NG_SMALL>, dim3(1), dim3(SCAN_T), 0, s, B, n_slots, rot);
    else hipLaunchKernelGGL(k_order_evals<SCAN_NG>, dim3(1), dim3(SCAN_T), 0, s, B, n_slots, rot);
}
void tree_launch_advance_auto(hipStream_t s, const Geo &g, const SearchCfg &c, const TreeBufs &B, int n_slots, StartArgs sa)
{
    hipLaunchKernelGGL(k_driver_flags, dim3((n_slots + WAVE - 1) / WAVE), dim3(WAVE), 0, s, B, n_slots);
    if (n_slots <= SCAN_T * SCAN_NG_SMALL) hipLaunchKernelGGL(k_driver_scan<SCAN_NG_SMALL>, dim3(1), dim3(SCAN_T), 0, s, c, B, n_slots);
    else hipLaunchKernelGGL(k_driver_scan<SCAN_NG>, dim3(1), dim3(SCAN_T), 0, s, c, B, n_slots);
    if (gumbel_level(c) == 2) hipLaunchKernelGGL(k_advance_auto<2>, dim3(n_slots < 1024 ? n_slots : 1024), dim3(WAVE), 0, s, g, c, B, sa);
    else if (gumbel_level(c) == 1) hipLaunchKernelGGL(k_advance_auto<1>, dim3(n_slots < 1024 ? n_slots : 1024), dim3(WAVE), 0, s, g, c, B, sa);
    else hipLaunchKernelGGL(k_advance_auto<0>, dim3(n_slots < 1024 ? n_slots : 1024), dim3(WAVE), 0, s, g, c, B, sa);
}
void tree_launch_get_roots(hipStream_t s, const Geo &g, const TreeBufs &B, int n_slots, double *priors, float *tv,
                           int32_t *nv, int32_t *changed, int32_t *stats, float *q, float *root_tv, int32_t *root_nv,
                           uint64_t *edges, int16_t *b2c2, int8_t *to_play, int8_t *just_played, int8_t *result,
                           int8_t *expanded)
{
    hipLaunchKernelGGL(k_get_roots, dim3(n_slots), dim3(WAVE), 0, s, g, B, n_slots, priors, tv, nv, changed, stats, q,
                       root_tv, root_nv, edges, b2c2, to_play, just_played, result, expanded);
}
void tree_launch_get_leaves(hipStream_t s, const Geo &g, const TreeBufs &B, int n_slots, int16_t *leaf_x,
                            uint8_t *need_eval, int32_t *n_active)
{
    hipLaunchKernelGGL(k_get_leaves, dim3(n_slots), dim3(WAVE), 0, s, g, B, n_slots, leaf_x, need_eval, n_active);
}
void tree_launch_stop_search(hipStream_t s, const TreeBufs &B, int n_slots)
{
    hipLaunchKernelGGL(k_stop_search, dim3((n_slots + 255) / 256), dim3(256), 0, s, B, n_slots);
}
void tree_launch_count_active(hipStream_t s, const TreeBufs &B, int n_slots, int32_t *out3)
{
    hipLaunchKernelGGL(k_count_active, dim3((n_slots + 255) / 256), dim3(256), 0, s, B, n_slots, out3);
}
void tree_launch_slot_summary(hipStream_t s, const TreeBufs &B, int n_slots, SlotSummary *out_dev)
{
    int blocks = (n_slots + 255) / 256;
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(k_slot_summary, dim3(blocks), dim3(256), 0, s, B, n_slots, out_dev);
    hipLaunchKernelGGL(k_slot_error_code, dim3(1), dim3(1), 0, s, B, out_dev);
}
void tree_launch_rules(hipStream_t s, const Geo &g, int op, int n, uint64_t *edges, int16_t *b2c2, int8_t *to_play,
                       int8_t *just_played, const int32_t *moves, int8_t *n_closed, int8_t *closed_lc, uint8_t *valid,
                       int8_t *result, int16_t *x)
{
    hipLaunchKernelGGL(k_rules, dim3((n + 127) / 128), dim3(128), 0, s, g, op, n, edges, b2c2, to_play, just_played,
                       moves, n_closed, closed_lc, valid, result, x);
}
