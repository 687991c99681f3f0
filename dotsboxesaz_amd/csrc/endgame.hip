// endgame.hip -- exact endgame solver for ANY board the engine supports (A <= 256): a position with F <= 16 free edges is a game
// over the 2^F subsets of those edges, and one workgroup solves it in LDS.  No solve step, no dbaz_engine, no
// search or network code: the engine reaches the evaluator kernels below through the four functions at the end (endgame.h).
//
// k_endgame_score, one workgroup per feature row x int16 [3*HW] (planes 0, 1: edges; plane 2: the mover's doubled boxes_to_close):
//   1. setup: lane i < E looks at real edge i; the free ones are ranked in ascending action order (ballot + per-wave counts):
//      compact edge j = the j-th free real edge.  Every compact edge gets the "other" masks of solver_move_q over the COMPACT
//      edges: per bordering box the other edges that are still free (0: the edge completes that box whatever else is drawn;
//      SOLVER_NO_BOX: no such box).  The closed boxes are counted from planes 0 / 1.
//   2. solve: D[mask] of solver.hip over the 2^F masks of the compact edges, popcount layers F .. 0, one barrier each; the masks
//      of a layer come from the popcount-sorted list of F bits (built on the host at handle creation), so every lane has a state.
//   3. outputs with dbaz_solver_score's meaning, plus n_free.
// k_endgame_policy: steps 1 and 2, then a one-hot optimal move and the true value per row (dbaz_exact_policy).
// k_endgame_table / k_endgame_eval: a search root's table kept per slot in HBM, and the leaves of that game answered from it.
// k_endgame_candidates / k_endgame_list / k_endgame_targets: exact training targets (dbaz_exact_targets): the rows with
//   F <= max_free listed deepest first, then steps 1 and 2 per listed row and the solved z and pi written in place.
#include <algorithm>
#include <string>
#include <vector>

#include "endgame.h"
#include "table_row.h"

// counters of one dbaz_exact_targets call (device): rows per F <= max_free, the append cursors of k_endgame_list, and the
// statistics of the dataset form -- [0] finished rows left alone, [1] rows whose z differed from v, [2 + F] rows relabelled
struct TargetCounters {
    uint32_t hist[ENDGAME_MAX_FREE + 1];
    uint32_t cursor[ENDGAME_MAX_FREE + 1];
    unsigned long long stats[ENDGAME_MAX_FREE + 3];
};

struct dbaz_endgame {
    EndgameGeo g;
    int dev = 0;
    void *bufs[4] = {nullptr, nullptr, nullptr, nullptr}; // action, nbr, perm, off
    // scratch of dbaz_exact_targets, grown on demand: the candidate list and n_free per row; the counters
    int32_t *tg_list = nullptr;
    int16_t *tg_nfree = nullptr;
    size_t tg_cap = 0;
    TargetCounters *tg_cnt = nullptr;
    std::string err;
};

static thread_local std::string g_endgame_error; // message of a failed dbaz_endgame_create; per thread

// ------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------
#define ENDGAME_TABLE_GRID 1024 // workgroups of k_endgame_table: four rounds of the chip at two per CU

// static LDS of one workgroup, next to the dynamic int8 table [2^max_free]
struct EndgameLds {
    int16_t cidx[DBAZ_MAX_A];               // action -> compact edge, -1: drawn or a sentinel slot
    uint32_t other[ENDGAME_MAX_FREE][2];
    uint8_t act[ENDGAME_MAX_FREE];          // compact edge -> action
    int wave[DBAZ_MAX_A / 64];
    int closed;
};

// step 1 of the header comment for one position; returns F, the same in every thread.  F > g.max_free: nothing but F is valid
// (the caller returns; no thread is left behind a barrier).  Otherwise L is complete and visible to the whole workgroup.
// drawn(a): is the edge (or sentinel slot) of action index a drawn -- a feature row, or the free-edge mask of a search root
struct RowEdges {
    const int16_t *xr;
    __device__ __forceinline__ bool operator()(int a) const { return xr[a] != 0; }
};
template <typename T>
struct PlaneEdges { // T = float: the search's feature planes (TreeBufs.feat)
    const T *xr;
    __device__ __forceinline__ bool operator()(int a) const { return xr[a] != (T)0; }
};
struct MaskEdges {
    uint64_t free_edges[4];
    __device__ __forceinline__ bool operator()(int a) const { return !((free_edges[a >> 6] >> (a & 63)) & 1ull); }
};

// THREADS: the workgroup's size, at least one lane per action slot
template <typename Edges, int THREADS = ENDGAME_THREADS>
static __device__ __forceinline__ int endgame_setup(const EndgameGeo &g, const Edges &drawn, EndgameLds &L)
{
    static_assert(THREADS >= DBAZ_MAX_A && THREADS % 64 == 0, "one lane per action slot");
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < DBAZ_MAX_A) L.cidx[tid] = -1;
    if (tid == 0) L.closed = 0;
    const int a_mine = tid < g.E ? (int)g.action[tid] : 0;
    const bool is_free = tid < g.E && !drawn(a_mine);
    const uint64_t bal = __ballot(is_free);
    if (tid < DBAZ_MAX_A && lane == 0) L.wave[tid >> 6] = __popcll(bal);
    __syncthreads();
    int F = 0, before = 0;
    for (int w = 0; w < DBAZ_MAX_A / 64; w++) {
        F += L.wave[w];
        if (w < (tid >> 6)) before += L.wave[w];
    }
    if (F > g.max_free) return F;
    const int j = before + __popcll(bal & ((1ull << lane) - 1ull));
    if (is_free) {
        L.cidx[a_mine] = (int16_t)j;
        L.act[j] = (uint8_t)a_mine;
    }
    const int W = g.cols + 1, B = g.rows * g.cols;
    for (int b = tid; b < B; b += THREADS) {
        const int at = (b / g.cols) * W + b % g.cols;
        if (drawn(at) && drawn(at + W) && drawn(g.HW + at) && drawn(g.HW + at + 1)) atomicAdd(&L.closed, 1);
    }
    __syncthreads();
    if (is_free)
        for (int k = 0; k < 2; k++) {
            const int16_t *nb = g.nbr + (tid * 2 + k) * 3;
            uint32_t o = SOLVER_NO_BOX;
            if (nb[0] >= 0) {
                o = 0;
                for (int i = 0; i < 3; i++) {
                    const int c = L.cidx[nb[i]];
                    if (c >= 0) o |= 1u << c;
                }
            }
            L.other[j][k] = o;
        }
    __syncthreads();
    return F;
}

// step 2: the subgame of the F compact edges into sd[2^F], by popcount layers; the box masks are the same for every lane: keep
// them in scalar registers.  Ends behind a barrier: sd is complete for the whole workgroup.
template <int THREADS = ENDGAME_THREADS>
static __device__ __forceinline__ void endgame_solve(const EndgameGeo &g, int F, const EndgameLds &L, int8_t *sd)
{
    const int tid = threadIdx.x;
    uint32_t o0[ENDGAME_MAX_FREE], o1[ENDGAME_MAX_FREE];
#pragma unroll
    for (int b = 0; b < ENDGAME_MAX_FREE; b++) {
        o0[b] = b < F ? __builtin_amdgcn_readfirstlane(L.other[b][0]) : SOLVER_NO_BOX;
        o1[b] = b < F ? __builtin_amdgcn_readfirstlane(L.other[b][1]) : SOLVER_NO_BOX;
    }
    const uint32_t full = (1u << F) - 1u;
    const uint16_t *list = g.perm + full;
    const uint32_t *off = g.off + F * ENDGAME_OFF_STRIDE;
    for (int k = F; k >= 0; k--) {
        const uint32_t end = off[k + 1];
        for (uint32_t i = off[k] + tid; i < end; i += THREADS) {
            const uint32_t low = list[i];
            int best = -128;
#pragma unroll
            for (int b = 0; b < ENDGAME_MAX_FREE; b++) {
                if (b >= F) break;
                const uint32_t bit = 1u << b;
                const int qq = solver_move_q(o0[b], o1[b], low, (int)sd[low | bit]); // a drawn b reads sd[low]: unused
                best = (low & bit) ? best : max(best, qq);
            }
            sd[low] = (int8_t)(low == full ? 0 : best);
        }
        __syncthreads();
    }
}

// endgame_pick, the evaluator's epilogue (one wavefront per position, lane = one compact edge): solver.h

__global__ void __launch_bounds__(ENDGAME_THREADS) k_endgame_score(EndgameGeo g, const int16_t *__restrict__ x, const float *__restrict__ pi,
                                                                   int8_t *__restrict__ value, int8_t *__restrict__ diff,
                                                                   int8_t *__restrict__ q, float *__restrict__ mass,
                                                                   int16_t *__restrict__ n_free)
{
    extern __shared__ __attribute__((aligned(16))) int8_t sd[]; // [2^max_free]
    __shared__ EndgameLds L;

    const int tid = threadIdx.x;
    const size_t r = blockIdx.x;
    const int16_t *xr = x + r * 3 * (size_t)g.HW;

    const int F = endgame_setup(g, RowEdges{xr}, L);
    int8_t *qr = q + r * (size_t)g.A;
    if (F > g.max_free) { // not solved: n_free says why
        for (int a = tid; a < g.A; a += ENDGAME_THREADS) qr[a] = -128;
        if (tid == 0) {
            value[r] = 0;
            diff[r] = -128;
            if (mass) mass[r] = 0.0f;
            n_free[r] = (int16_t)F;
        }
        return;
    }
    endgame_solve(g, F, L, sd);

    // 3. outputs
    const RowFacts f = solver_facts(g.rows * g.cols, L.closed, (int)xr[2 * g.HW]);
    const bool open = f.res == DBAZ_RESULT_NONE;
    const int d0 = (int)sd[0];
    const int v = open ? sgn(f.margin + d0) : f.res;
    for (int a = tid; a < g.A; a += ENDGAME_THREADS) {
        const int c = L.cidx[a];
        qr[a] = (int8_t)(open && c >= 0 ? solver_move_q(L.other[c][0], L.other[c][1], 0u, (int)sd[1u << c]) : -128);
    }
    if (tid == 0) {
        value[r] = (int8_t)v;
        diff[r] = (int8_t)d0;
        n_free[r] = (int16_t)F;
        if (mass) {
            float sum = 0.0f;
            for (int c = 0; open && c < F; c++) { // ascending action order
                const int qq = solver_move_q(L.other[c][0], L.other[c][1], 0u, (int)sd[1u << c]);
                if (sgn(f.margin + qq) == v) sum += pi[r * (size_t)g.A + L.act[c]];
            }
            mass[r] = sum;
        }
    }
}

// The solver as a (p, v) evaluator, every row solved from scratch (the counterpart of k_solver_eval without a table): one
// workgroup per row, k_endgame_score's setup and solve, then wave 0 picks with lane j = compact edge j.  p [n][A]: one-hot on the
// pick; v = sign(margin + D[0]).  A finished game: p = 0, v = get_result.  F > max_free: p = 0, v = 0, solved = 0.
__global__ void __launch_bounds__(ENDGAME_THREADS) k_endgame_policy(EndgameGeo g, const int16_t *__restrict__ x, uint64_t pick_seed,
                                                                    float *__restrict__ P, float *__restrict__ V,
                                                                    uint8_t *__restrict__ solved)
{
    extern __shared__ __attribute__((aligned(16))) int8_t sd[]; // [2^max_free]
    __shared__ EndgameLds L;
    __shared__ int s_pick;

    const int tid = threadIdx.x;
    const size_t r = blockIdx.x;
    const int16_t *xr = x + r * 3 * (size_t)g.HW;
    float *pr = P + r * (size_t)g.A;

    const int F = endgame_setup(g, RowEdges{xr}, L);
    if (F > g.max_free) {
        for (int a = tid; a < g.A; a += ENDGAME_THREADS) pr[a] = 0.0f;
        if (tid == 0) {
            V[r] = 0.0f;
            solved[r] = 0;
        }
        return;
    }
    endgame_solve(g, F, L, sd);

    const RowFacts f = solver_facts(g.rows * g.cols, L.closed, (int)xr[2 * g.HW]);
    const bool open = f.res == DBAZ_RESULT_NONE;
    if (tid < 64) {
        const bool cand = open && tid < F;
        const int qq = cand ? solver_move_q(L.other[tid][0], L.other[tid][1], 0u, (int)sd[1u << tid]) : 0;
        const int pick = endgame_pick(cand, qq, cand ? (int)L.act[tid] : 0, pick_seed);
        if (tid == 0) s_pick = pick;
    }
    __syncthreads();
    const int pick = s_pick;
    for (int a = tid; a < g.A; a += ENDGAME_THREADS) pr[a] = a == pick ? 1.0f : 0.0f;
    if (tid == 0) {
        V[r] = (float)(open ? sgn(f.margin + (int)sd[0]) : f.res);
        solved[r] = 1;
    }
}

// One game's table for the search (endgame.h): one workgroup per slot that needs a table.  The grid is at most
// ENDGAME_TABLE_GRID workgroups, each looking at the slots blockIdx.x, + gridDim.x, ...: a slot without a request costs one word
// read (a workgroup holds 64 KB of LDS, so one workgroup per idle slot would go through the chip in many rounds).  A request is
// kept, dropped or solved by slot_request_rule (endgame.h); a solved one is k_endgame_score's setup and solve, and goes from LDS
// to the slot's region in 16-byte stores together with the header.
__global__ void __launch_bounds__(ENDGAME_THREADS) k_endgame_table(EndgameGeo g, EndgameReq *__restrict__ req, EndgameSlotHdr *__restrict__ hdr,
                                                                   int8_t *__restrict__ tables, size_t stride, int n_slots,
                                                                   unsigned long long *__restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) int8_t sd[]; // [max(16, 2^max_free)]
    __shared__ EndgameLds L;

    const int tid = threadIdx.x;
    for (size_t slot = blockIdx.x; slot < (size_t)n_slots; slot += gridDim.x) {
    EndgameReq *rq = req + slot;
    EndgameSlotHdr *h = hdr + slot;
    if (!*(volatile const int32_t *)&rq->want) continue; // the same answer in every thread: nobody has written yet
    MaskEdges me;
    for (int w = 0; w < 4; w++) me.free_edges[w] = rq->free_edges[w];
    const int64_t game = rq->game;
    const int model = rq->model;
    const SlotDecision d = slot_request_rule(me.free_edges, h->valid, h->game, h->free_edges, game, g.max_free);
    const int F = d.F;
    __syncthreads(); // every thread has read the request and the header
    if (tid == 0) {
        rq->want = 0;
        h->model = model;
        if (!d.keep && !d.solve) h->valid = 0;
    }
    if (!d.solve) continue;

    endgame_setup(g, me, L);
    endgame_solve(g, F, L, sd);

    const int n16 = max(1, (1 << F) >> 4);
    uint4 *dst = reinterpret_cast<uint4 *>(tables + slot * stride);
    const uint4 *src = reinterpret_cast<const uint4 *>(sd);
    for (int i = tid; i < n16; i += ENDGAME_THREADS) dst[i] = src[i];
    if (tid < F) {
        h->other[tid][0] = L.other[tid][0];
        h->other[tid][1] = L.other[tid][1];
        h->act[tid] = L.act[tid];
    }
    if (tid == 0) {
        for (int w = 0; w < 4; w++) h->free_edges[w] = me.free_edges[w];
        h->game = game;
        h->F0 = F;
        h->table = (int32_t)slot;
        h->valid = 1;
        atomicAdd(stats, 1ull);
    }
    __syncthreads(); // the next slot of this workgroup reuses L and sd
    }
}

// requests for k_endgame_table from feature rows (dbaz_exact_policy_from): one thread per root row
__global__ void k_endgame_requests(EndgameGeo g, const int16_t *__restrict__ x, int n, EndgameReq *__restrict__ req)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int16_t *xr = x + (size_t)r * 3 * g.HW;
    EndgameReq rq;
    for (int w = 0; w < 4; w++) rq.free_edges[w] = 0ull;
    for (int i = 0; i < g.E; i++) {
        const int a = (int)g.action[i];
        if (xr[a] == 0) rq.free_edges[a >> 6] |= 1ull << (a & 63);
    }
    rq.game = r;
    rq.want = 1;
    rq.model = 0;
    req[r] = rq;
}

// A slot's table as a (p, v) evaluator with k_solver_eval's contract: rows x[list[j]], j < min(*n_dev, max_n), of slot
// list[j] / per_slot; T = float (TreeBufs.feat planes) or int16.  One wavefront per row, table_row (table_row.h) against the
// slot's header and table, without the served check: the caller lists only rows the header serves.  endgame_pick names the
// move; v = sign(margin + T[mask]).  A finished position gets p = 0 and v = get_result; a row of a slot without a valid table
// p = 0, v = 0.
#define ENDGAME_EVAL_WAVES 4
template <typename T>
__global__ void __launch_bounds__(64 * ENDGAME_EVAL_WAVES) k_endgame_eval(TablesBoard B, int max_free, const EndgameSlotHdr *__restrict__ hdr,
                                                                          const int8_t *__restrict__ tables, size_t tab_stride, int n_tables,
                                                                          const T *__restrict__ x, const int32_t *__restrict__ list,
                                                                          const int32_t *__restrict__ n_dev, int max_n, int per_slot,
                                                                          uint64_t seed0, uint64_t seed1, float *__restrict__ P,
                                                                          float *__restrict__ V, int stride, unsigned long long *__restrict__ stats)
{
    const int lane = threadIdx.x & 63;
    const int n = n_dev ? min(*n_dev, max_n) : max_n;
    if (stats && blockIdx.x == 0 && threadIdx.x == 0 && n > 0) atomicAdd(stats + 1, (unsigned long long)n);
    for (int j = blockIdx.x * ENDGAME_EVAL_WAVES + (threadIdx.x >> 6); j < n; j += gridDim.x * ENDGAME_EVAL_WAVES) {
        const int r = list ? list[j] : j;
        if ((unsigned)r >= (unsigned)max_n) continue; // never outside the caller's buffers
        const size_t slot = (size_t)(r / per_slot);
        const EndgameSlotHdr *h = hdr + slot;
        float *pr = P + (size_t)r * stride;
        const int table = h->table;
        // no table (the engine never lists such a leaf; dbaz_exact_policy_from: a root with F > max_free), and never outside the regions
        if (!h->valid || (unsigned)table >= (unsigned)n_tables) {
            for (int i = lane; i < stride; i += 64) pr[i] = 0.0f;
            if (lane == 0) V[r] = 0.0f;
            continue;
        }
        const int8_t *Tb = tables + (size_t)table * tab_stride;
        const TableRow d = table_row<false>(B, *h, min(h->F0, max_free), Tb, x + (size_t)r * 3 * B.HW, lane);
        const int pick = endgame_pick(d.cand, d.q, d.a, h->model ? seed1 : seed0);
        for (int i = lane; i < stride; i += 64) pr[i] = i == pick ? 1.0f : 0.0f;
        if (lane == 0) V[r] = (float)(d.open ? sgn(d.f.margin + (int)Tb[d.m]) : d.f.res);
    }
}

// ---- exact training targets (dbaz_exact_targets) --------------------------------------------------------------
// Most rows of a training window have F > max_free and the rest have F spread over 0 .. max_free, so the rows are sorted out
// before anything is solved.  k_endgame_candidates, one wavefront per row and no table: F from the edge planes, n_free and the
// "untouched" side outputs of every row, and the histogram of the F <= max_free (per workgroup in LDS, then one atomic per
// occupied bin).  x_stride: shorts between two rows (3*HW for dense rows, the dataset's padded rows are further apart).
#define ENDGAME_CAND_WAVES 4
__global__ void __launch_bounds__(64 * ENDGAME_CAND_WAVES) k_endgame_candidates(EndgameGeo g, const int16_t *__restrict__ x, int x_stride, int n,
                                                                                int16_t *__restrict__ n_free, float *__restrict__ mass,
                                                                                uint8_t *__restrict__ relabelled, TargetCounters *__restrict__ cnt)
{
    __shared__ uint32_t s_hist[ENDGAME_MAX_FREE + 1];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x <= ENDGAME_MAX_FREE) s_hist[threadIdx.x] = 0;
    __syncthreads();
    for (int r = blockIdx.x * ENDGAME_CAND_WAVES + (threadIdx.x >> 6); r < n; r += gridDim.x * ENDGAME_CAND_WAVES) {
        const int16_t *xr = x + (size_t)r * x_stride;
        int F = 0;
        for (int i0 = 0; i0 < g.E; i0 += 64) {
            const int i = i0 + lane;
            F += __popcll(__ballot(i < g.E && xr[g.action[i]] == 0));
        }
        if (lane == 0) {
            n_free[r] = (int16_t)F;
            if (mass) mass[r] = 0.0f;
            if (relabelled) relabelled[r] = 0;
            if (F <= g.max_free) atomicAdd(&s_hist[F], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x <= ENDGAME_MAX_FREE && s_hist[threadIdx.x]) atomicAdd(&cnt->hist[threadIdx.x], s_hist[threadIdx.x]);
}

// The candidate list from n_free and the finished histogram: the rows with F <= max_free, deepest first (bucket F starts behind
// the rows of every deeper bucket).  One thread per row; the lanes of a wavefront that share an F take their places with one
// atomic.  The order inside a bucket is whatever the atomics give: every row is relabelled on its own, so no output depends on it.
__global__ void __launch_bounds__(256) k_endgame_list(int max_free, int n, const int16_t *__restrict__ n_free, TargetCounters *__restrict__ cnt,
                                                      int32_t *__restrict__ list)
{
    const int r = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int F = r < n ? (int)n_free[r] : max_free + 1;
    uint32_t start = 0; // of bucket f while the loop goes down
    for (int f = max_free; f >= 0; f--) {
        const uint64_t same = __ballot(F == f);
        if (same) {
            const int first = __ffsll((long long)same) - 1;
            uint32_t at = 0;
            if (lane == first) at = atomicAdd(&cnt->cursor[f], (uint32_t)__popcll(same));
            at = (uint32_t)__shfl((int)at, first);
            if (F == f) list[start + at + (uint32_t)__popcll(same & ((1ull << lane) - 1ull))] = r;
        }
        start += cnt->hist[f];
    }
}

// One workgroup per listed row of the class f_lo .. g.max_free (the host passes the class's upper end as the geometry's max_free:
// the dynamic table sd holds 2^max_free bytes): k_endgame_score's setup and solve, then the rule of include/dbaz.h in place.
// The grid is fixed (the host does not know the counts); workgroup b takes the class's rows b, b + gridDim.x, ... of the
// deepest-first list, so every workgroup gets the same mix of depths.  Wave 0, lane c = compact edge c, finds the members and
// S (row_members, table_row.h); the workgroup writes the row's pi (relabel_entry).  The statistics are kept per workgroup in LDS.
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_endgame_targets(EndgameGeo g, int f_lo, TargetCounters *__restrict__ cnt, const int32_t *__restrict__ list,
                                                             int n, const int16_t *__restrict__ x, int x_stride, int pi_mode, int z_mode,
                                                             float *pi, float *z, float *__restrict__ mass, uint8_t *__restrict__ relabelled,
                                                             int want_stats)
{
    extern __shared__ __attribute__((aligned(16))) int8_t sd[]; // [max(16, 2^g.max_free)]
    __shared__ EndgameLds L;
    __shared__ RowMembers s_members;
    __shared__ uint32_t s_stats[ENDGAME_MAX_FREE + 3];

    const int tid = threadIdx.x;
    uint32_t begin = 0, count = 0;
    for (int f = ENDGAME_MAX_FREE; f >= f_lo; f--) {
        const uint32_t h = cnt->hist[f];
        if (f > g.max_free) begin += h;
        else count += h;
    }
    if (tid < ENDGAME_MAX_FREE + 3) s_stats[tid] = 0;
    __syncthreads();
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const int r = list[begin + i];
        if ((unsigned)r >= (unsigned)n) continue; // never outside the caller's buffers (the same answer in every thread)
        const int16_t *xr = x + (size_t)r * x_stride;
        float *pr = pi ? pi + (size_t)r * g.A : nullptr;
        const int F = endgame_setup<RowEdges, THREADS>(g, RowEdges{xr}, L);
        if (F > g.max_free) { // not a row of this class: cannot happen with a list built from the same rows
            __syncthreads();
            continue;
        }
        endgame_solve<THREADS>(g, F, L, sd);

        const RowFacts f = solver_facts(g.rows * g.cols, L.closed, (int)xr[2 * g.HW]);
        const bool open = f.res == DBAZ_RESULT_NONE;
        if (open) {
            const int v = sgn(f.margin + (int)sd[0]);
            if (tid < 64) {
                const bool edge = tid < F;
                const int qq = edge ? solver_move_q(L.other[tid][0], L.other[tid][1], 0u, (int)sd[1u << tid]) : 0;
                const RowMembers M = row_members(edge, f.margin, qq, v, pr && edge ? pr[L.act[tid]] : 0.0f, F);
                if (tid == 0) s_members = M;
            }
            __syncthreads();
            const RowMembers M = s_members;
            if (pi_mode)
                for (int a = tid; a < g.A; a += THREADS) {
                    const int c = L.cidx[a];
                    pr[a] = relabel_entry(M, pi_mode, c >= 0 && ((M.set >> c) & 1u), pr[a]);
                }
            if (tid == 0) {
                if (z && z[r] != (float)v) s_stats[1]++;
                s_stats[2 + F]++;
                if (z_mode) z[r] = (float)v;
                if (mass) mass[r] = M.sum;
                if (relabelled) relabelled[r] = 1;
            }
        } else if (tid == 0) s_stats[0]++;
        __syncthreads(); // the next row of this workgroup reuses L and sd
    }
    if (want_stats && tid < ENDGAME_MAX_FREE + 3 && s_stats[tid]) atomicAdd(&cnt->stats[tid], (unsigned long long)s_stats[tid]);
}

// Leaves of the search solved from scratch (endgame.h, dbaz_attach_leaf_solver): k_endgame_targets' shape on the search's feature
// planes.  One launch per class of F with the class's upper end as the geometry's max_free (sd holds 2^max_free bytes) and a
// fixed grid; workgroup b takes entries b, b + gridDim.x, ... of the class's list, whose length is read here.  Per entry
// k_endgame_policy's steps and answer: setup and solve, wave 0 picks, the workgroup writes the one-hot row of `stride` floats and
// v.  An entry whose row lies outside the caller's buffers is skipped; one with F above the class (select lists none) gets
// k_endgame_policy's p = 0, v = 0.  The leaves solved per F are counted per workgroup in LDS and added once at the end.
template <int THREADS, typename T>
__global__ void __launch_bounds__(THREADS) k_endgame_leaves(EndgameGeo g, const int32_t *__restrict__ list, const int32_t *__restrict__ cnt, int cap,
                                                            const T *__restrict__ x, int max_n, uint64_t seed0, uint64_t seed1, float *__restrict__ P,
                                                            float *__restrict__ V, int stride, unsigned long long *__restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) int8_t sd[]; // [max(16, 2^g.max_free)]
    __shared__ EndgameLds L;
    __shared__ int s_pick;
    __shared__ uint32_t s_stats[ENDGAME_MAX_FREE + 1];

    const int tid = threadIdx.x;
    const int count = min(max(*cnt, 0), cap);
    if ((int)blockIdx.x >= count) return; // the same answer in every thread
    if (tid <= ENDGAME_MAX_FREE) s_stats[tid] = 0;
    __syncthreads();
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
        const int entry = list[i];
        const int r = entry & ((1 << LEAF_SOLVE_MODEL_SHIFT) - 1);
        if (entry < 0 || r >= max_n) continue; // never outside the caller's buffers (the same answer in every thread)
        const T *xr = x + (size_t)r * 3 * g.HW;
        float *pr = P + (size_t)r * stride;
        const int F = endgame_setup<PlaneEdges<T>, THREADS>(g, PlaneEdges<T>{xr}, L);
        if (F > g.max_free) {
            for (int a = tid; a < stride; a += THREADS) pr[a] = 0.0f;
            if (tid == 0) V[r] = 0.0f;
            __syncthreads();
            continue;
        }
        endgame_solve<THREADS>(g, F, L, sd);

        const RowFacts f = solver_facts(g.rows * g.cols, L.closed, (int)xr[2 * g.HW]);
        const bool open = f.res == DBAZ_RESULT_NONE; // a finished position is never listed: p = 0, v = get_result all the same
        if (tid < 64) {
            const bool cand = open && tid < F;
            const int qq = cand ? solver_move_q(L.other[tid][0], L.other[tid][1], 0u, (int)sd[1u << tid]) : 0;
            const int pick = endgame_pick(cand, qq, cand ? (int)L.act[tid] : 0, (entry >> LEAF_SOLVE_MODEL_SHIFT) & 1 ? seed1 : seed0);
            if (tid == 0) s_pick = pick;
        }
        __syncthreads();
        const int pick = s_pick;
        for (int a = tid; a < stride; a += THREADS) pr[a] = a == pick ? 1.0f : 0.0f;
        if (tid == 0) {
            V[r] = (float)(open ? sgn(f.margin + (int)sd[0]) : f.res);
            s_stats[F]++;
        }
        __syncthreads(); // the next entry of this workgroup reuses L, sd and s_pick
    }
    if (tid <= ENDGAME_MAX_FREE && s_stats[tid]) atomicAdd(&stats[tid], (unsigned long long)s_stats[tid]);
}

// ------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------
extern "C" const char *dbaz_endgame_last_error(const dbaz_endgame *g) { return g ? g->err.c_str() : g_endgame_error.c_str(); }

extern "C" void dbaz_endgame_destroy(dbaz_endgame *g)
{
    if (!g) return;
    (void)hipSetDevice(g->dev);
    for (void *b : g->bufs)
        if (b) (void)hipFree(b);
    for (void *b : {(void *)g->tg_list, (void *)g->tg_nfree, (void *)g->tg_cnt})
        if (b) (void)hipFree(b);
    delete g;
}

extern "C" int dbaz_endgame_create(int32_t rows, int32_t cols, int32_t device, int32_t max_free, dbaz_endgame **out)
{
    if (!out) return fail(g_endgame_error, DBAZ_EINVAL, "null argument");
    *out = nullptr;
    if (rows < 1 || cols < 1) return fail(g_endgame_error, DBAZ_EINVAL, "board %dx%d: rows and cols must be >= 1", rows, cols);
    const long long A = 2ll * (rows + 1ll) * (cols + 1ll);
    if (A > DBAZ_MAX_A) return fail(g_endgame_error, DBAZ_EINVAL, "board %dx%d has %lld action slots: at most %d are supported", rows, cols, A, DBAZ_MAX_A);
    if (max_free < 0 || max_free > ENDGAME_MAX_FREE)
        return fail(g_endgame_error, DBAZ_EINVAL, "max_free %d: a position's 2^F subgame table lives in LDS, 1 <= max_free <= %d (0 = %d)", max_free,
                    ENDGAME_MAX_FREE, ENDGAME_MAX_FREE);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(g_endgame_error, DBAZ_EDEVICE, "no HIP device %d (there is no CPU fallback)", device);

    const int H = rows + 1, W = cols + 1, HW = H * W;
    std::vector<uint8_t> action;
    std::vector<int> index(2 * HW, -1);
    for (int a = 0; a < 2 * HW; a++) {
        const int p = a / HW, l = (a % HW) / W, c = a % W;
        if (p == 0 ? c < cols : l < rows) { // sentinels: board[0,:,W-1] and board[1,H-1,:]
            index[a] = (int)action.size();
            action.push_back((uint8_t)a);
        }
    }
    const int E = (int)action.size();
    std::vector<int16_t> nbr((size_t)E * 6, -1);
    std::vector<int> used(E, 0);
    for (int l = 0; l < rows; l++)
        for (int c = 0; c < cols; c++) {
            const int ed[4] = {l * W + c, (l + 1) * W + c, HW + l * W + c, HW + l * W + c + 1};
            for (int i = 0; i < 4; i++) {
                const int e = index[ed[i]];
                int16_t *nb = &nbr[((size_t)e * 2 + used[e]++) * 3];
                for (int k = 0; k < 4; k++)
                    if (k != i) *nb++ = (int16_t)ed[k];
            }
        }
    std::vector<uint16_t> perm;
    std::vector<uint32_t> off((ENDGAME_MAX_FREE + 1) * ENDGAME_OFF_STRIDE, 0);
    for (int F = 0; F <= ENDGAME_MAX_FREE; F++) {
        std::vector<uint32_t> p, o;
        popcount_order(F, p, o);
        perm.insert(perm.end(), p.begin(), p.end()); // list F starts at 2^F - 1
        std::copy(o.begin(), o.end(), off.begin() + F * ENDGAME_OFF_STRIDE);
    }

    dbaz_endgame *g = new dbaz_endgame();
    g->dev = device;
    const void *src[4] = {action.data(), nbr.data(), perm.data(), off.data()};
    const size_t bytes[4] = {action.size(), nbr.size() * 2, perm.size() * 2, off.size() * 4};
    hipError_t e = hipSetDevice(device);
    for (int i = 0; i < 4 && e == hipSuccess; i++) {
        e = hipMalloc(&g->bufs[i], bytes[i]);
        if (e != hipSuccess) g->bufs[i] = nullptr;
        else e = hipMemcpy(g->bufs[i], src[i], bytes[i], hipMemcpyHostToDevice);
    }
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_endgame_score, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << ENDGAME_MAX_FREE);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_endgame_policy, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << ENDGAME_MAX_FREE);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_endgame_table, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << ENDGAME_MAX_FREE);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_endgame_targets<ENDGAME_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << ENDGAME_MAX_FREE);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_endgame_leaves<ENDGAME_THREADS, float>, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << ENDGAME_MAX_FREE);
    if (e != hipSuccess) {
        const std::string msg = hipGetErrorString(e);
        (void)hipGetLastError();
        dbaz_endgame_destroy(g);
        return fail(g_endgame_error, DBAZ_EDEVICE, "endgame setup failed: %s", msg.c_str());
    }
    g->g.rows = rows; g->g.cols = cols; g->g.HW = HW; g->g.A = 2 * HW; g->g.E = E;
    g->g.max_free = max_free == 0 ? ENDGAME_MAX_FREE : max_free;
    g->g.action = (const uint8_t *)g->bufs[0];
    g->g.nbr = (const int16_t *)g->bufs[1];
    g->g.perm = (const uint16_t *)g->bufs[2];
    g->g.off = (const uint32_t *)g->bufs[3];
    *out = g;
    return DBAZ_OK;
}

extern "C" int dbaz_endgame_score(dbaz_endgame *g, int32_t n, const int16_t *x_dev, const float *pi_dev, int8_t *value_dev, int8_t *diff_dev,
                                  int8_t *q_dev, float *mass_dev, int16_t *n_free_dev, void *stream)
{
    if (!g) return DBAZ_EINVAL;
    if (n < 0 || (n > 0 && (!x_dev || !value_dev || !diff_dev || !q_dev || !n_free_dev)) || (pi_dev && !mass_dev))
        return fail(g->err, DBAZ_EINVAL, "dbaz_endgame_score: bad argument (n = %d)", n);
    if (n == 0) return DBAZ_OK;
    CHECK_HIP(g->err, hipSetDevice(g->dev));
    k_endgame_score<<<(unsigned)n, ENDGAME_THREADS, (size_t)1 << g->g.max_free, (hipStream_t)stream>>>(g->g, x_dev, pi_dev, value_dev, diff_dev, q_dev,
                                                                                                      pi_dev ? mass_dev : nullptr, n_free_dev);
    CHECK_HIP(g->err, hipGetLastError());
    return DBAZ_OK;
}

extern "C" int dbaz_exact_policy(dbaz_endgame *g, int32_t n, const int16_t *x_dev, uint64_t pick_seed, float *p_dev, float *v_dev,
                                 uint8_t *solved_dev, void *stream)
{
    if (!g) return DBAZ_EINVAL;
    if (n < 0 || (n > 0 && (!x_dev || !p_dev || !v_dev || !solved_dev))) return fail(g->err, DBAZ_EINVAL, "dbaz_exact_policy: bad argument (n = %d)", n);
    if (n == 0) return DBAZ_OK;
    CHECK_HIP(g->err, hipSetDevice(g->dev));
    k_endgame_policy<<<(unsigned)n, ENDGAME_THREADS, (size_t)1 << g->g.max_free, (hipStream_t)stream>>>(g->g, x_dev, pick_seed, p_dev, v_dev,
                                                                                                       solved_dev);
    CHECK_HIP(g->err, hipGetLastError());
    return DBAZ_OK;
}

// ---- exact training targets: dense rows through the C ABI, the engine's resident dataset through endgame.h
// The classes of F one k_endgame_targets launch serves, deepest first: the table of a class takes 2^f_hi bytes of LDS, so the
// shallow classes fit more workgroups on a CU, and 256 threads cover every popcount layer of F <= 10 (C(10, 5) = 252 masks) in one
// pass.  grid: eight times what the chip holds at once (256 CUs x the workgroups per CU that LDS and wave slots admit) -- a CU
// that is done with a workgroup takes the next one, which evens out CUs of different pace; measured in DESIGN.md 5.
struct TargetClass {
    int f_lo, f_hi, threads, grid;
};
static const TargetClass kTargetClasses[] = {{16, 16, ENDGAME_THREADS, 4096}, {14, 15, ENDGAME_THREADS, 8192}, {11, 13, ENDGAME_THREADS, 8192},
                                             {0, 10, 256, 16384}};

int endgame_targets(dbaz_endgame *g, hipStream_t s, int32_t n, const int16_t *x, int x_stride, int pi_mode, int z_mode, float *pi, float *z,
                    int16_t *n_free, float *mass, uint8_t *relabelled, int64_t *stats_host)
{
    if (pi_mode < 0 || pi_mode > 2 || z_mode < 0 || z_mode > 1)
        return fail(g->err, DBAZ_EINVAL, "exact targets: pi_mode %d / z_mode %d (pi_mode 0 keep, 1 uniform, 2 restrict; z_mode 0 keep, 1 solved)", pi_mode, z_mode);
    if (n < 0 || (n > 0 && (!x || (pi_mode != 0 && !pi) || (z_mode != 0 && !z))))
        return fail(g->err, DBAZ_EINVAL, "exact targets: bad argument (n = %d; a mode other than keep needs its array)", n);
    if (stats_host) std::fill(stats_host, stats_host + 4 + ENDGAME_MAX_FREE + 1, (int64_t)0);
    if (n == 0) return DBAZ_OK;
    CHECK_HIP(g->err, hipSetDevice(g->dev));
    if (!g->tg_cnt) CHECK_HIP(g->err, hipMalloc((void **)&g->tg_cnt, sizeof(TargetCounters)));
    if ((size_t)n > g->tg_cap) { // hipFree waits for the kernels that still use the old scratch
        if (g->tg_list) (void)hipFree(g->tg_list);
        if (g->tg_nfree) (void)hipFree(g->tg_nfree);
        g->tg_list = nullptr;
        g->tg_nfree = nullptr;
        g->tg_cap = 0;
        const size_t cap = (size_t)n + (size_t)n / 2;
        CHECK_HIP(g->err, hipMalloc((void **)&g->tg_list, cap * sizeof(int32_t)));
        CHECK_HIP(g->err, hipMalloc((void **)&g->tg_nfree, cap * sizeof(int16_t)));
        g->tg_cap = cap;
    }
    int16_t *nf = n_free ? n_free : g->tg_nfree;
    CHECK_HIP(g->err, hipMemsetAsync(g->tg_cnt, 0, sizeof(TargetCounters), s));
    const int cand_blocks = std::min((n + ENDGAME_CAND_WAVES - 1) / ENDGAME_CAND_WAVES, 16384);
    k_endgame_candidates<<<cand_blocks, 64 * ENDGAME_CAND_WAVES, 0, s>>>(g->g, x, x_stride, n, nf, mass, relabelled, g->tg_cnt);
    k_endgame_list<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(g->g.max_free, n, nf, g->tg_cnt, g->tg_list);
    for (const TargetClass &c : kTargetClasses) {
        if (c.f_lo > g->g.max_free) continue;
        EndgameGeo gc = g->g;
        gc.max_free = std::min(c.f_hi, g->g.max_free);
        const size_t lds = std::max<size_t>(16, (size_t)1 << gc.max_free);
        const unsigned grid = (unsigned)std::min(n, c.grid);
        if (c.threads == 256)
            k_endgame_targets<256><<<grid, 256, lds, s>>>(gc, c.f_lo, g->tg_cnt, g->tg_list, n, x, x_stride, pi_mode, z_mode, pi, z, mass, relabelled,
                                                          stats_host != nullptr);
        else
            k_endgame_targets<ENDGAME_THREADS><<<grid, ENDGAME_THREADS, lds, s>>>(gc, c.f_lo, g->tg_cnt, g->tg_list, n, x, x_stride, pi_mode, z_mode, pi,
                                                                                  z, mass, relabelled, stats_host != nullptr);
    }
    CHECK_HIP(g->err, hipGetLastError());
    if (stats_host) {
        unsigned long long st[ENDGAME_MAX_FREE + 3];
        CHECK_HIP(g->err, hipMemcpyAsync(st, g->tg_cnt->stats, sizeof st, hipMemcpyDeviceToHost, s));
        CHECK_HIP(g->err, hipStreamSynchronize(s));
        stats_host[0] = n;
        stats_host[2] = (int64_t)st[0];
        stats_host[3] = (int64_t)st[1];
        for (int f = 0; f <= ENDGAME_MAX_FREE; f++) {
            stats_host[4 + f] = (int64_t)st[2 + f];
            stats_host[1] += (int64_t)st[2 + f];
        }
    }
    return DBAZ_OK;
}

extern "C" int dbaz_exact_targets(dbaz_endgame *g, int32_t n, const int16_t *x_dev, int32_t pi_mode, int32_t z_mode, float *pi_dev, float *z_dev,
                                  int16_t *n_free_dev, float *mass_dev, uint8_t *relabelled_dev, void *stream)
{
    if (!g) return DBAZ_EINVAL;
    return endgame_targets(g, (hipStream_t)stream, n, x_dev, 3 * g->g.HW, pi_mode, z_mode, pi_dev, z_dev, n_free_dev, mass_dev, relabelled_dev, nullptr);
}

// ---- the engine's side (endgame.h): one game's table behind the evaluator boundary
bool endgame_serves(const dbaz_endgame *g, int rows, int cols, int device, int *max_free)
{
    *max_free = g->g.max_free;
    return g->g.rows == rows && g->g.cols == cols && g->dev == device;
}

size_t endgame_table_stride(const dbaz_endgame *g) { return std::max<size_t>(16, (size_t)1 << g->g.max_free); }

void endgame_tables(const dbaz_endgame *g, hipStream_t stream, EndgameReq *req, EndgameSlotHdr *hdr, int8_t *tables, int n_slots,
                    unsigned long long *stats)
{
    const size_t stride = endgame_table_stride(g);
    k_endgame_table<<<(unsigned)std::min(n_slots, ENDGAME_TABLE_GRID), ENDGAME_THREADS, stride, stream>>>(g->g, req, hdr, tables, stride, n_slots,
                                                                                                    stats);
}

// The leaf solver's launches of one step: the classes of kTargetClasses that leaf_free reaches, deepest first, each with the grid
// the chip holds at once (256 CUs x the workgroups per CU that the class's LDS and 32 wave slots admit) -- a step lists hundreds
// of leaves, not a dataset, and a class without entries costs one word read per workgroup.
static const int kLeafGrids[LEAF_SOLVE_CLASSES] = {512, 1024, 1024, 2048};

void endgame_solve_leaves(const dbaz_endgame *g, hipStream_t stream, int leaf_free, const int32_t *list_dev, const int32_t *cnt_dev, int cap,
                          const float *x, int max_n, uint64_t seed0, uint64_t seed1, float *P, float *V, int AS, unsigned long long *stats)
{
    static_assert(sizeof kTargetClasses / sizeof kTargetClasses[0] == LEAF_SOLVE_CLASSES, "leaf_solve_class (endgame.h) names these classes");
    for (int c = 0; c < LEAF_SOLVE_CLASSES; c++) {
        const TargetClass &tc = kTargetClasses[c];
        if (tc.f_lo > leaf_free) continue;
        EndgameGeo gc = g->g;
        gc.max_free = std::min(tc.f_hi, std::min(leaf_free, g->g.max_free));
        const size_t lds = std::max<size_t>(16, (size_t)1 << gc.max_free);
        const unsigned grid = (unsigned)std::max(1, std::min(cap, kLeafGrids[c]));
        const int32_t *list = list_dev + (size_t)c * cap;
        if (tc.threads == 256)
            k_endgame_leaves<256, float><<<grid, 256, lds, stream>>>(gc, list, cnt_dev + c, cap, x, max_n, seed0, seed1, P, V, AS, stats);
        else
            k_endgame_leaves<ENDGAME_THREADS, float><<<grid, ENDGAME_THREADS, lds, stream>>>(gc, list, cnt_dev + c, cap, x, max_n, seed0, seed1, P, V, AS,
                                                                                            stats);
    }
}

template <typename T>
void endgame_forward(int rows, int cols, int max_free, size_t tab_stride, int n_tables, hipStream_t stream, const EndgameSlotHdr *hdr,
                     const int8_t *tables, const T *x, const int32_t *list_dev, const int32_t *n_dev, int max_n, int per_slot, uint64_t seed0, uint64_t seed1, float *P,
                     float *V, int AS, unsigned long long *stats)
{
    const int blocks = std::min((max_n + ENDGAME_EVAL_WAVES - 1) / ENDGAME_EVAL_WAVES, 4096);
    k_endgame_eval<T><<<blocks, 64 * ENDGAME_EVAL_WAVES, 0, stream>>>(tables_board(rows, cols), max_free, hdr, tables, tab_stride, n_tables, x, list_dev,
                                                                    n_dev, max_n, per_slot, seed0, seed1, P, V, AS, stats);
}
template void endgame_forward<float>(int, int, int, size_t, int, hipStream_t, const EndgameSlotHdr *, const int8_t *, const float *, const int32_t *,
                                     const int32_t *, int, int, uint64_t, uint64_t, float *, float *, int, unsigned long long *); // the engine's

// The table path on its own: the yardstick of k_endgame_table / k_endgame_eval against dbaz_exact_policy, the int16 form of the
// evaluator, and the place where the two kernels are timed.
extern "C" int dbaz_exact_policy_from(dbaz_endgame *g, int32_t n_roots, const int16_t *roots_dev, int32_t per_root, const int16_t *x_dev,
                                      uint64_t pick_seed, float *p_dev, float *v_dev, float *ms_out, void *stream)
{
    if (!g) return DBAZ_EINVAL;
    if (n_roots < 0 || per_root < 1 || (long long)n_roots * per_root > 0x7fffffffll || (n_roots > 0 && (!roots_dev || !x_dev || !p_dev || !v_dev)))
        return fail(g->err, DBAZ_EINVAL, "dbaz_exact_policy_from: bad argument (n_roots = %d, per_root = %d)", n_roots, per_root);
    if (ms_out) ms_out[0] = ms_out[1] = 0.0f;
    if (n_roots == 0) return DBAZ_OK;
    CHECK_HIP(g->err, hipSetDevice(g->dev));
    hipStream_t s = (hipStream_t)stream;
    const size_t stride = endgame_table_stride(g), n = (size_t)n_roots;
    void *buf[4] = {nullptr, nullptr, nullptr, nullptr}; // tables, headers, requests, stats
    const size_t bytes[4] = {n * stride, n * sizeof(EndgameSlotHdr), n * sizeof(EndgameReq), 16};
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; i++) {
        e = hipMalloc(&buf[i], bytes[i]);
        if (e != hipSuccess) buf[i] = nullptr;
        else if (i) e = hipMemsetAsync(buf[i], 0, bytes[i], s);
    }
    for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    if (e == hipSuccess) {
        k_endgame_requests<<<(unsigned)((n_roots + 255) / 256), 256, 0, s>>>(g->g, roots_dev, n_roots, (EndgameReq *)buf[2]);
        e = hipEventRecord(ev[0], s);
    }
    if (e == hipSuccess) {
        endgame_tables(g, s, (EndgameReq *)buf[2], (EndgameSlotHdr *)buf[1], (int8_t *)buf[0], n_roots, (unsigned long long *)buf[3]);
        e = hipEventRecord(ev[1], s);
    }
    if (e == hipSuccess) {
        endgame_forward<int16_t>(g->g.rows, g->g.cols, g->g.max_free, stride, n_roots, s, (const EndgameSlotHdr *)buf[1], (const int8_t *)buf[0], x_dev, nullptr,
                                 nullptr, n_roots * per_root, per_root, pick_seed, pick_seed, p_dev, v_dev, g->g.A, nullptr);
        e = hipEventRecord(ev[2], s);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventSynchronize(ev[2]); // the scratch buffers go away below
    if (e == hipSuccess && ms_out) {
        e = hipEventElapsedTime(&ms_out[0], ev[0], ev[1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_out[1], ev[1], ev[2]);
    }
    for (hipEvent_t v : ev)
        if (v) (void)hipEventDestroy(v);
    for (void *b : buf)
        if (b) (void)hipFree(b);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(g->err, DBAZ_EDEVICE, "dbaz_exact_policy_from (%d roots x %zu bytes): %s", n_roots, stride, hipGetErrorString(e));
    }
    return DBAZ_OK;
}
