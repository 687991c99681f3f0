// solver.hip -- exact solver for small Dots & Boxes boards (E <= 31 real edges): retrograde analysis on the GPU, a kernel that
// scores feature rows against the solved table and one that serves the table as a (p, v) evaluator (k_solver_eval; the engine
// launches it through solver.h).  No dbaz_engine, no search or network code.
//
// Table: int8 D[2^E] in HBM.  D[mask] = best achievable (mover's boxes) - (opponent's boxes) over the boxes still open, optimal
// play by both sides, from the edge set `mask` (compact edge order, solver.h).  It depends on the mask only.
//   D[full] = 0;   for a free edge e completing c boxes:  Q = c + D[mask|e] if c > 0 (the mover continues), else -D[mask|e];
//   D[mask] = max Q.   A state with k edges reads only states with k + 1 edges.
//
// k_solver_subcube: a workgroup owns one pattern of the high E - L bits and solves the 2^L subcube of the low L bits in LDS.
//   A. successors that set a HIGH bit were written by earlier launches: for every free high edge the workgroup streams the
//      2^L-byte subcube of that successor from HBM, 16 consecutive entries per lane, and keeps the running maximum in LDS;
//   B. successors that set a LOW bit are in LDS: popcount layers L .. 0 of the low bits, one barrier each; the low masks of a
//      layer come from a popcount-sorted list, so every lane of a wave has a state to solve;
//   C. the finished subcube goes to HBM in 16-byte stores.
// One launch per popcount layer of the high bits (E - L + 1 launches).
// k_solver_layer: the plain form, one thread per mask and one launch per popcount layer of all E bits (A/B partner).
//
// Both kernels read their geometry from an array in HBM, one BatchGeo per blockIdx.y: the whole board is an array of one.
//
// The second half of the file runs the same two kernels on the subgames of positions of any board, F <= 31 free
// edges each: a pool of tables (dbaz_tables_*), many roots solved side by side with grid.y = the roots of equal F, and rows of
// many games answered in one launch, each from its game's table (k_tables_score, k_tables_targets).  dbaz_deep_* is a pool of one
// table on the same path, plus the table as an evaluator (k_deep_policy).  dbaz_replay_exact_targets takes packed replay rows
// instead of feature rows: games, roots and geometries are found on the device (k_replay_*), the rows relabelled where they lie.
// At the end, the same bodies inside the search
// (dbaz_attach_tables): one table per engine slot, solved from requests that exist only on the device (k_slot_requests,
// k_slot_solve; slot_tables_plan.h).
#include <hipcub/hipcub.hpp>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "deep_batch.h"
#include "endgame.h"
#include "position_geo.h"
#include "replay_chunks.h"
#include "replay_row.h"
#include "slot_tables_plan.h"
#include "solver.h"
#include "table_pool.h"
#include "table_row.h"

// One root's solve geometry as the two solving kernels read it from HBM: what the bodies need of a SolverGeo, and the table slot
// the root owns.  A whole board (dbaz_solver) is one entry with F = E and slot 0.
typedef uint32_t SolverOther[SOLVER_MAX_E][2];
struct BatchGeo {
    int32_t F, slot;
    SolverOther other;
};
static_assert(sizeof(BatchGeo) == 256, "one root's solve geometry");

// the popcount-ordered work lists of one (F, L) on the device: they depend on nothing else and stay on the handle that asked
struct WorkLists {
    int F = 0, L = 0;
    uint32_t *hi_dev = nullptr, *off_dev = nullptr;
    uint16_t *low_dev = nullptr;
    std::vector<uint32_t> hoff;
};

struct dbaz_solver {
    SolverGeo g;
    int dev = 0;
    int8_t *D = nullptr;     // [2^E]
    BatchGeo *geo_dev = nullptr; // [1]: g as the solving kernels read it
    hipStream_t stream = nullptr;
    bool solved = false;
    int low_bits = 0;        // of the last solve (-1: plain kernel)
    double solve_ms = -1.0;
    int d0 = -128;
    std::vector<WorkLists> lists;
    std::string err;
};

// the message of a failed create, per family and thread (fail, solver.h)
static thread_local std::string g_solver_error, g_deep_error, g_tables_error;

// ------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------
// The bodies of the two solving kernels, shared with k_slot_solve: other = the geometry's box masks, E its edges, D its table.
// m: the thread's mask (one thread per mask of the table)
static __device__ __forceinline__ void solver_layer_body(const SolverOther &other, int E, int8_t *D, int k, uint32_t m)
{
    if (m >= (1u << E) || __popc(m) != k) return;
    int best = k == E ? 0 : -128;
    for (int e = 0; e < E; e++) {
        if ((m >> e) & 1u) continue;
        best = max(best, solver_move_q(other[e][0], other[e][1], m, (int)D[m | (1u << e)]));
    }
    D[m] = (int8_t)best;
}

static __device__ __forceinline__ void solver_subcube_body(const SolverOther &other, int E, int8_t *D, int L, uint32_t hi,
                                                           const uint16_t *__restrict__ low_perm, const uint32_t *__restrict__ low_off)
{
    extern __shared__ __attribute__((aligned(16))) int8_t sd[]; // [2^L]
    const uint32_t tid = threadIdx.x;
    const uint32_t base = hi << L, nlow = 1u << L;
    const int nh = E - L;

    // A: running maximum over the moves that draw a high edge
    for (uint32_t chunk = tid * 16u; chunk < nlow; chunk += SOLVER_THREADS * 16u) {
        int best[16];
#pragma unroll
        for (int j = 0; j < 16; j++) best[j] = -128;
        for (int h = 0; h < nh; h++) {
            if ((hi >> h) & 1u) continue;
            const int e = L + h;
            const uint32_t o0 = other[e][0], o1 = other[e][1];
            const uint4 v = *reinterpret_cast<const uint4 *>(D + ((size_t)(base | (1u << e)) + chunk));
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int d = (int)(int8_t)(w[j >> 2] >> ((j & 3) * 8));
                best[j] = max(best[j], solver_move_q(o0, o1, base | (chunk + j), d));
            }
        }
        uint32_t p[4];
#pragma unroll
        for (int q = 0; q < 4; q++)
            p[q] = (uint32_t)(uint8_t)best[4 * q] | (uint32_t)(uint8_t)best[4 * q + 1] << 8 | (uint32_t)(uint8_t)best[4 * q + 2] << 16 |
                   (uint32_t)(uint8_t)best[4 * q + 3] << 24;
        *reinterpret_cast<uint4 *>(sd + chunk) = make_uint4(p[0], p[1], p[2], p[3]);
    }
    __syncthreads();

    // B: the moves that draw a low edge, by popcount layers of the low bits
    const uint32_t full = (1u << E) - 1u;
    for (int k = L; k >= 0; k--) {
        for (uint32_t i = low_off[k] + tid; i < low_off[k + 1]; i += SOLVER_THREADS) {
            const uint32_t low = low_perm[i], m = base | low;
            int best = (int)sd[low];
            for (int b = 0; b < L; b++) {
                const uint32_t bit = 1u << b;
                if (low & bit) continue;
                best = max(best, solver_move_q(other[b][0], other[b][1], m, (int)sd[low | bit]));
            }
            sd[low] = (int8_t)(m == full ? 0 : best);
        }
        __syncthreads();
    }

    // C
    for (uint32_t chunk = tid * 16u; chunk < nlow; chunk += SOLVER_THREADS * 16u)
        *reinterpret_cast<uint4 *>(D + ((size_t)base + chunk)) = *reinterpret_cast<const uint4 *>(sd + chunk);
}

// The two solving kernels: blockIdx.y = the root within a group of roots with the same F (deep_batch.h; a whole board or a single
// position is a group of one), geo = the group's geometries; the root's table is T + slot * 2^stride_bits.  Every workgroup reads
// one geometry, so the reads are wave-uniform.
__global__ void __launch_bounds__(256) k_solver_layer(const BatchGeo *__restrict__ geo, int8_t *T, int stride_bits, int k)
{
    const BatchGeo &g = geo[blockIdx.y];
    solver_layer_body(g.other, g.F, T + ((size_t)g.slot << stride_bits), k, blockIdx.x * 256u + threadIdx.x);
}

__global__ void __launch_bounds__(SOLVER_THREADS) k_solver_subcube(const BatchGeo *__restrict__ geo, int8_t *T, int stride_bits, int L,
                                                                   const uint32_t *__restrict__ hi_list, const uint16_t *__restrict__ low_perm,
                                                                   const uint32_t *__restrict__ low_off)
{
    const BatchGeo &g = geo[blockIdx.y];
    solver_subcube_body(g.other, g.F, T + ((size_t)g.slot << stride_bits), L, hi_list[blockIdx.x], low_perm, low_off);
}

// solver_facts (solver.h) of a position given as a mask: the closed boxes come from the box masks.  Shared by k_solver_score and
// k_solver_eval.
__device__ __forceinline__ RowFacts solver_row_facts(const SolverGeo &g, uint32_t m, int own_b2c)
{
    int closed = 0;
    for (int b = 0; b < g.n_boxes; b++) closed += (int)((m & g.box[b]) == g.box[b]);
    return solver_facts(g.rows * g.cols, closed, own_b2c);
}

// One thread per feature row x int16 [3*HW] (planes 0, 1: edges; plane 2: the mover's doubled boxes_to_close).
__global__ void __launch_bounds__(256) k_solver_score(SolverGeo g, const int8_t *__restrict__ D, const int16_t *__restrict__ x,
                                                      const float *__restrict__ pi, int n, int8_t *__restrict__ value,
                                                      int8_t *__restrict__ diff, int8_t *__restrict__ q, float *__restrict__ mass)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int16_t *xr = x + (size_t)r * 3 * g.HW;
    uint32_t m = 0;
    for (int i = 0; i < g.E; i++)
        if (xr[g.action[i]] != 0) m |= 1u << i;
    const RowFacts f = solver_row_facts(g, m, (int)xr[2 * g.HW]);
    const int margin = f.margin;
    const int d = (int)D[m];
    int8_t *qr = q + (size_t)r * g.A;
    for (int a = 0; a < g.A; a++) qr[a] = -128;
    diff[r] = (int8_t)d;
    if (f.res != DBAZ_RESULT_NONE) {
        value[r] = (int8_t)f.res;
        if (mass) mass[r] = 0.0f;
        return;
    }
    const int v = sgn(margin + d);
    float sum = 0.0f;
    for (int i = 0; i < g.E; i++) { // ascending action order
        if ((m >> i) & 1u) continue;
        const int qq = solver_move_q(g.other[i][0], g.other[i][1], m, (int)D[m | (1u << i)]);
        const int a = g.action[i];
        qr[a] = (int8_t)qq;
        if (pi && sgn(margin + qq) == v) sum += pi[(size_t)r * g.A + a];
    }
    value[r] = (int8_t)v;
    if (mass) mass[r] = sum;
}

// The table as a (p, v) evaluator with nn_forward's contract (nn.h): rows x[list[j]], j < min(*n_dev, max_n) (list == nullptr:
// identity, n_dev == nullptr: max_n rows), T = int16 (dataset rows) or float (TreeBufs.feat planes); a one-hot policy row goes to
// P[list[j] * stride ..+stride) and v = sign(margin + D[mask]) to V[list[j]].  One wavefront per row, lane i = compact edge i:
// the mask is a ballot over planes 0 / 1, every free lane reads D of its successor, the wave maximum of Q names the optimal set,
// and the pick is its k-th member in ascending edge order (k = 0, or solver_pick_mix % n_opt with a seed).  One-hot, not uniform
// over the optimal set: DESIGN 4.6.  A finished position gets p = 0 and v = get_result.
#define SOLVER_EVAL_WAVES 4
template <typename T>
__global__ void __launch_bounds__(64 * SOLVER_EVAL_WAVES) k_solver_eval(SolverGeo g, const int8_t *__restrict__ D, const T *__restrict__ x,
                                                                        const int32_t *__restrict__ list, const int32_t *__restrict__ n_dev,
                                                                        int max_n, uint64_t pick_seed, float *__restrict__ P,
                                                                        float *__restrict__ V, int stride)
{
    const int lane = threadIdx.x & 63;
    const int n = n_dev ? min(*n_dev, max_n) : max_n;
    for (int j = blockIdx.x * SOLVER_EVAL_WAVES + (threadIdx.x >> 6); j < n; j += gridDim.x * SOLVER_EVAL_WAVES) {
        const int r = list ? list[j] : j;
        if ((unsigned)r >= (unsigned)max_n) continue; // never outside the caller's buffers
        const T *xr = x + (size_t)r * 3 * g.HW;
        const bool edge = lane < g.E;
        const bool drawn = edge && xr[g.action[edge ? lane : 0]] != (T)0;
        const uint32_t m = (uint32_t)__ballot(drawn);
        const RowFacts f = solver_row_facts(g, m, (int)xr[2 * g.HW]);
        const bool open = f.res == DBAZ_RESULT_NONE;
        const bool cand = open && edge && !drawn;
        int q = -1024;
        if (cand) q = solver_move_q(g.other[lane][0], g.other[lane][1], m, (int)D[m | (1u << lane)]);
        int best = q;
        for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
        uint32_t opt = (uint32_t)__ballot(cand && q == best);
        int pick_a = -1;
        if (opt) {
            int k = pick_seed ? (int)(solver_pick_mix(m, pick_seed) % (uint64_t)__popc(opt)) : 0;
            for (; k > 0; k--) opt &= opt - 1u;
            pick_a = (int)g.action[__ffs((int)opt) - 1];
        }
        float *pr = P + (size_t)r * stride;
        for (int a = lane; a < stride; a += 64) pr[a] = a == pick_a ? 1.0f : 0.0f;
        if (lane == 0) V[r] = open ? (float)sgn(f.margin + (int)D[m]) : (float)f.res;
    }
}

// ------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------
static void solver_geometry(int rows, int cols, SolverGeo &g)
{
    const int H = rows + 1, W = cols + 1, HW = H * W;
    g = SolverGeo();
    g.rows = rows; g.cols = cols; g.HW = HW; g.A = 2 * HW;
    int index[DBAZ_MAX_A];
    int E = 0;
    for (int a = 0; a < g.A; a++) {
        const int p = a / HW, l = (a % HW) / W, c = a % W;
        const bool real = p == 0 ? c < cols : l < rows; // sentinels: board[0,:,W-1] and board[1,H-1,:]
        index[a] = real ? E : -1;
        if (real) g.action[E++] = (uint8_t)a;
    }
    g.E = E;
    for (int e = 0; e < SOLVER_MAX_E; e++) g.other[e][0] = g.other[e][1] = SOLVER_NO_BOX;
    int used[SOLVER_MAX_E] = {0};
    for (int l = 0; l < rows; l++)
        for (int c = 0; c < cols; c++) {
            const int ed[4] = {index[l * W + c], index[(l + 1) * W + c], index[HW + l * W + c], index[HW + l * W + c + 1]};
            uint32_t bm = 0;
            for (int j = 0; j < 4; j++) bm |= 1u << ed[j];
            g.box[g.n_boxes++] = bm;
            for (int j = 0; j < 4; j++) g.other[ed[j]][used[ed[j]]++] = bm & ~(1u << ed[j]);
        }
}

extern "C" const char *dbaz_solver_last_error(const dbaz_solver *s) { return s ? s->err.c_str() : g_solver_error.c_str(); }

// The work lists of (F, L) in a handle's cache, built and copied the first time the pair is asked for: its index, or -1 with *e set.
static int work_lists(std::vector<WorkLists> &cache, int F, int L, hipError_t *e)
{
    for (size_t i = 0; i < cache.size(); i++)
        if (cache[i].F == F && cache[i].L == L) return (int)i;
    WorkLists l;
    l.F = F;
    l.L = L;
    std::vector<uint32_t> lperm, loff, hperm;
    popcount_order(L, lperm, loff);
    popcount_order(F - L, hperm, l.hoff);
    const std::vector<uint16_t> l16(lperm.begin(), lperm.end());
    *e = hipMalloc((void **)&l.hi_dev, hperm.size() * 4);
    if (*e == hipSuccess) *e = hipMalloc((void **)&l.low_dev, l16.size() * 2);
    if (*e == hipSuccess) *e = hipMalloc((void **)&l.off_dev, loff.size() * 4);
    if (*e == hipSuccess) *e = hipMemcpy(l.hi_dev, hperm.data(), hperm.size() * 4, hipMemcpyHostToDevice);
    if (*e == hipSuccess) *e = hipMemcpy(l.low_dev, l16.data(), l16.size() * 2, hipMemcpyHostToDevice);
    if (*e == hipSuccess) *e = hipMemcpy(l.off_dev, loff.data(), loff.size() * 4, hipMemcpyHostToDevice);
    if (*e != hipSuccess) {
        for (void *b : {(void *)l.hi_dev, (void *)l.low_dev, (void *)l.off_dev})
            if (b) (void)hipFree(b);
        (void)hipGetLastError();
        return -1;
    }
    cache.push_back(std::move(l));
    return (int)cache.size() - 1;
}

static void free_work_lists(std::vector<WorkLists> &cache)
{
    for (WorkLists &l : cache)
        for (void *b : {(void *)l.hi_dev, (void *)l.low_dev, (void *)l.off_dev})
            if (b) (void)hipFree(b);
    cache.clear();
}

extern "C" void dbaz_solver_destroy(dbaz_solver *s)
{
    if (!s) return;
    (void)hipSetDevice(s->dev);
    if (s->D) (void)hipFree(s->D);
    if (s->geo_dev) (void)hipFree(s->geo_dev);
    free_work_lists(s->lists);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

extern "C" int dbaz_solver_create(int32_t rows, int32_t cols, int32_t device, dbaz_solver **out)
{
    if (!out) return fail(g_solver_error, DBAZ_EINVAL, "null argument");
    *out = nullptr;
    if (rows < 1 || cols < 1) return fail(g_solver_error, DBAZ_EINVAL, "board %dx%d: rows and cols must be >= 1", rows, cols);
    const long long E = 2ll * rows * cols + rows + cols;
    if (E > SOLVER_MAX_E)
        return fail(g_solver_error, DBAZ_EINVAL, "board %dx%d has %lld edges: the solver's table holds 2^E bytes, E <= %d", rows, cols, E, SOLVER_MAX_E);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(g_solver_error, DBAZ_EDEVICE, "no HIP device %d (there is no CPU fallback)", device);
    dbaz_solver *s = new dbaz_solver();
    s->dev = device;
    solver_geometry(rows, cols, s->g);
    BatchGeo bg; // the board as a group of one root: it never changes, so it goes up once
    bg.F = s->g.E;
    bg.slot = 0;
    memcpy(bg.other, s->g.other, sizeof bg.other);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreate(&s->stream);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_solver_subcube, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << SOLVER_MAX_LOW);
    if (e == hipSuccess) e = hipMalloc((void **)&s->geo_dev, sizeof bg);
    if (e == hipSuccess) e = hipMemcpy(s->geo_dev, &bg, sizeof bg, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        const std::string msg = hipGetErrorString(e);
        (void)hipGetLastError();
        dbaz_solver_destroy(s);
        return fail(g_solver_error, DBAZ_EDEVICE, "solver setup failed: %s", msg.c_str());
    }
    *out = s;
    return DBAZ_OK;
}

extern "C" int dbaz_solver_solve(dbaz_solver *s, int32_t low_bits)
{
    if (!s) return DBAZ_EINVAL;
    const int E = s->g.E;
    const bool plain = low_bits == -1;
    const int L = low_bits == 0 ? default_low_bits(E) : low_bits;
    if (!plain && (L < SOLVER_MIN_LOW || L > SOLVER_MAX_LOW || L > E || E - L > SOLVER_MAX_HIGH))
        return fail(s->err, DBAZ_EINVAL, "low_bits %d: E = %d needs max(%d, E - %d) <= low_bits <= min(E, %d) (0 = default, -1 = plain kernel)",
                    low_bits, E, SOLVER_MIN_LOW, SOLVER_MAX_HIGH, SOLVER_MAX_LOW);
    CHECK_HIP(s->err, hipSetDevice(s->dev));
    const size_t bytes = (size_t)1 << E;
    if (!s->D) {
        const hipError_t e = hipMalloc((void **)&s->D, bytes);
        if (e != hipSuccess) {
            s->D = nullptr;
            (void)hipGetLastError();
            return fail(s->err, DBAZ_EDEVICE, "table of %zu bytes: %s", bytes, hipGetErrorString(e));
        }
    }
    s->solved = false;
    hipError_t e = hipSuccess;
    const int li = plain ? -1 : work_lists(s->lists, E, L, &e);
    if (e != hipSuccess) return fail(s->err, DBAZ_EDEVICE, "solver work lists: %s", hipGetErrorString(e));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, s->stream);
    if (e == hipSuccess) {
        if (plain) {
            const unsigned grid = (unsigned)((bytes + 255) / 256);
            for (int k = E; k >= 0; k--) k_solver_layer<<<grid, 256, 0, s->stream>>>(s->geo_dev, s->D, 0, k);
        } else {
            const WorkLists &w = s->lists[(size_t)li];
            for (int k = E - L; k >= 0; k--)
                k_solver_subcube<<<w.hoff[k + 1] - w.hoff[k], SOLVER_THREADS, (size_t)1 << L, s->stream>>>(s->geo_dev, s->D, 0, L, w.hi_dev + w.hoff[k],
                                                                                                          w.low_dev, w.off_dev);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev1, s->stream);
    if (e == hipSuccess) e = hipEventSynchronize(ev1);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    int8_t d0 = 0;
    if (e == hipSuccess) e = hipMemcpy(&d0, s->D, 1, hipMemcpyDeviceToHost);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (e != hipSuccess) return fail(s->err, DBAZ_EDEVICE, "solve failed: %s", hipGetErrorString(e));
    s->solved = true;
    s->low_bits = plain ? -1 : L;
    s->solve_ms = ms;
    s->d0 = d0;
    return DBAZ_OK;
}

extern "C" int dbaz_solver_info(const dbaz_solver *s, int32_t *n_edges, int64_t *table_bytes, double *solve_ms, int32_t *d0)
{
    if (!s) return DBAZ_EINVAL;
    if (n_edges) *n_edges = s->g.E;
    if (table_bytes) *table_bytes = (int64_t)1 << s->g.E;
    if (solve_ms) *solve_ms = s->solve_ms;
    if (d0) *d0 = s->d0;
    return DBAZ_OK;
}

extern "C" int dbaz_solver_table(dbaz_solver *s, int8_t *host_dst, int64_t first, int64_t count)
{
    if (!s) return DBAZ_EINVAL;
    if (!s->solved) return fail(s->err, DBAZ_ESTATE, "dbaz_solver_table before dbaz_solver_solve");
    const int64_t n = (int64_t)1 << s->g.E;
    if (!host_dst || first < 0 || count < 0 || first > n || count > n - first)
        return fail(s->err, DBAZ_EINVAL, "table slice [%lld, +%lld) outside [0, %lld)", (long long)first, (long long)count, (long long)n);
    if (count == 0) return DBAZ_OK;
    CHECK_HIP(s->err, hipSetDevice(s->dev));
    CHECK_HIP(s->err, hipMemcpy(host_dst, s->D + first, (size_t)count, hipMemcpyDeviceToHost));
    return DBAZ_OK;
}

extern "C" int dbaz_solver_score(dbaz_solver *s, int32_t n, const int16_t *x_dev, const float *pi_dev, int8_t *value_dev, int8_t *diff_dev,
                                 int8_t *q_dev, float *policy_mass_dev, void *stream)
{
    if (!s) return DBAZ_EINVAL;
    if (!s->solved) return fail(s->err, DBAZ_ESTATE, "dbaz_solver_score before dbaz_solver_solve");
    if (n < 0 || (n > 0 && (!x_dev || !value_dev || !diff_dev || !q_dev)) || (pi_dev && !policy_mass_dev))
        return fail(s->err, DBAZ_EINVAL, "dbaz_solver_score: bad argument (n = %d)", n);
    if (n == 0) return DBAZ_OK;
    CHECK_HIP(s->err, hipSetDevice(s->dev));
    k_solver_score<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(s->g, s->D, x_dev, pi_dev, n, value_dev, diff_dev, q_dev,
                                                                     pi_dev ? policy_mass_dev : nullptr);
    CHECK_HIP(s->err, hipGetLastError());
    return DBAZ_OK;
}

template <typename T>
static void launch_eval(const dbaz_solver *s, hipStream_t stream, const T *x, const int32_t *list_dev, const int32_t *n_dev, int max_n,
                        uint64_t pick_seed, float *P, float *V, int stride)
{
    const int blocks = std::min((max_n + SOLVER_EVAL_WAVES - 1) / SOLVER_EVAL_WAVES, 4096);
    k_solver_eval<T><<<blocks, 64 * SOLVER_EVAL_WAVES, 0, stream>>>(s->g, s->D, x, list_dev, n_dev, max_n, pick_seed, P, V, stride);
}

extern "C" int dbaz_perfect_policy(dbaz_solver *s, int32_t n, const int16_t *x_dev, uint64_t pick_seed, float *p_dev, float *v_dev, void *stream)
{
    if (!s) return DBAZ_EINVAL;
    if (!s->solved) return fail(s->err, DBAZ_ESTATE, "dbaz_perfect_policy before dbaz_solver_solve");
    if (n < 0 || (n > 0 && (!x_dev || !p_dev || !v_dev))) return fail(s->err, DBAZ_EINVAL, "dbaz_perfect_policy: bad argument (n = %d)", n);
    if (n == 0) return DBAZ_OK;
    CHECK_HIP(s->err, hipSetDevice(s->dev));
    launch_eval<int16_t>(s, (hipStream_t)stream, x_dev, nullptr, nullptr, n, pick_seed, p_dev, v_dev, s->g.A);
    CHECK_HIP(s->err, hipGetLastError());
    return DBAZ_OK;
}

// ---- the engine's side (solver.h): the table behind the evaluator boundary
bool solver_serves(const dbaz_solver *s, int rows, int cols, int device, bool *solved)
{
    *solved = s->solved;
    return s->g.rows == rows && s->g.cols == cols && s->dev == device;
}

void solver_forward(const dbaz_solver *s, hipStream_t stream, const float *feat, const int32_t *list_dev, const int32_t *n_dev, int max_n,
                    uint64_t pick_seed, float *P, float *V, int AS)
{
    launch_eval<float>(s, stream, feat, list_dev, n_dev, max_n, pick_seed, P, V, AS);
}

// ====================================================================================
// Deep endgames: positions with F <= 31 free edges on any board (A <= DBAZ_MAX_A), solved by the kernels above into
// a pool of tables, and feature rows answered each from its table
// ====================================================================================
// D depends only on which edges are free, so a position is a game over the 2^F subsets of its free edges, and every position that
// can follow it is an entry of the same table.  position_geometry (position_geo.h) turns a root row into the solve geometry -- F
// edges, `other` over the compact edges -- and k_solver_subcube / k_solver_layer solve it into int8 T[2^F] in HBM as they solve a
// whole board.
//
// dbaz_tables owns n_tables slots of 2^max_free bytes.  A solve takes n <= n_tables roots: root i is solved into slot i, the roots
// of equal F sharing their launches (deep_batch.h).  Per root the device keeps a BatchGeo (in plan order, for the solve) and a
// DeepRoot (by root index, for the rows).  k_tables_score and k_tables_targets then answer rows, the root of row r being
// table_of[r]; an index outside [0, n_solved) is "not served", decided before any address is formed from it.  dbaz_deep is a pool
// of ONE table: the same functions with n = 1, every row answered from table 0 (table_of == nullptr), plus k_deep_policy.
//
// A row is SERVED when its free real edges are a subset of its root's.  One wavefront per row reads it against the root and
// the table: table_row (table_row.h), with the served check.
static_assert(POSITION_NO_BOX == SOLVER_NO_BOX && POSITION_MAX_FREE == SOLVER_MAX_E, "position_geo.h restates solver.h");
static_assert(DEEP_BATCH_MAX_FREE == SOLVER_MAX_E && DEEP_BATCH_MIN_LOW == SOLVER_MIN_LOW && DEEP_BATCH_MAX_LOW == SOLVER_MAX_LOW &&
                  DEEP_BATCH_MAX_HIGH == SOLVER_MAX_HIGH && DEEP_BATCH_LAYER_THREADS == 256,
              "deep_batch.h restates solver.h");

#define DEEP_DEFAULT_FREE 24 // 16 MiB, the size of the solved 3x3 board
#define DEEP_WAVES 4
#define TABLES_DEFAULT 64    // tables of a pool: 1 GiB at the default max_free

// A table's root, read from HBM by the wavefronts that answer its rows (table_row.h).  The board is not restated here: every
// kernel that reads a root has the pool's TablesBoard in its arguments.
struct DeepRoot {
    int32_t F;
    uint64_t free_edges[4];               // the root's free real edges by action index
    uint32_t other[SOLVER_MAX_E][2];      // solver_move_q's box masks over the compact edges
    uint8_t act[SOLVER_MAX_E + 1];        // compact edge -> action index
};

// device scratch that grows on demand and keeps nothing across a growth
struct DevScratch {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t need(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 2 + 256;
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        else p = nullptr;
        return e;
    }
};

// what one dbaz_replay_exact_targets call needs besides the pool; one call at a time per handle
struct ReplayScratch {
    DevScratch keys, keys2, idx, idx2; // (game_idx, move_idx) and the row index beside it, before and after the sort
    DevScratch n_free, flag, gid, gstart, games, first, cum, tmp, small;
    std::vector<hipEvent_t> marks;     // the call's timeline
};

struct dbaz_tables {
    TablesBoard board;
    int dev = 0, max_free = 0, n_tables = 0;
    const char *api = "dbaz_tables";      // the family a message names
    int8_t *T = nullptr;                  // [n_tables][2^max_free]; root i's table is the first 2^F_i bytes of slot i
    BatchGeo *geo_dev = nullptr;          // [n_tables], in the order of the last solve's plan
    DeepRoot *roots_dev = nullptr;        // [n_tables], by root index
    int8_t *d0_dev = nullptr;             // [n_tables]
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t used = nullptr;            // behind the last kernel that reads the pool on a caller's stream: the next solve waits for it
    hipEvent_t caller = nullptr;          // dbaz_replay_exact_targets: where the caller's stream stood when the call began
    ReplayScratch replay;
    int n_solved = 0;
    std::vector<int32_t> n_free, d0;      // of the solved roots
    std::vector<BatchGeo> geo_host;       // what the last solve uploaded; alive until its copies are done
    std::vector<DeepRoot> roots_host;
    std::vector<WorkLists> lists;
    double solve_ms = -1.0;
    std::string err;
};

// A pool of one table.  Everything dbaz_deep_info reports is the pool's: no root solved means no table.
struct dbaz_deep : dbaz_tables {};

// dbaz_endgame_score's outputs of the served rows, plus `served`, for one row of one wavefront.  q[a] goes out once per action
// slot: the lane of slot a fetches the Q of the slot's compact edge (edge_rank).  policy_mass is row_members' S.
static __device__ __forceinline__ void deep_score_row(const TablesBoard &B, const DeepRoot &R, const int8_t *__restrict__ Tb,
                                                      const int16_t *__restrict__ x, const float *__restrict__ pi, int r, int lane,
                                                      int8_t *__restrict__ value, int8_t *__restrict__ diff, int8_t *__restrict__ q,
                                                      float *__restrict__ mass, int16_t *__restrict__ n_free, uint8_t *__restrict__ served)
{
    const int A = B.A;
    const TableRow d = table_row<true>(B, R, R.F, Tb, x + (size_t)r * 3 * B.HW, lane);
    const int t = d.served ? (int)Tb[d.m] : -128;
    const int v = !d.served ? 0 : d.open ? sgn(d.f.margin + t) : d.f.res;
    int8_t *qr = q + (size_t)r * A;
#pragma unroll
    for (int w = 0; w < DBAZ_MAX_A / 64; w++) {
        const int a = w * 64 + lane;
        const int qc = __shfl(d.q, edge_rank(R.free_edges, a) & 63);
        const bool is_cand = d.served && d.open && ((d.row_free[w] >> lane) & 1ull);
        if (a < A) qr[a] = (int8_t)(is_cand ? qc : -128);
    }
    float sum = 0.0f;
    if (mass) sum = row_members(d.cand, d.f.margin, d.q, v, d.cand ? pi[(size_t)r * A + d.a] : 0.0f, R.F).sum;
    if (lane == 0) {
        value[r] = (int8_t)v;
        diff[r] = (int8_t)t;
        n_free[r] = (int16_t)d.n_free;
        served[r] = d.served ? 1 : 0;
        if (mass) mass[r] = sum;
    }
}

// T[slot i][0], the score difference of root i for its mover
__global__ void __launch_bounds__(256) k_tables_heads(const int8_t *__restrict__ T, int stride_bits, int n, int8_t *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = T[(size_t)i << stride_bits];
}

// One wavefront per row: the root of row r = roots[table_of[r]] and its table = T + table_of[r] * 2^stride_bits; table_of == nullptr
// means table 0 for every row (the pool of one).
__global__ void __launch_bounds__(64 * DEEP_WAVES) k_tables_score(TablesBoard B, const DeepRoot *__restrict__ roots, int n_solved,
                                                                  const int8_t *__restrict__ T, int stride_bits, const int16_t *__restrict__ x,
                                                                  const float *__restrict__ pi, const int32_t *__restrict__ table_of, int n,
                                                                  int8_t *__restrict__ value, int8_t *__restrict__ diff, int8_t *__restrict__ q,
                                                                  float *__restrict__ mass, int16_t *__restrict__ n_free, uint8_t *__restrict__ served)
{
    const int lane = threadIdx.x & 63;
    for (int r = blockIdx.x * DEEP_WAVES + (threadIdx.x >> 6); r < n; r += gridDim.x * DEEP_WAVES) {
        const int t = table_of ? __builtin_amdgcn_readfirstlane(table_of[r]) : 0; // one row per wavefront: a scalar, so are the root's reads
        if ((unsigned)t >= (unsigned)n_solved) { // not served: no root, no table
            uint64_t row_free[4];
            const int nf = row_free_edges(B, x + (size_t)r * 3 * B.HW, lane, row_free);
            int8_t *qr = q + (size_t)r * B.A;
            for (int a = lane; a < B.A; a += 64) qr[a] = -128;
            if (lane == 0) {
                value[r] = 0;
                diff[r] = -128;
                n_free[r] = (int16_t)nf;
                served[r] = 0;
                if (mass) mass[r] = 0.0f;
            }
            continue;
        }
        deep_score_row(B, roots[t], T + ((size_t)t << stride_bits), x, pi, r, lane, value, diff, q, mass, n_free, served);
    }
}

// dbaz_exact_targets' rule (include/dbaz.h) with v and q from the row's table: a row that is not served or of a finished game is
// left alone; otherwise z <- v and pi by pi_mode over the members (row_members, relabel_entry: table_row.h).  pi and z are read
// and written by the same wavefront only.
__global__ void __launch_bounds__(64 * DEEP_WAVES) k_tables_targets(TablesBoard B, const DeepRoot *__restrict__ roots, int n_solved,
                                                                    const int8_t *__restrict__ T, int stride_bits, const int16_t *__restrict__ x,
                                                                    const int32_t *__restrict__ table_of, int n, int pi_mode, int z_mode, float *pi,
                                                                    float *z, int16_t *__restrict__ n_free, float *__restrict__ mass,
                                                                    uint8_t *__restrict__ relabelled)
{
    const int lane = threadIdx.x & 63;
    for (int r = blockIdx.x * DEEP_WAVES + (threadIdx.x >> 6); r < n; r += gridDim.x * DEEP_WAVES) {
        const int16_t *xr = x + (size_t)r * 3 * B.HW;
        const int t = __builtin_amdgcn_readfirstlane(table_of[r]); // one row per wavefront: a scalar, so are the root's reads
        int nf = 0;
        bool touched = false;
        float sum = 0.0f;
        if ((unsigned)t >= (unsigned)n_solved) {
            uint64_t row_free[4];
            nf = row_free_edges(B, xr, lane, row_free);
        } else {
            const DeepRoot &R = roots[t];
            const int8_t *Tb = T + ((size_t)t << stride_bits);
            const TableRow d = table_row<true>(B, R, R.F, Tb, xr, lane);
            nf = d.n_free;
            if (d.served && d.open) {
                touched = true;
                const int v = sgn(d.f.margin + (int)Tb[d.m]);
                float *pr = pi ? pi + (size_t)r * B.A : nullptr;
                const RowMembers M = row_members(d.cand, d.f.margin, d.q, v, pr && d.cand ? pr[d.a] : 0.0f, R.F);
                sum = M.sum;
                if (pi_mode) {
#pragma unroll
                    for (int w = 0; w < DBAZ_MAX_A / 64; w++) {
                        const int a = w * 64 + lane;
                        const bool member = ((d.row_free[w] >> lane) & 1ull) && ((M.set >> (edge_rank(R.free_edges, a) & 31)) & 1u);
                        if (a < B.A) pr[a] = relabel_entry(M, pi_mode, member, pr[a]);
                    }
                }
                if (lane == 0 && z_mode) z[r] = (float)v;
            }
        }
        if (lane == 0) {
            if (n_free) n_free[r] = (int16_t)nf;
            if (mass) mass[r] = sum;
            if (relabelled) relabelled[r] = touched ? 1 : 0;
        }
    }
}

// ---- exact targets on packed replay rows (dbaz_replay_exact_targets, include/dbaz.h) ---------------------------
// The rows of one call lie in HBM as the engine packed them (replay_row.h), in any order.  k_replay_scan keys every row by
// (game_idx, move_idx) and counts its free edges; a radix sort of the keys puts each game's rows together in move order;
// k_replay_flags / an inclusive scan / k_replay_gstart cut the sorted rows into games (and flag a key that occurs twice);
// k_replay_games finds each game's root.  Per chunk of roots (replay_chunks.h) k_replay_roots builds the geometries where the root
// rows lie, the solving kernels fill the chunk's tables, and k_replay_relabel rewrites the candidate rows in place.
static __device__ __forceinline__ uint32_t slot_box_other(const TablesBoard &B, const uint64_t (&fe)[4], int bl, int bc, int a); // below, with k_slot_requests

#define REPLAY_WAVES 4
#define REPLAY_COUNTERS (4 + SOLVER_MAX_E + 1) // relabelled, finished, unserved, z_changed, by_free[32]

static __device__ __forceinline__ unsigned long long replay_key(int32_t game, int16_t move)
{
    return ((unsigned long long)((uint32_t)game ^ 0x80000000u) << 16) | (unsigned long long)(uint16_t)((uint16_t)move ^ 0x8000u);
}

// One wavefront per packed row: the sort key, the row's own index beside it, and F from the edge planes.
__global__ void __launch_bounds__(64 * REPLAY_WAVES) k_replay_scan(TablesBoard B, const unsigned char *__restrict__ rows, int row_bytes, int n,
                                                                   unsigned long long *__restrict__ keys, int32_t *__restrict__ idx,
                                                                   int32_t *__restrict__ n_free)
{
    const int lane = threadIdx.x & 63;
    for (int r = blockIdx.x * REPLAY_WAVES + (threadIdx.x >> 6); r < n; r += gridDim.x * REPLAY_WAVES) {
        const unsigned char *row = rows + (size_t)r * row_bytes;
        uint64_t fe[4];
        const int F = row_free_edges(B, reinterpret_cast<const int16_t *>(row + ROW_X_OFF), lane, fe);
        if (lane == 0) {
            keys[r] = replay_key(*reinterpret_cast<const int32_t *>(row + ROW_GAME_OFF), *reinterpret_cast<const int16_t *>(row + ROW_MOVE_OFF));
            idx[r] = r;
            n_free[r] = F;
        }
    }
}

// One thread per sorted position: a new game starts here; a key equal to its predecessor's sets hdr[0].
__global__ void __launch_bounds__(256) k_replay_flags(const unsigned long long *__restrict__ keys, int n, int32_t *__restrict__ flag,
                                                      int32_t *__restrict__ hdr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool first = i == 0 || (keys[i] >> 16) != (keys[i - 1] >> 16);
    if (i > 0 && keys[i] == keys[i - 1]) atomicOr(hdr, 1);
    flag[i] = first ? 1 : 0;
}

// gid: the inclusive sum of flag.  gstart[g] = where game g begins among the sorted rows, gstart[games] = n; hdr[1] = games.
__global__ void __launch_bounds__(256) k_replay_gstart(const int32_t *__restrict__ flag, const int32_t *__restrict__ gid, int n,
                                                       int32_t *__restrict__ gstart, int32_t *__restrict__ hdr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) gstart[gid[i] - 1] = i;
    if (i == n - 1) {
        gstart[gid[i]] = n;
        hdr[1] = gid[i];
    }
}

// One lane per game: its root is its first row in move order with F <= max_free.  root_of (may be null): per row the row index of
// its game's root if the row is that root or comes after it, else -1.  Nothing is written once a duplicate key was flagged.
__global__ void __launch_bounds__(256) k_replay_games(const unsigned long long *__restrict__ keys, const int32_t *__restrict__ idx,
                                                      const int32_t *__restrict__ n_free, const int32_t *__restrict__ gstart,
                                                      const int32_t *__restrict__ hdr, int n, int max_free, ReplayGame *__restrict__ games,
                                                      int32_t *__restrict__ root_of)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (hdr[0] != 0 || g >= min(hdr[1], n)) return;
    const int lo = gstart[g], hi = min(gstart[g + 1], n);
    int first = -1, root_row = -1, F = -1;
    for (int i = lo; i < hi; i++) {
        const int r = idx[i];
        if ((unsigned)r >= (unsigned)n) continue; // never outside the caller's rows
        if (first < 0 && n_free[r] <= max_free) {
            first = i;
            root_row = r;
            F = n_free[r];
        }
        if (root_of) root_of[r] = root_row;
    }
    ReplayGame out;
    out.game_idx = (int32_t)((uint32_t)(keys[lo] >> 16) ^ 0x80000000u);
    out.F = F;
    out.first = first < 0 ? hi : first;
    out.end = hi;
    games[g] = out;
}

// The device form of position_geometry, one wavefront per root of the chunk: root k = the row at sorted position first[k], into
// geo[k] (slot k) for the solve and roots[k] for the rows.  Lane l looks at action slots l, 64 + l, ...; a free one writes its
// compact edge's entries, the box neighbours in the order of the board's box scan; lanes F .. 31 write the entries no edge owns.
// A row with more than max_free free edges (the scan has seen to it that there is none) gets an empty root, which serves nothing.
__global__ void __launch_bounds__(64 * REPLAY_WAVES) k_replay_roots(TablesBoard B, int max_free, const unsigned char *__restrict__ rows, int row_bytes,
                                                                    int n, const int32_t *__restrict__ idx, const int32_t *__restrict__ first,
                                                                    int n_roots, BatchGeo *__restrict__ geo, DeepRoot *__restrict__ roots)
{
    const int lane = threadIdx.x & 63, W = B.cols + 1;
    for (int k = blockIdx.x * REPLAY_WAVES + (threadIdx.x >> 6); k < n_roots; k += gridDim.x * REPLAY_WAVES) {
        const int pos = first[k];
        const int r = (unsigned)pos < (unsigned)n ? idx[pos] : -1;
        uint64_t fe[4] = {0ull, 0ull, 0ull, 0ull};
        int F = 0;
        if ((unsigned)r < (unsigned)n) F = row_free_edges(B, reinterpret_cast<const int16_t *>(rows + (size_t)r * row_bytes + ROW_X_OFF), lane, fe);
        if (F > max_free) {
            F = 0;
            fe[0] = fe[1] = fe[2] = fe[3] = 0ull;
        }
        BatchGeo *bg = geo + k;
        DeepRoot *R = roots + k;
        if (lane >= F && lane <= SOLVER_MAX_E) {
            R->act[lane] = 0;
            if (lane < SOLVER_MAX_E) bg->other[lane][0] = bg->other[lane][1] = R->other[lane][0] = R->other[lane][1] = SOLVER_NO_BOX;
        }
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int a = w * 64 + lane;
            if (!((fe[w] >> lane) & 1ull)) continue;
            const int j = edge_rank(fe, a);
            uint32_t o[2] = {SOLVER_NO_BOX, SOLVER_NO_BOX};
            int used = 0;
            if (a < B.HW) { // a horizontal edge: the boxes above and below
                const int l = a / W, c = a % W;
                if (l >= 1) o[used++] = slot_box_other(B, fe, l - 1, c, a);
                if (l < B.rows) o[used++] = slot_box_other(B, fe, l, c, a);
            } else { // a vertical edge: the boxes to its left and right
                const int l = (a - B.HW) / W, c = (a - B.HW) % W;
                if (c >= 1) o[used++] = slot_box_other(B, fe, l, c - 1, a);
                if (c < B.cols) o[used++] = slot_box_other(B, fe, l, c, a);
            }
            bg->other[j][0] = R->other[j][0] = o[0];
            bg->other[j][1] = R->other[j][1] = o[1];
            R->act[j] = (uint8_t)a;
        }
        if (lane == 0) {
            bg->F = R->F = F;
            bg->slot = k;
            for (int w = 0; w < 4; w++) R->free_edges[w] = fe[w];
        }
    }
}

// One wavefront per candidate row of the chunk.  The candidates of the chunk's root k are the sorted positions
// first[k] .. first[k] + (cum[k + 1] - cum[k]) - 1, candidate number c - cum[0] of the chunk belongs to the root with
// cum[k] <= c < cum[k + 1].  The rule of include/dbaz.h in visit space: a row that its root does not serve or whose game is over
// is only counted; otherwise O comes from the table as in k_tables_targets, the visits on O are summed in int32, and the
// row's visits and z are rewritten by the wavefront that read them.  The visits are 2-byte aligned (replay_row.h): they are read and
// written as halves.  Counters: per workgroup in LDS, added once.
__global__ void __launch_bounds__(64 * REPLAY_WAVES) k_replay_relabel(TablesBoard B, const DeepRoot *__restrict__ roots, int n_roots,
                                                                      const int8_t *__restrict__ T, int stride_bits, unsigned char *rows,
                                                                      int row_bytes, int n, const int32_t *__restrict__ idx,
                                                                      const int32_t *__restrict__ first, const int32_t *__restrict__ cum,
                                                                      int pi_mode, int z_mode, unsigned long long *__restrict__ counters)
{
    __shared__ unsigned int cnt[REPLAY_COUNTERS];
    for (int i = threadIdx.x; i < REPLAY_COUNTERS; i += blockDim.x) cnt[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int c0 = cum[0], total = cum[n_roots] - c0;
    for (int w = blockIdx.x * REPLAY_WAVES + (threadIdx.x >> 6); w < total; w += gridDim.x * REPLAY_WAVES) {
        const int c = c0 + w;
        int lo = 0, hi = n_roots; // the last k with cum[k] <= c: the same search in every lane
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (cum[mid] <= c) lo = mid;
            else hi = mid;
        }
        const int k = lo, pos = first[k] + (c - cum[k]);
        const int r = (unsigned)pos < (unsigned)n ? idx[pos] : -1;
        if ((unsigned)r >= (unsigned)n) continue; // never outside the caller's rows
        unsigned char *row = rows + (size_t)r * row_bytes;
        const DeepRoot &R = roots[k];
        const int8_t *Tb = T + ((size_t)k << stride_bits);
        const TableRow d = table_row<true>(B, R, R.F, Tb, reinterpret_cast<const int16_t *>(row + ROW_X_OFF), lane);
        if (!d.served || !d.open) {
            if (lane == 0) atomicAdd(&cnt[d.served ? 1 : 2], 1u);
            continue;
        }
        const int v = sgn(d.f.margin + (int)Tb[d.m]);
        const uint32_t set = (uint32_t)__ballot(d.cand && sgn(d.f.margin + d.q) == v);
        uint16_t *vis = reinterpret_cast<uint16_t *>(row + ROW_X_OFF + (size_t)3 * B.HW * 2);
        int32_t mine[DBAZ_MAX_A / 64];
        bool member[DBAZ_MAX_A / 64];
        int32_t sum = 0;
#pragma unroll
        for (int q = 0; q < DBAZ_MAX_A / 64; q++) {
            const int a = q * 64 + lane;
            member[q] = ((d.row_free[q] >> lane) & 1ull) && ((set >> (edge_rank(R.free_edges, a) & 31)) & 1u);
            mine[q] = a < B.A ? (int32_t)((uint32_t)vis[2 * a] | ((uint32_t)vis[2 * a + 1] << 16)) : 0;
            if (member[q]) sum += mine[q];
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (pi_mode) {
#pragma unroll
            for (int q = 0; q < DBAZ_MAX_A / 64; q++) {
                const int a = q * 64 + lane;
                const int32_t out = !member[q] ? 0 : (pi_mode == 1 || sum == 0) ? 1 : mine[q];
                if (a < B.A) {
                    vis[2 * a] = (uint16_t)((uint32_t)out & 0xFFFFu);
                    vis[2 * a + 1] = (uint16_t)((uint32_t)out >> 16);
                }
            }
        }
        if (lane == 0) {
            int8_t *z = reinterpret_cast<int8_t *>(row + ROW_Z_OFF);
            if ((int)*z != v) atomicAdd(&cnt[3], 1u);
            if (z_mode) *z = (int8_t)v;
            atomicAdd(&cnt[0], 1u);
            atomicAdd(&cnt[4 + min(d.n_free, SOLVER_MAX_E)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < REPLAY_COUNTERS; i += blockDim.x)
        if (cnt[i]) atomicAdd(&counters[i], (unsigned long long)cnt[i]);
}

// The table as a (p, v) evaluator with dbaz_exact_policy's outputs: one-hot on endgame_pick's move, v the true result.  A finished
// game: p = 0, v = get_result; a row that is not served: p = 0, v = 0.  One root, one table (dbaz_deep_policy).
__global__ void __launch_bounds__(64 * DEEP_WAVES) k_deep_policy(TablesBoard B, const DeepRoot *__restrict__ root, const int8_t *__restrict__ Tb,
                                                                 const int16_t *__restrict__ x, int n, uint64_t pick_seed, float *__restrict__ P,
                                                                 float *__restrict__ V, uint8_t *__restrict__ served)
{
    const DeepRoot &R = *root;
    const int lane = threadIdx.x & 63, A = B.A;
    for (int r = blockIdx.x * DEEP_WAVES + (threadIdx.x >> 6); r < n; r += gridDim.x * DEEP_WAVES) {
        const TableRow d = table_row<true>(B, R, R.F, Tb, x + (size_t)r * 3 * B.HW, lane);
        const int pick = endgame_pick(d.cand, d.q, d.a, pick_seed);
        float *pr = P + (size_t)r * A;
        for (int a = lane; a < A; a += 64) pr[a] = a == pick ? 1.0f : 0.0f;
        if (lane == 0) {
            V[r] = !d.served ? 0.0f : (float)(d.open ? sgn(d.f.margin + (int)Tb[d.m]) : d.f.res);
            served[r] = d.served ? 1 : 0;
        }
    }
}

// ---- host: the static functions take the pool; dbaz_tables_* and dbaz_deep_* are the two families of entries over them
static void tables_release(dbaz_tables *t)
{
    (void)hipSetDevice(t->dev);
    for (void *b : {(void *)t->T, (void *)t->geo_dev, (void *)t->roots_dev, (void *)t->d0_dev})
        if (b) (void)hipFree(b);
    free_work_lists(t->lists);
    ReplayScratch &rs = t->replay;
    for (DevScratch *b : {&rs.keys, &rs.keys2, &rs.idx, &rs.idx2, &rs.n_free, &rs.flag, &rs.gid, &rs.gstart, &rs.games, &rs.first, &rs.cum, &rs.tmp, &rs.small})
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : rs.marks) (void)hipEventDestroy(e);
    for (hipEvent_t e : {t->ev0, t->ev1, t->used, t->caller})
        if (e) (void)hipEventDestroy(e);
    if (t->stream) (void)hipStreamDestroy(t->stream);
}

// Checks the arguments, then makes the stream and the events; no table memory before the first solve.  err: the family's slot
// for a failed create.  On a failure nothing is left on the device.
static int tables_init(dbaz_tables *t, std::string &err, const char *api, int rows, int cols, int device, int max_free, int n_tables)
{
    if (rows < 1 || cols < 1) return fail(err, DBAZ_EINVAL, "board %dx%d: rows and cols must be >= 1", rows, cols);
    const long long A = 2ll * (rows + 1ll) * (cols + 1ll);
    if (A > DBAZ_MAX_A) return fail(err, DBAZ_EINVAL, "board %dx%d has %lld action slots: at most %d are supported", rows, cols, A, DBAZ_MAX_A);
    if (max_free < 0 || max_free > SOLVER_MAX_E)
        return fail(err, DBAZ_EINVAL, "max_free %d: a position's table holds 2^F bytes, 1 <= max_free <= %d (0 = %d)", max_free, SOLVER_MAX_E,
                    DEEP_DEFAULT_FREE);
    if (n_tables < 0 || n_tables > DEEP_BATCH_MAX_TABLES)
        return fail(err, DBAZ_EINVAL, "n_tables %d: a pool holds 1 <= n_tables <= %d tables (0 = %d)", n_tables, DEEP_BATCH_MAX_TABLES, TABLES_DEFAULT);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(err, DBAZ_EDEVICE, "no HIP device %d (there is no CPU fallback)", device);
    t->api = api;
    t->board = tables_board(rows, cols);
    t->dev = device;
    t->max_free = max_free == 0 ? DEEP_DEFAULT_FREE : max_free;
    t->n_tables = n_tables == 0 ? TABLES_DEFAULT : n_tables;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreate(&t->stream);
    if (e == hipSuccess) e = hipEventCreate(&t->ev0);
    if (e == hipSuccess) e = hipEventCreate(&t->ev1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->used, hipEventDisableTiming);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_solver_subcube, hipFuncAttributeMaxDynamicSharedMemorySize, 1 << SOLVER_MAX_LOW);
    if (e != hipSuccess) {
        const std::string msg = hipGetErrorString(e);
        (void)hipGetLastError();
        tables_release(t);
        return fail(err, DBAZ_EDEVICE, "%s_create: setup failed: %s", api, msg.c_str());
    }
    return DBAZ_OK;
}

template <typename H>
static int tables_create(H **out, std::string &err, const char *api, int rows, int cols, int device, int max_free, int n_tables)
{
    if (!out) return fail(err, DBAZ_EINVAL, "null argument");
    *out = nullptr;
    H *h = new H();
    const int rc = tables_init(h, err, api, rows, cols, device, max_free, n_tables);
    if (rc == DBAZ_OK) *out = h;
    else delete h;
    return rc;
}

// The pool and the per-root arrays, allocated by the first solve and kept.
static int tables_pool(dbaz_tables *t)
{
    CHECK_HIP(t->err, hipSetDevice(t->dev));
    if (t->T) return DBAZ_OK;
    const size_t bytes = (size_t)deep_batch_slot_offset(t->n_tables, t->max_free); // 64 bits: 64 x 2^31 is past 32
    hipError_t e = hipMalloc((void **)&t->T, bytes);
    if (e == hipSuccess && !t->geo_dev) e = hipMalloc((void **)&t->geo_dev, (size_t)t->n_tables * sizeof(BatchGeo));
    if (e == hipSuccess && !t->roots_dev) e = hipMalloc((void **)&t->roots_dev, (size_t)t->n_tables * sizeof(DeepRoot));
    if (e == hipSuccess && !t->d0_dev) e = hipMalloc((void **)&t->d0_dev, (size_t)t->n_tables);
    if (e != hipSuccess) {
        if (t->T) (void)hipFree(t->T);
        t->T = nullptr;
        (void)hipGetLastError();
        return fail(t->err, DBAZ_EDEVICE, "pool of %d tables, %zu bytes: %s", t->n_tables, bytes, hipGetErrorString(e));
    }
    return DBAZ_OK;
}

// lists[g]: the entry of t->lists that group g of the plan solves with (-1 for a plain group)
static int tables_plan_lists(dbaz_tables *t, const DeepBatchPlan &plan, std::vector<int> &lists)
{
    lists.assign(plan.groups.size(), -1);
    for (size_t g = 0; g < plan.groups.size(); g++)
        if (!plan.groups[g].plain) {
            hipError_t e = hipSuccess;
            lists[g] = work_lists(t->lists, plan.groups[g].F, plan.groups[g].L, &e);
            if (e != hipSuccess)
                return fail(t->err, DBAZ_EDEVICE, "work lists of F = %d, L = %d: %s", plan.groups[g].F, plan.groups[g].L, hipGetErrorString(e));
        }
    return DBAZ_OK;
}

// The plan's launches on the handle's stream, back to back -- no host synchronisation between groups -- over the geometries
// t->geo_dev holds in plan order, and then every root's T[0]
static void tables_launch_plan(dbaz_tables *t, const DeepBatchPlan &plan, const std::vector<int> &lists, int n_roots)
{
    for (const DeepBatchLaunch &l : plan.launches) {
        const DeepBatchGroup &g = plan.groups[l.group];
        const dim3 grid(l.grid_x, l.grid_y);
        if (g.plain) k_solver_layer<<<grid, 256, 0, t->stream>>>(t->geo_dev + g.first, t->T, t->max_free, l.k);
        else {
            const WorkLists &w = t->lists[(size_t)lists[l.group]];
            k_solver_subcube<<<grid, SOLVER_THREADS, (size_t)1 << g.L, t->stream>>>(t->geo_dev + g.first, t->T, t->max_free, g.L,
                                                                                   w.hi_dev + w.hoff[l.k], w.low_dev, w.off_dev);
        }
    }
    k_tables_heads<<<(n_roots + 255) / 256, 256, 0, t->stream>>>(t->T, t->max_free, n_roots, t->d0_dev);
}

static int tables_solve(dbaz_tables *t, int32_t n_roots, const int16_t *roots_host, int32_t low_bits)
{
    t->n_solved = 0; // whatever happens below, the old tables are not handed out again
    t->n_free.clear();
    t->d0.clear();
    if (!roots_host) return fail(t->err, DBAZ_EINVAL, "%s_solve: null root rows", t->api);
    if (n_roots < 1) return fail(t->err, DBAZ_EINVAL, "%s_solve: %d roots (at least 1, at most the pool's %d)", t->api, n_roots, t->n_tables);
    if (n_roots > t->n_tables) return fail(t->err, DBAZ_EINVAL, "%s_solve: %d roots do not fit a pool of %d tables", t->api, n_roots, t->n_tables);
    const TablesBoard &B = t->board;
    std::vector<PositionGeo> pg((size_t)n_roots);
    std::vector<int32_t> F((size_t)n_roots);
    for (int i = 0; i < n_roots; i++) {
        position_geometry(B.rows, B.cols, roots_host + (size_t)i * 3 * B.HW, pg[i]);
        F[i] = pg[i].F;
    }
    DeepBatchPlan plan;
    if (deep_batch_plan(F.data(), n_roots, t->max_free, t->n_tables, low_bits, plan) != 0)
        return fail(t->err, DBAZ_EINVAL, "%s_solve: %s", t->api, plan.error.c_str());
    std::vector<int> lists;
    int rc = tables_pool(t);
    if (rc == DBAZ_OK) rc = tables_plan_lists(t, plan, lists);
    if (rc != DBAZ_OK) return rc;

    t->geo_host.assign((size_t)n_roots, BatchGeo());
    t->roots_host.assign((size_t)n_roots, DeepRoot());
    for (int at = 0; at < n_roots; at++) {
        const int i = plan.order[at];
        BatchGeo &bg = t->geo_host[at];
        DeepRoot &R = t->roots_host[i];
        bg.F = R.F = F[i];
        bg.slot = i;
        for (int w = 0; w < 4; w++) R.free_edges[w] = pg[i].free_edges[w];
        for (int j = 0; j < SOLVER_MAX_E; j++) {
            R.act[j] = pg[i].act[j];
            for (int k = 0; k < 2; k++) R.other[j][k] = bg.other[j][k] = pg[i].other[j][k];
        }
    }
    hipError_t e = hipStreamWaitEvent(t->stream, t->used, 0); // rows still being answered from the old tables and roots
    if (e == hipSuccess) e = hipMemcpyAsync(t->geo_dev, t->geo_host.data(), (size_t)n_roots * sizeof(BatchGeo), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->roots_dev, t->roots_host.data(), (size_t)n_roots * sizeof(DeepRoot), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipEventRecord(t->ev0, t->stream);
    if (e == hipSuccess) {
        tables_launch_plan(t, plan, lists, n_roots);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(t->ev1, t->stream);
    std::vector<int8_t> heads((size_t)n_roots);
    if (e == hipSuccess) e = hipMemcpyAsync(heads.data(), t->d0_dev, (size_t)n_roots, hipMemcpyDeviceToHost, t->stream);
    const hipError_t done = hipStreamSynchronize(t->stream); // also on a failure above: the host buffers leave scope
    if (e == hipSuccess) e = done;
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, t->ev0, t->ev1);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(t->err, DBAZ_EDEVICE, "solve failed: %s", hipGetErrorString(e));
    }
    t->n_free.assign(F.begin(), F.end());
    t->d0.assign(heads.begin(), heads.end());
    t->solve_ms = ms;
    t->n_solved = n_roots;
    return DBAZ_OK;
}

static int tables_table(dbaz_tables *t, int32_t i, int8_t *host_dst, int64_t first, int64_t count)
{
    if (t->n_solved == 0) return fail(t->err, DBAZ_ESTATE, "%s_table before a successful %s_solve", t->api, t->api);
    if (i < 0 || i >= t->n_solved) return fail(t->err, DBAZ_EINVAL, "table %d: the last solve filled tables 0 .. %d", i, t->n_solved - 1);
    const int64_t n = (int64_t)1 << t->n_free[(size_t)i];
    if (!host_dst || first < 0 || count < 0 || first > n || count > n - first)
        return fail(t->err, DBAZ_EINVAL, "table slice [%lld, +%lld) outside [0, %lld)", (long long)first, (long long)count, (long long)n);
    if (count == 0) return DBAZ_OK;
    CHECK_HIP(t->err, hipSetDevice(t->dev));
    CHECK_HIP(t->err, hipMemcpy(host_dst, t->T + deep_batch_slot_offset(i, t->max_free) + first, (size_t)count, hipMemcpyDeviceToHost));
    return DBAZ_OK;
}

static unsigned deep_blocks(int n) { return (unsigned)std::min((n + DEEP_WAVES - 1) / DEEP_WAVES, 16384); }

// one_table: every row is answered from table 0 and there is no table_dev (the pool of one)
static int tables_score(dbaz_tables *t, bool one_table, int32_t n, const int16_t *x_dev, const float *pi_dev, const int32_t *table_dev,
                        int8_t *value_dev, int8_t *diff_dev, int8_t *q_dev, float *mass_dev, int16_t *n_free_dev, uint8_t *served_dev, void *stream)
{
    if (t->n_solved == 0) return fail(t->err, DBAZ_ESTATE, "%s_score before a successful %s_solve", t->api, t->api);
    if (n < 0 || (n > 0 && (!x_dev || (!one_table && !table_dev) || !value_dev || !diff_dev || !q_dev || !n_free_dev || !served_dev)) ||
        (pi_dev && !mass_dev))
        return fail(t->err, DBAZ_EINVAL, "%s_score: bad argument (n = %d)", t->api, n);
    if (n == 0) return DBAZ_OK;
    CHECK_HIP(t->err, hipSetDevice(t->dev));
    k_tables_score<<<deep_blocks(n), 64 * DEEP_WAVES, 0, (hipStream_t)stream>>>(t->board, t->roots_dev, t->n_solved, t->T, t->max_free, x_dev, pi_dev,
                                                                               table_dev, n, value_dev, diff_dev, q_dev, pi_dev ? mass_dev : nullptr,
                                                                               n_free_dev, served_dev);
    CHECK_HIP(t->err, hipGetLastError());
    CHECK_HIP(t->err, hipEventRecord(t->used, (hipStream_t)stream));
    return DBAZ_OK;
}

extern "C" const char *dbaz_tables_last_error(const dbaz_tables *t) { return t ? t->err.c_str() : g_tables_error.c_str(); }

extern "C" void dbaz_tables_destroy(dbaz_tables *t)
{
    if (!t) return;
    tables_release(t);
    delete t;
}

extern "C" int dbaz_tables_create(int32_t rows, int32_t cols, int32_t device, int32_t max_free, int32_t n_tables, dbaz_tables **out)
{
    return tables_create(out, g_tables_error, "dbaz_tables", rows, cols, device, max_free, n_tables);
}

extern "C" int dbaz_tables_solve(dbaz_tables *t, int32_t n_roots, const int16_t *roots_host, int32_t low_bits)
{
    return t ? tables_solve(t, n_roots, roots_host, low_bits) : DBAZ_EINVAL;
}

extern "C" int dbaz_tables_info(const dbaz_tables *t, int32_t *n_solved, int64_t *table_bytes, int64_t *pool_bytes, double *solve_ms)
{
    if (!t) return DBAZ_EINVAL;
    if (n_solved) *n_solved = t->n_solved;
    if (table_bytes) *table_bytes = (int64_t)1 << t->max_free;
    if (pool_bytes) *pool_bytes = (int64_t)t->n_tables << t->max_free;
    if (solve_ms) *solve_ms = t->solve_ms;
    return DBAZ_OK;
}

extern "C" int dbaz_tables_roots(const dbaz_tables *t, int32_t *n_free_out, int32_t *d0_out)
{
    if (!t) return DBAZ_EINVAL;
    if (n_free_out) std::copy(t->n_free.begin(), t->n_free.end(), n_free_out);
    if (d0_out) std::copy(t->d0.begin(), t->d0.end(), d0_out);
    return DBAZ_OK;
}

extern "C" int dbaz_tables_table(dbaz_tables *t, int32_t i, int8_t *host_dst, int64_t first, int64_t count)
{
    return t ? tables_table(t, i, host_dst, first, count) : DBAZ_EINVAL;
}

extern "C" int dbaz_tables_score(dbaz_tables *t, int32_t n, const int16_t *x_dev, const float *pi_dev, const int32_t *table_dev, int8_t *value_dev,
                                 int8_t *diff_dev, int8_t *q_dev, float *mass_dev, int16_t *n_free_dev, uint8_t *served_dev, void *stream)
{
    return !t ? DBAZ_EINVAL : tables_score(t, false, n, x_dev, pi_dev, table_dev, value_dev, diff_dev, q_dev, mass_dev, n_free_dev, served_dev, stream);
}

extern "C" int dbaz_tables_targets(dbaz_tables *t, int32_t n, const int16_t *x_dev, const int32_t *table_dev, int32_t pi_mode, int32_t z_mode,
                                   float *pi_dev, float *z_dev, int16_t *n_free_dev, float *mass_dev, uint8_t *relabelled_dev, void *stream)
{
    if (!t) return DBAZ_EINVAL;
    if (t->n_solved == 0) return fail(t->err, DBAZ_ESTATE, "dbaz_tables_targets before a successful dbaz_tables_solve");
    if (pi_mode < 0 || pi_mode > 2 || z_mode < 0 || z_mode > 1)
        return fail(t->err, DBAZ_EINVAL, "dbaz_tables_targets: pi_mode %d / z_mode %d (pi_mode 0 keep, 1 uniform, 2 restrict; z_mode 0 keep, 1 solved)", pi_mode,
                    z_mode);
    if (n < 0 || (n > 0 && (!x_dev || !table_dev || (pi_mode != 0 && !pi_dev) || (z_mode != 0 && !z_dev))))
        return fail(t->err, DBAZ_EINVAL, "dbaz_tables_targets: bad argument (n = %d; a mode other than keep needs its array)", n);
    if (n == 0) return DBAZ_OK;
    CHECK_HIP(t->err, hipSetDevice(t->dev));
    k_tables_targets<<<deep_blocks(n), 64 * DEEP_WAVES, 0, (hipStream_t)stream>>>(t->board, t->roots_dev, t->n_solved, t->T, t->max_free, x_dev, table_dev,
                                                                                 n, pi_mode, z_mode, pi_dev, z_dev, n_free_dev, mass_dev, relabelled_dev);
    CHECK_HIP(t->err, hipGetLastError());
    CHECK_HIP(t->err, hipEventRecord(t->used, (hipStream_t)stream));
    return DBAZ_OK;
}

// ---- dbaz_replay_exact_targets: packed replay rows in, packed replay rows out (kernels: k_replay_* above)
static_assert(sizeof(ReplayGame) == 16, "one game's record as the host reads it back");
#define REPLAY_STATS 8          // rows, games, roots, chunks, relabelled, finished, unserved, z_changed
#define REPLAY_PHASES 5         // scan, group, geometry, solve, relabel

static hipError_t replay_sort(ReplayScratch &rs, int n, hipStream_t s, bool run)
{
    size_t bytes = run ? rs.tmp.cap : 0;
    return hipcub::DeviceRadixSort::SortPairs(run ? rs.tmp.p : nullptr, bytes, (unsigned long long *)rs.keys.p, (unsigned long long *)rs.keys2.p,
                                              (int32_t *)rs.idx.p, (int32_t *)rs.idx2.p, n, 0, 48, s) == hipSuccess
               ? (run ? hipSuccess : rs.tmp.need(bytes))
               : hipErrorUnknown;
}

static hipError_t replay_scan_sum(ReplayScratch &rs, int n, hipStream_t s, bool run)
{
    size_t bytes = run ? rs.tmp.cap : 0;
    return hipcub::DeviceScan::InclusiveSum(run ? rs.tmp.p : nullptr, bytes, (int32_t *)rs.flag.p, (int32_t *)rs.gid.p, n, s) == hipSuccess
               ? (run ? hipSuccess : rs.tmp.need(bytes))
               : hipErrorUnknown;
}

// event `at` of the call's timeline, created the first time a call gets that far
static hipError_t replay_mark(dbaz_tables *t, size_t at)
{
    ReplayScratch &rs = t->replay;
    while (rs.marks.size() <= at) {
        hipEvent_t ev = nullptr;
        const hipError_t e = hipEventCreate(&ev);
        if (e != hipSuccess) return e;
        rs.marks.push_back(ev);
    }
    return hipEventRecord(rs.marks[at], t->stream);
}

extern "C" int dbaz_replay_exact_targets(dbaz_tables *t, void *rows_dev, int64_t n_rows, int32_t row_bytes, int32_t pi_mode, int32_t z_mode,
                                         int32_t *root_of_dev, int64_t *stats_host, void *stream)
{
    if (!t) return DBAZ_EINVAL;
    const TablesBoard &B = t->board;
    if (pi_mode < 0 || pi_mode > 2 || z_mode < 0 || z_mode > 1)
        return fail(t->err, DBAZ_EINVAL, "dbaz_replay_exact_targets: pi_mode %d / z_mode %d (pi_mode 0 keep, 1 uniform, 2 restrict; z_mode 0 keep, 1 solved)",
                    pi_mode, z_mode);
    if (row_bytes != replay_row_bytes(B.HW))
        return fail(t->err, DBAZ_EINVAL, "dbaz_replay_exact_targets: row_bytes %d, a packed replay row of a %dx%d board has %d", row_bytes, B.rows, B.cols,
                    replay_row_bytes(B.HW));
    if (n_rows < 0 || n_rows > 0x7FFFFFF0ll || (n_rows > 0 && !rows_dev) || ((uintptr_t)rows_dev & 7) != 0)
        return fail(t->err, DBAZ_EINVAL, "dbaz_replay_exact_targets: bad rows (n_rows = %lld; the rows are 8-byte aligned and at most 2^31 - 16)",
                    (long long)n_rows);
    if (stats_host) std::fill(stats_host, stats_host + REPLAY_STATS + SOLVER_MAX_E + 1 + REPLAY_PHASES, (int64_t)0);
    if (n_rows == 0) return DBAZ_OK;

    t->n_solved = 0; // the pool is about to be overwritten: the old tables are not handed out again
    t->n_free.clear();
    t->d0.clear();
    const int n = (int)n_rows;
    ReplayScratch &rs = t->replay;
    unsigned char *rows = (unsigned char *)rows_dev;
    int rc = tables_pool(t);
    if (rc != DBAZ_OK) return rc;
    hipError_t e = hipSuccess;
    if (!t->caller) e = hipEventCreateWithFlags(&t->caller, hipEventDisableTiming);
    for (DevScratch *b : {&rs.keys, &rs.keys2})
        if (e == hipSuccess) e = b->need((size_t)n * 8);
    for (DevScratch *b : {&rs.idx, &rs.idx2, &rs.n_free, &rs.flag, &rs.gid})
        if (e == hipSuccess) e = b->need((size_t)n * 4);
    if (e == hipSuccess) e = rs.gstart.need(((size_t)n + 1) * 4);
    if (e == hipSuccess) e = rs.games.need((size_t)n * sizeof(ReplayGame));
    if (e == hipSuccess) e = rs.first.need((size_t)n * 4);
    if (e == hipSuccess) e = rs.cum.need(((size_t)n + 1) * 4);
    if (e == hipSuccess) e = rs.small.need(64 + REPLAY_COUNTERS * 8);
    if (e == hipSuccess) e = replay_sort(rs, n, t->stream, false);
    if (e == hipSuccess) e = replay_scan_sum(rs, n, t->stream, false);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(t->err, DBAZ_EDEVICE, "dbaz_replay_exact_targets: scratch for %d rows: %s", n, hipGetErrorString(e));
    }
    int32_t *hdr = (int32_t *)rs.small.p;                                           // [0]: a key occurs twice; [1]: games
    unsigned long long *counters = (unsigned long long *)((char *)rs.small.p + 64); // [REPLAY_COUNTERS]
    const unsigned row_blocks = deep_blocks(n), lane_blocks = (unsigned)((n + 255) / 256);

    // the rows as the caller's stream leaves them, and the pool after its last readers
    CHECK_HIP(t->err, hipEventRecord(t->caller, (hipStream_t)stream));
    CHECK_HIP(t->err, hipStreamWaitEvent(t->stream, t->caller, 0));
    CHECK_HIP(t->err, hipStreamWaitEvent(t->stream, t->used, 0));
    CHECK_HIP(t->err, hipMemsetAsync(rs.small.p, 0, 64 + REPLAY_COUNTERS * 8, t->stream));
    size_t mark = 0;
    CHECK_HIP(t->err, replay_mark(t, mark++)); // 0
    k_replay_scan<<<row_blocks, 64 * REPLAY_WAVES, 0, t->stream>>>(B, rows, row_bytes, n, (unsigned long long *)rs.keys.p, (int32_t *)rs.idx.p,
                                                                   (int32_t *)rs.n_free.p);
    CHECK_HIP(t->err, replay_mark(t, mark++)); // 1
    CHECK_HIP(t->err, replay_sort(rs, n, t->stream, true));
    const unsigned long long *keys = (const unsigned long long *)rs.keys2.p;
    const int32_t *idx = (const int32_t *)rs.idx2.p;
    k_replay_flags<<<lane_blocks, 256, 0, t->stream>>>(keys, n, (int32_t *)rs.flag.p, hdr);
    CHECK_HIP(t->err, replay_scan_sum(rs, n, t->stream, true));
    k_replay_gstart<<<lane_blocks, 256, 0, t->stream>>>((const int32_t *)rs.flag.p, (const int32_t *)rs.gid.p, n, (int32_t *)rs.gstart.p, hdr);
    k_replay_games<<<lane_blocks, 256, 0, t->stream>>>(keys, idx, (const int32_t *)rs.n_free.p, (const int32_t *)rs.gstart.p, hdr, n, t->max_free,
                                                       (ReplayGame *)rs.games.p, root_of_dev);
    CHECK_HIP(t->err, hipGetLastError());
    CHECK_HIP(t->err, replay_mark(t, mark++)); // 2
    int32_t head[2] = {0, 0};
    CHECK_HIP(t->err, hipMemcpyAsync(head, hdr, sizeof head, hipMemcpyDeviceToHost, t->stream));
    CHECK_HIP(t->err, hipStreamSynchronize(t->stream));
    if (head[0] != 0) return fail(t->err, DBAZ_EINVAL, "dbaz_replay_exact_targets: two rows of one call have the same (game_idx, move_idx)");
    const int n_games = head[1];
    if (n_games < 1 || n_games > n) return fail(t->err, DBAZ_EDEVICE, "dbaz_replay_exact_targets: %d games in %d rows", n_games, n);
    std::vector<ReplayGame> games((size_t)n_games);
    CHECK_HIP(t->err, hipMemcpy(games.data(), rs.games.p, (size_t)n_games * sizeof(ReplayGame), hipMemcpyDeviceToHost));
    ReplayChunks ch;
    if (replay_chunks_plan(games.data(), n_games, n, t->max_free, t->n_tables, ch) != 0)
        return fail(t->err, DBAZ_EDEVICE, "dbaz_replay_exact_targets: the games' records do not tile the %d sorted rows", n);
    const int n_roots = (int)ch.order.size(), n_chunks = (int)ch.chunk_first.size() - 1;

    // per chunk: geometry, solve, relabel -- back to back; the next chunk's solve overwrites the tables behind this chunk's rows
    std::vector<int8_t> heads;
    int last = 0;
    if (n_roots > 0) {
        CHECK_HIP(t->err, hipMemcpyAsync(rs.first.p, ch.first.data(), (size_t)n_roots * 4, hipMemcpyHostToDevice, t->stream));
        CHECK_HIP(t->err, hipMemcpyAsync(rs.cum.p, ch.cum.data(), ((size_t)n_roots + 1) * 4, hipMemcpyHostToDevice, t->stream));
    }
    for (int c = 0; c < n_chunks; c++) {
        const int lo = ch.chunk_first[c], m = ch.chunk_first[c + 1] - lo;
        DeepBatchPlan plan;
        if (deep_batch_plan(ch.n_free.data() + lo, m, t->max_free, t->n_tables, 0, plan) != 0)
            rc = fail(t->err, DBAZ_EDEVICE, "dbaz_replay_exact_targets: chunk %d: %s", c, plan.error.c_str());
        for (int at = 0; rc == DBAZ_OK && at < m; at++)
            if (plan.order[at] != at) rc = fail(t->err, DBAZ_EDEVICE, "dbaz_replay_exact_targets: chunk %d is not in plan order", c);
        std::vector<int> lists;
        if (rc == DBAZ_OK) rc = tables_plan_lists(t, plan, lists);
        if (rc != DBAZ_OK) break;
        const int32_t *first = (const int32_t *)rs.first.p + lo, *cum = (const int32_t *)rs.cum.p + lo;
        const int cand = ch.cum[lo + m] - ch.cum[lo];
        e = replay_mark(t, mark++); // 3 + 3 c
        k_replay_roots<<<deep_blocks(m), 64 * REPLAY_WAVES, 0, t->stream>>>(B, t->max_free, rows, row_bytes, n, idx, first, m, t->geo_dev, t->roots_dev);
        if (e == hipSuccess) e = replay_mark(t, mark++);
        tables_launch_plan(t, plan, lists, m);
        if (e == hipSuccess) e = replay_mark(t, mark++);
        k_replay_relabel<<<deep_blocks(cand), 64 * REPLAY_WAVES, 0, t->stream>>>(B, t->roots_dev, m, t->T, t->max_free, rows, row_bytes, n, idx, first, cum,
                                                                                pi_mode, z_mode, counters);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            rc = fail(t->err, DBAZ_EDEVICE, "dbaz_replay_exact_targets: chunk %d: %s", c, hipGetErrorString(e));
            break;
        }
        last = m;
    }
    if (rc == DBAZ_OK && (e = replay_mark(t, mark++)) != hipSuccess) rc = fail(t->err, DBAZ_EDEVICE, "dbaz_replay_exact_targets: %s", hipGetErrorString(e));
    unsigned long long got[REPLAY_COUNTERS] = {0};
    heads.assign((size_t)last, 0);
    if (rc == DBAZ_OK) {
        e = hipMemcpyAsync(got, counters, sizeof got, hipMemcpyDeviceToHost, t->stream);
        if (e == hipSuccess && last > 0) e = hipMemcpyAsync(heads.data(), t->d0_dev, (size_t)last, hipMemcpyDeviceToHost, t->stream);
        if (e != hipSuccess) rc = fail(t->err, DBAZ_EDEVICE, "dbaz_replay_exact_targets: %s", hipGetErrorString(e));
    }
    e = hipStreamSynchronize(t->stream); // also on a failure above: the rows are final, or the call says why not
    if (rc == DBAZ_OK && e != hipSuccess) rc = fail(t->err, DBAZ_EDEVICE, "dbaz_replay_exact_targets failed: %s", hipGetErrorString(e));
    if (rc != DBAZ_OK) {
        (void)hipGetLastError();
        return rc;
    }
    // the call's timeline: marks 0 1 2 bound scan and group, the host plans the chunks between marks 2 and 3, then three intervals per chunk
    float ms[REPLAY_PHASES] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (size_t i = 0; i + 1 < mark; i++) {
        float d = 0.0f;
        if (i == 2 || hipEventElapsedTime(&d, rs.marks[i], rs.marks[i + 1]) != hipSuccess) continue;
        ms[i < 2 ? i : 2 + (i - 3) % 3] += d;
    }
    (void)hipGetLastError();
    if (last > 0) { // the last chunk's tables: a solved pool like any other
        t->n_free.assign(ch.n_free.begin() + ch.chunk_first[n_chunks - 1], ch.n_free.end());
        t->d0.assign(heads.begin(), heads.end());
        t->solve_ms = ms[3];
        t->n_solved = last;
    }
    if (stats_host) {
        stats_host[0] = n;
        stats_host[1] = n_games;
        stats_host[2] = n_roots;
        stats_host[3] = n_chunks;
        for (int i = 0; i < 4; i++) stats_host[4 + i] = (int64_t)got[i];
        for (int f = 0; f <= SOLVER_MAX_E; f++) stats_host[REPLAY_STATS + f] = (int64_t)got[4 + f];
        for (int i = 0; i < REPLAY_PHASES; i++) stats_host[REPLAY_STATS + SOLVER_MAX_E + 1 + i] = (int64_t)((double)ms[i] * 1e6);
    }
    return DBAZ_OK;
}

// ---- dbaz_deep_*: the pool of one
extern "C" const char *dbaz_deep_last_error(const dbaz_deep *d) { return d ? d->err.c_str() : g_deep_error.c_str(); }

extern "C" void dbaz_deep_destroy(dbaz_deep *d)
{
    if (!d) return;
    tables_release(d);
    delete d;
}

extern "C" int dbaz_deep_create(int32_t rows, int32_t cols, int32_t device, int32_t max_free, dbaz_deep **out)
{
    return tables_create(out, g_deep_error, "dbaz_deep", rows, cols, device, max_free, 1);
}

extern "C" int dbaz_deep_solve(dbaz_deep *d, const int16_t *root_row_host, int32_t low_bits)
{
    return d ? tables_solve(d, 1, root_row_host, low_bits) : DBAZ_EINVAL;
}

extern "C" int dbaz_deep_info(const dbaz_deep *d, int32_t *n_free, int64_t *table_bytes, double *solve_ms, int32_t *d0)
{
    if (!d) return DBAZ_EINVAL;
    if (n_free) *n_free = d->n_solved ? d->n_free[0] : -1;
    if (table_bytes) *table_bytes = (int64_t)1 << d->max_free;
    if (solve_ms) *solve_ms = d->solve_ms;
    if (d0) *d0 = d->n_solved ? d->d0[0] : -128;
    return DBAZ_OK;
}

extern "C" int dbaz_deep_table(dbaz_deep *d, int8_t *host_dst, int64_t first, int64_t count)
{
    return d ? tables_table(d, 0, host_dst, first, count) : DBAZ_EINVAL;
}

extern "C" int dbaz_deep_score(dbaz_deep *d, int32_t n, const int16_t *x_dev, const float *pi_dev, int8_t *value_dev, int8_t *diff_dev, int8_t *q_dev,
                               float *mass_dev, int16_t *n_free_dev, uint8_t *served_dev, void *stream)
{
    return d ? tables_score(d, true, n, x_dev, pi_dev, nullptr, value_dev, diff_dev, q_dev, mass_dev, n_free_dev, served_dev, stream) : DBAZ_EINVAL;
}

extern "C" int dbaz_deep_policy(dbaz_deep *d, int32_t n, const int16_t *x_dev, uint64_t pick_seed, float *p_dev, float *v_dev, uint8_t *served_dev,
                                void *stream)
{
    if (!d) return DBAZ_EINVAL;
    if (d->n_solved == 0) return fail(d->err, DBAZ_ESTATE, "dbaz_deep_policy before a successful dbaz_deep_solve");
    if (n < 0 || (n > 0 && (!x_dev || !p_dev || !v_dev || !served_dev))) return fail(d->err, DBAZ_EINVAL, "dbaz_deep_policy: bad argument (n = %d)", n);
    if (n == 0) return DBAZ_OK;
    CHECK_HIP(d->err, hipSetDevice(d->dev));
    k_deep_policy<<<deep_blocks(n), 64 * DEEP_WAVES, 0, (hipStream_t)stream>>>(d->board, d->roots_dev, d->T, x_dev, n, pick_seed, p_dev, v_dev, served_dev);
    CHECK_HIP(d->err, hipGetLastError());
    CHECK_HIP(d->err, hipEventRecord(d->used, (hipStream_t)stream));
    return DBAZ_OK;
}

// ====================================================================================
// Deep tables inside the search (dbaz_attach_tables): one table per engine slot, solved from requests that exist
// only on the device
// ====================================================================================
// A pass is k_slot_requests and then S launches of k_slot_solve on one stream (slot_tables_plan.h); stream order is the only
// synchronisation between them.  The pass's roots go on a device list with one atomic each, and the counter of the NEXT pass is
// zeroed by this one (two counters, used in turn), so the host neither resets nor reads anything.
// The pooled form (dbaz_attach_tables_pool, table_pool.h) puts k_pool_decide and k_pool_grant in front: the slots share n_tables
// regions, given back and granted on the device; the per-slot form launches neither.
static_assert(sizeof(SlotTablesPlan().widest) == sizeof(SlotTables().widest), "solver.h restates slot_tables_plan.h");

// what k_slot_solve needs to know about roots of one F
struct SlotDepthDev {
    int32_t L, top, plain, pad;
    const uint32_t *hi;   // the high patterns of F - L bits in ascending popcount order
    const uint16_t *low;  // the low masks of L bits, likewise
    const uint32_t *loff; // [L + 2] layers of `low`
    uint32_t hoff[SOLVER_MAX_HIGH + 2]; // layers of `hi`
};

// solver_move_q's mask of box (bl, bc) for its edge `a`: the box's other edges that are free, over the compact edges
static __device__ __forceinline__ uint32_t slot_box_other(const TablesBoard &B, const uint64_t (&fe)[4], int bl, int bc, int a)
{
    const int W = B.cols + 1, at = bl * W + bc;
    const int ed[4] = {at, at + W, B.HW + at, B.HW + at + 1};
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (ed[i] != a && ((word_of(fe, ed[i] >> 6) >> (ed[i] & 63)) & 1ull)) o |= 1u << edge_rank(fe, ed[i]);
    return o;
}

// Step 1 of a pass, one wavefront per slot with a request (a slot without one costs one word read): slot_request_rule
// (endgame.h) keeps or drops the table, or the slot gets a new header -- F0, the free-edge set, act and `other` as
// position_geometry builds them, the real edges and box neighbours from the board alone -- and its BatchGeo goes on the pass's list.  Lane l looks at action slots l, 64 + l, ...; a free one writes its compact edge's entries.
// POOLED (dbaz_attach_tables_pool): k_pool_decide and k_pool_grant have run, so every request still standing is a solve, into the
// region the header names; a slot whose header names none was denied, and its header stays invalid.  wait_mode
// (dbaz_attach_tables_pool_wait): such a slot waits instead -- its request stays standing for the next pass and its header says
// ENDGAME_WAITING, so that the search leaves it alone; the pass that solves a slot's table leaves its step there (endgame.h).
#define SLOT_REQ_WAVES 4
template <bool POOLED>
__global__ void __launch_bounds__(64 * SLOT_REQ_WAVES) k_slot_requests(TablesBoard B, int max_free, EndgameReq *__restrict__ req,
                                                                       EndgameSlotHdr *__restrict__ hdr, int n_slots, BatchGeo *__restrict__ geo,
                                                                       uint32_t *__restrict__ count, uint32_t *__restrict__ count_next,
                                                                       unsigned long long *__restrict__ stats, int wait_mode, int step)
{
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) *count_next = 0u; // nobody reads it before the next pass
    const int W = B.cols + 1;
    for (int slot = blockIdx.x * SLOT_REQ_WAVES + (threadIdx.x >> 6); slot < n_slots; slot += gridDim.x * SLOT_REQ_WAVES) {
        EndgameReq *rq = req + slot;
        EndgameSlotHdr *h = hdr + slot;
        if (!*(volatile const int32_t *)&rq->want) continue; // the same answer in every lane: nobody has written yet
        uint64_t fe[4];
#pragma unroll
        for (int w = 0; w < 4; w++) fe[w] = rq->free_edges[w] & __ballot(board_real_edge(B, w * 64 + lane));
        const int64_t game = rq->game;
        const int model = rq->model;
        const SlotDecision d = slot_request_rule(fe, h->valid, h->game, h->free_edges, game, max_free);
        const int F = d.F;
        const int table = POOLED ? h->table : slot;
        const bool waits = POOLED && wait_mode && d.solve && table < 0; // the pool is dry: the request stands
        if (lane == 0) {
            if (!waits) rq->want = 0;
            h->model = model;
            if (!d.keep && !d.solve) h->valid = 0;
            if (waits) h->wait = ENDGAME_WAITING;
        }
        if (!d.solve) continue;
        if (POOLED && table < 0) continue; // denied: the leaves of this search go to the model's own evaluator (or the slot waits)

        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(count, 1u);
        at = (uint32_t)__shfl((int)at, 0);
        if (at >= (uint32_t)n_slots) continue; // one request per slot: cannot happen
        BatchGeo *bg = geo + at;
        if (lane >= F && lane < SOLVER_MAX_E) { // the entries no edge owns, as position_geometry leaves them
            bg->other[lane][0] = bg->other[lane][1] = SOLVER_NO_BOX;
            h->other[lane][0] = h->other[lane][1] = SOLVER_NO_BOX;
            h->act[lane] = 0;
        }
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int a = w * 64 + lane;
            if (!((fe[w] >> lane) & 1ull)) continue;
            const int j = edge_rank(fe, a);
            uint32_t o[2] = {SOLVER_NO_BOX, SOLVER_NO_BOX};
            int used = 0;
            if (a < B.HW) { // a horizontal edge: the boxes above and below, in the order of the board's box scan
                const int l = a / W, c = a % W;
                if (l >= 1) o[used++] = slot_box_other(B, fe, l - 1, c, a);
                if (l < B.rows) o[used++] = slot_box_other(B, fe, l, c, a);
            } else { // a vertical edge: the boxes to its left and right
                const int l = (a - B.HW) / W, c = (a - B.HW) % W;
                if (c >= 1) o[used++] = slot_box_other(B, fe, l, c - 1, a);
                if (c < B.cols) o[used++] = slot_box_other(B, fe, l, c, a);
            }
            bg->other[j][0] = h->other[j][0] = o[0];
            bg->other[j][1] = h->other[j][1] = o[1];
            h->act[j] = (uint8_t)a;
        }
        if (lane == 0) {
            bg->F = F;
            bg->slot = table;
            for (int w = 0; w < 4; w++) h->free_edges[w] = fe[w];
            h->game = game;
            h->F0 = F;
            if (!POOLED) h->table = table;
            if (POOLED && wait_mode) h->wait = step; // k_select of this very step leaves the slot alone (0: no step runs next to this pass)
            h->valid = 1; // the table is complete before anything later on this stream reads it
            atomicAdd(stats, 1ull);
        }
    }
}

// ---- the pooled form (table_pool.h): two light kernels in front of k_slot_requests ----
// k_pool_decide, one wavefront per slot with a request: slot_request_rule as above.  A keep is finished here; a drop and a release
// request (EndgameReq::want == 2, left by the driver when the slot's game ended) invalidate the header and push the slot's region
// back on the free stack -- the position comes from one atomic, so the stack's order is not reproducible, which changes no
// result; a solve stays standing for k_slot_requests, and ask[slot] says whether the slot needs a region for it.  In wait mode the
// request of a waiting slot is still standing and is decided again like a new one; a release or a drop ends its wait.
__global__ void __launch_bounds__(64 * SLOT_REQ_WAVES) k_pool_decide(TablesBoard B, int max_free, EndgameReq *__restrict__ req,
                                                                     EndgameSlotHdr *__restrict__ hdr, int n_slots, TablePoolState *__restrict__ pool,
                                                                     int32_t *__restrict__ stack, uint8_t *__restrict__ ask)
{
    const int lane = threadIdx.x & 63;
    const int n_tables = pool->n_tables; // never written after the attach
    for (int slot = blockIdx.x * SLOT_REQ_WAVES + (threadIdx.x >> 6); slot < n_slots; slot += gridDim.x * SLOT_REQ_WAVES) {
        EndgameReq *rq = req + slot;
        EndgameSlotHdr *h = hdr + slot;
        const int want = *(volatile const int32_t *)&rq->want; // the same answer in every lane: nobody has written yet
        if (!want) {
            if (lane == 0) ask[slot] = 0;
            continue;
        }
        uint64_t fe[4];
#pragma unroll
        for (int w = 0; w < 4; w++) fe[w] = rq->free_edges[w] & __ballot(board_real_edge(B, w * 64 + lane));
        const int held = h->table;
        SlotDecision d = slot_request_rule(fe, h->valid, h->game, h->free_edges, rq->game, max_free);
        if (want == 2) d.keep = d.solve = false; // the game is over, whichever it was: no later search of this slot is served by it
        const int model = rq->model;
        if (lane == 0) {
            ask[slot] = d.solve && held < 0 ? 1 : 0;
            if (!d.solve) rq->want = 0;
            if (d.keep) h->model = model;
            if (!d.keep && !d.solve) {
                h->valid = 0;
                h->table = -1;
                if (pool->wait_mode) h->wait = 0;
                if ((unsigned)held < (unsigned)n_tables) {
                    const int at = atomicAdd(&pool->top, 1);
                    if ((unsigned)at < (unsigned)n_tables) stack[at] = held; // every region is held or on the stack, never both
                }
            }
        }
    }
}

// k_pool_grant, ONE workgroup: the asking slots in ascending slot order, TABLE_POOL_GROUP of them per round, take the free regions
// from the top of the stack (table_pool_grant) as long as they last; then the pool's figures are settled.
__global__ void __launch_bounds__(TABLE_POOL_GROUP) k_pool_grant(EndgameSlotHdr *__restrict__ hdr, int n_slots, TablePoolState *__restrict__ pool,
                                                                 const int32_t *__restrict__ stack, const uint8_t *__restrict__ ask)
{
    __shared__ int s_wave[TABLE_POOL_GROUP / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n_tables = pool->n_tables;
    const int n_free = min(max(pool->top, 0), n_tables);
    long long base = 0; // asking slots of the rounds before
    for (int g0 = 0; g0 < n_slots; g0 += TABLE_POOL_GROUP) {
        const int slot = g0 + t;
        const bool asks = slot < n_slots && ask[slot] != 0;
        const unsigned long long b = __ballot(asks);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < TABLE_POOL_GROUP / 64; w++) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (asks) {
            const int pos = table_pool_grant(n_free, base + before + __popcll(b & ((1ull << lane) - 1ull)));
            if (pos >= 0) hdr[slot].table = stack[pos];
        }
        base += total;
        __syncthreads(); // s_wave is written again
    }
    if (t == 0) {
        TablePoolState s = *pool;
        s.top = n_free;
        table_pool_settle(s, base);
        *pool = s;
    }
}

// a clear-all point: every region free, no header names one (the headers have just been zeroed on this stream)
__global__ void __launch_bounds__(256) k_pool_reset(EndgameSlotHdr *__restrict__ hdr, int n_slots, TablePoolState *__restrict__ pool,
                                                    int32_t *__restrict__ stack, int n_tables)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_slots) hdr[i].table = -1;
    if (i < n_tables) stack[i] = table_pool_initial(n_tables, i);
    if (i == 0) {
        pool->top = n_tables;
        pool->waiting = 0; // the zeroed headers and requests: nobody waits
    }
}

// Launch s of a pass: for every listed root its own layer k = top(F) - s (k < 0: the root is finished).  The fixed grid strides
// over (root, work item) pairs, `width` items per root -- the widest layer any F <= max_free has in this launch; an item the
// root's layer does not have is skipped.  Every condition in the loop is the same for the whole workgroup.
__global__ void __launch_bounds__(SOLVER_THREADS) k_slot_solve(const BatchGeo *__restrict__ geo, const uint32_t *__restrict__ count, int n_slots,
                                                               int n_tables, int8_t *T, int stride_bits, const SlotDepthDev *__restrict__ depth, int max_free,
                                                               int s, uint32_t width)
{
    const uint32_t n = min(*count, (uint32_t)n_slots);
    const uint64_t total = (uint64_t)n * width;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const BatchGeo &g = geo[w / width];
        const uint32_t item = (uint32_t)(w % width);
        if ((unsigned)g.F > (unsigned)max_free || (unsigned)g.slot >= (unsigned)n_tables) continue; // never outside the regions
        const SlotDepthDev &d = depth[g.F];
        const int k = d.top - s;
        if (k < 0) continue;
        int8_t *D = T + ((size_t)g.slot << stride_bits);
        if (d.plain) { // 2^F <= 8 masks: one work item, no LDS
            if (item == 0) solver_layer_body(g.other, g.F, D, k, threadIdx.x);
            continue;
        }
        const uint32_t first = d.hoff[k];
        if (item >= d.hoff[k + 1] - first) continue;
        solver_subcube_body(g.other, g.F, D, d.L, d.hi[first + item], d.low, d.loff);
        __syncthreads(); // the next item of this workgroup reuses the LDS subcube
    }
}

bool tables_serves(const dbaz_tables *t, int rows, int cols, int device, int *max_free)
{
    *max_free = t->max_free;
    return t->board.rows == rows && t->board.cols == cols && t->dev == device;
}

int slot_tables_setup(dbaz_tables *t, int n_slots, int n_tables, SlotTables *st, void *allocs[6], bool wait)
{
    SlotTablesPlan plan;
    if (slot_tables_plan(t->max_free, plan) != 0) return fail(t->err, DBAZ_EINVAL, "slot tables: max_free %d is outside 0 .. %d", t->max_free, SOLVER_MAX_E);
    CHECK_HIP(t->err, hipSetDevice(t->dev));
    // The work lists of every (F, L) with F <= max_free in ONE buffer that the caller owns -- not the lists cached on t, which go
    // away with t while the engine may search on under another handle: all 32-bit lists (the high patterns per F, the layer
    // offsets of the low masks per L) first, then the 16-bit low masks per L.
    std::vector<uint32_t> words;
    std::vector<uint16_t> halves;
    size_t hi_at[SOLVER_MAX_E + 1] = {0}, loff_at[SOLVER_MAX_LOW + 1] = {0}, low_at[SOLVER_MAX_LOW + 1] = {0};
    bool have_low[SOLVER_MAX_LOW + 1] = {false};
    SlotDepthDev depth[SOLVER_MAX_E + 1];
    for (int F = 0; F <= SOLVER_MAX_E; F++) {
        SlotDepthDev &d = depth[F];
        d = SlotDepthDev();
        d.plain = 1;
        if (F > t->max_free) continue;
        d.L = plan.depth[F].L;
        d.top = plan.depth[F].top;
        d.plain = plan.depth[F].plain ? 1 : 0;
        if (d.plain) continue;
        std::vector<uint32_t> hperm, hoff;
        popcount_order(F - d.L, hperm, hoff);
        std::copy(hoff.begin(), hoff.end(), d.hoff);
        hi_at[F] = words.size();
        words.insert(words.end(), hperm.begin(), hperm.end());
        if (!have_low[d.L]) {
            std::vector<uint32_t> lperm, loff;
            popcount_order(d.L, lperm, loff);
            have_low[d.L] = true;
            loff_at[d.L] = words.size();
            words.insert(words.end(), loff.begin(), loff.end());
            low_at[d.L] = halves.size();
            halves.insert(halves.end(), lperm.begin(), lperm.end());
        }
    }
    const size_t word_bytes = (words.size() * 4 + 15) / 16 * 16;
    // the pooled form besides: the pool's figures with the free stack behind them, and the asking flags of a pass
    void *p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const char *what[6] = {"the per-depth table", "the root list", "the counters", "the work lists", "the pool's free stack", "the asking flags"};
    const size_t bytes[6] = {sizeof depth, std::max<size_t>(1, (size_t)n_slots) * sizeof(BatchGeo), 2 * sizeof(uint32_t),
                             std::max<size_t>(16, word_bytes + halves.size() * 2), sizeof(TablePoolState) + (size_t)n_tables * sizeof(int32_t),
                             std::max<size_t>(16, (size_t)n_slots)};
    const int n_bufs = n_tables > 0 ? 6 : 4;
    hipError_t e = hipSuccess;
    int failed = 0;
    for (int i = 0; i < n_bufs && e == hipSuccess; i++) {
        failed = i;
        e = hipMalloc(&p[i], bytes[i]);
        if (e != hipSuccess) p[i] = nullptr;
        else if (i == 1 || i == 2 || i >= 4) e = hipMemset(p[i], 0, bytes[i]);
    }
    if (e == hipSuccess && n_tables > 0) { // all free; the headers get their -1 from slot_tables_pool_reset
        failed = 4;
        TablePoolState ps = TablePoolState();
        ps.n_tables = ps.top = n_tables;
        ps.wait_mode = wait ? 1 : 0;
        std::vector<int32_t> stack((size_t)n_tables);
        for (int i = 0; i < n_tables; i++) stack[(size_t)i] = table_pool_initial(n_tables, i);
        e = hipMemcpy(p[4], &ps, sizeof ps, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy((char *)p[4] + sizeof ps, stack.data(), stack.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        failed = 3;
        if (!words.empty()) e = hipMemcpy(p[3], words.data(), words.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess && !halves.empty()) e = hipMemcpy((char *)p[3] + word_bytes, halves.data(), halves.size() * 2, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        for (int F = 0; F <= t->max_free; F++) {
            SlotDepthDev &d = depth[F];
            if (d.plain) continue;
            d.hi = (const uint32_t *)p[3] + hi_at[F];
            d.loff = (const uint32_t *)p[3] + loff_at[d.L];
            d.low = (const uint16_t *)((const char *)p[3] + word_bytes) + low_at[d.L];
        }
        failed = 0;
        e = hipMemcpy(p[0], depth, sizeof depth, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { // (the dynamic LDS of k_slot_solve is 2^14 bytes at the most: default_low_bits never goes higher)
        for (void *q : p)
            if (q) (void)hipFree(q);
        (void)hipGetLastError();
        return fail(t->err, DBAZ_EDEVICE, "slot tables of %d slots: %s (%zu bytes): %s", n_slots, what[failed], bytes[failed], hipGetErrorString(e));
    }
    *st = SlotTables();
    st->rows = t->board.rows; st->cols = t->board.cols; st->max_free = t->max_free;
    st->n_launches = plan.n_launches;
    st->lds_bytes = plan.lds_bytes;
    std::copy(plan.widest, plan.widest + SOLVER_MAX_E + 1, st->widest);
    st->depth_dev = p[0];
    st->geo_dev = p[1];
    st->count_dev = (uint32_t *)p[2];
    st->pass = 0;
    st->n_tables = n_tables;
    st->pool_dev = p[4];
    st->ask_dev = (uint8_t *)p[5];
    st->wait_mode = n_tables > 0 && wait ? 1 : 0;
    for (int i = 0; i < 6; i++) allocs[i] = p[i];
    return DBAZ_OK;
}

void slot_tables_pass(SlotTables *st, hipStream_t stream, EndgameReq *req, EndgameSlotHdr *hdr, int8_t *tables, int n_slots,
                      unsigned long long *stats, int step)
{
    const TablesBoard B = tables_board(st->rows, st->cols);
    uint32_t *count = st->count_dev + (st->pass & 1u), *count_next = st->count_dev + ((st->pass + 1u) & 1u);
    st->pass++;
    const int blocks = std::min((n_slots + SLOT_REQ_WAVES - 1) / SLOT_REQ_WAVES, 1024);
    const int n_regions = st->n_tables > 0 ? st->n_tables : n_slots;
    if (st->n_tables > 0) { // releases, then grants in slot order, then the headers of the slots that hold a region
        TablePoolState *pool = (TablePoolState *)st->pool_dev;
        int32_t *stack = (int32_t *)(pool + 1);
        k_pool_decide<<<blocks, 64 * SLOT_REQ_WAVES, 0, stream>>>(B, st->max_free, req, hdr, n_slots, pool, stack, st->ask_dev);
        k_pool_grant<<<1, TABLE_POOL_GROUP, 0, stream>>>(hdr, n_slots, pool, stack, st->ask_dev);
        k_slot_requests<true><<<blocks, 64 * SLOT_REQ_WAVES, 0, stream>>>(B, st->max_free, req, hdr, n_slots, (BatchGeo *)st->geo_dev, count, count_next,
                                                                          stats, st->wait_mode, step);
    } else {
        k_slot_requests<false><<<blocks, 64 * SLOT_REQ_WAVES, 0, stream>>>(B, st->max_free, req, hdr, n_slots, (BatchGeo *)st->geo_dev, count, count_next,
                                                                           stats, 0, 0);
    }
    for (int s = 0; s < st->n_launches; s++) {
        // never more workgroups than (root, item) pairs the launch can have
        const unsigned grid = (unsigned)std::min<uint64_t>(SLOT_TABLES_GRID, (uint64_t)std::max(std::min(n_slots, n_regions), 1) * st->widest[s]);
        k_slot_solve<<<grid, SOLVER_THREADS, st->lds_bytes, stream>>>((const BatchGeo *)st->geo_dev, count, n_slots, n_regions, tables, st->max_free,
                                                                  (const SlotDepthDev *)st->depth_dev, st->max_free, s, st->widest[s]);
    }
}

void slot_tables_pool_reset(SlotTables *st, hipStream_t stream, EndgameSlotHdr *hdr, int n_slots)
{
    if (st->n_tables <= 0) return;
    TablePoolState *pool = (TablePoolState *)st->pool_dev;
    k_pool_reset<<<(std::max(n_slots, st->n_tables) + 255) / 256, 256, 0, stream>>>(hdr, n_slots, pool, (int32_t *)(pool + 1), st->n_tables);
}

hipError_t slot_tables_pool_read(const SlotTables *st, int32_t *in_use, int32_t *high_water, int64_t *denied, int32_t *waiting, int64_t *waited)
{
    TablePoolState ps = TablePoolState();
    hipError_t e = st->n_tables > 0 ? hipMemcpy(&ps, st->pool_dev, sizeof ps, hipMemcpyDeviceToHost) : hipSuccess;
    *in_use = ps.n_tables - ps.top;
    *high_water = ps.high_water;
    *denied = ps.denied;
    if (waiting) *waiting = ps.waiting;
    if (waited) *waited = ps.waited;
    return e;
}
