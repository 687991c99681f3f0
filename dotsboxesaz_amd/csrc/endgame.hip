// endgame.hip -- exact endgame solver for ANY board the engine supports (A <= 256): a position with F <= 16 free edges is a game
// over the 2^F subsets of those edges, and one workgroup solves it in LDS.  No table in HBM, no solve step, no
// dbaz_engine, no search or network code.
//
// k_endgame_score, one workgroup per feature row x int16 [3*HW] (planes 0, 1: edges; plane 2: the mover's doubled boxes_to_close):
//   1. setup: lane i < E looks at real edge i; the free ones are ranked in ascending action order (ballot + per-wave counts):
//      compact edge j = the j-th free real edge.  Every compact edge gets the "other" masks of solver_move_q over the COMPACT
//      edges: per bordering box the other edges that are still free (0: the edge completes that box whatever else is drawn;
//      SOLVER_NO_BOX: no such box).  The closed boxes are counted from planes 0 / 1.
//   2. solve: D[mask] of solver.hip over the 2^F masks of the compact edges, popcount layers F .. 0, one barrier each; the masks
//      of a layer come from the popcount-sorted list of F bits (built on the host at handle creation), so every lane has a state.
//   3. outputs with dbaz_solver_score's meaning, plus n_free.
#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "endgame.h"

struct dbaz_endgame {
    EndgameGeo g;
    int dev = 0;
    void *bufs[4] = {nullptr, nullptr, nullptr, nullptr}; // action, nbr, perm, off
    std::string err;
};

static thread_local std::string g_endgame_error; // message of a failed dbaz_endgame_create; per thread

static int gerr(dbaz_endgame *g, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    (g ? g->err : g_endgame_error) = buf;
    return code;
}

#define ENDGAME_HIP(g, call)                                                                                        \
    do {                                                                                                            \
        hipError_t _err = (call);                                                                                   \
        if (_err != hipSuccess) return gerr(g, DBAZ_EDEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_err), __FILE__, __LINE__); \
    } while (0)

// ------------------------------------------------------------------------------------
// kernel
// ------------------------------------------------------------------------------------
static __device__ __forceinline__ int sgn(int v) { return (v > 0) - (v < 0); }

__global__ void __launch_bounds__(ENDGAME_THREADS) k_endgame_score(EndgameGeo g, const int16_t *__restrict__ x, const float *__restrict__ pi,
                                                                   int8_t *__restrict__ value, int8_t *__restrict__ diff,
                                                                   int8_t *__restrict__ q, float *__restrict__ mass,
                                                                   int16_t *__restrict__ n_free)
{
    extern __shared__ __attribute__((aligned(16))) int8_t sd[]; // [2^max_free]
    __shared__ int16_t s_cidx[DBAZ_MAX_A];                      // action -> compact edge, -1: drawn or a sentinel slot
    __shared__ uint32_t s_other[ENDGAME_MAX_FREE][2];
    __shared__ uint8_t s_act[ENDGAME_MAX_FREE];                 // compact edge -> action
    __shared__ int s_wave[DBAZ_MAX_A / 64];
    __shared__ int s_closed;

    const int tid = threadIdx.x, lane = tid & 63;
    const size_t r = blockIdx.x;
    const int16_t *xr = x + r * 3 * (size_t)g.HW;

    // 1. the free real edges, ranked
    if (tid < DBAZ_MAX_A) s_cidx[tid] = -1;
    if (tid == 0) s_closed = 0;
    const int a_mine = tid < g.E ? (int)g.action[tid] : 0;
    const bool is_free = tid < g.E && xr[a_mine] == 0;
    const uint64_t bal = __ballot(is_free);
    if (tid < DBAZ_MAX_A && lane == 0) s_wave[tid >> 6] = __popcll(bal);
    __syncthreads();
    int F = 0, before = 0;
    for (int w = 0; w < DBAZ_MAX_A / 64; w++) {
        F += s_wave[w];
        if (w < (tid >> 6)) before += s_wave[w];
    }
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
    const int j = before + __popcll(bal & ((1ull << lane) - 1ull));
    if (is_free) {
        s_cidx[a_mine] = (int16_t)j;
        s_act[j] = (uint8_t)a_mine;
    }
    const int W = g.cols + 1, B = g.rows * g.cols;
    for (int b = tid; b < B; b += ENDGAME_THREADS) {
        const int at = (b / g.cols) * W + b % g.cols;
        if (xr[at] != 0 && xr[at + W] != 0 && xr[g.HW + at] != 0 && xr[g.HW + at + 1] != 0) atomicAdd(&s_closed, 1);
    }
    __syncthreads();
    if (is_free)
        for (int k = 0; k < 2; k++) {
            const int16_t *nb = g.nbr + (tid * 2 + k) * 3;
            uint32_t o = SOLVER_NO_BOX;
            if (nb[0] >= 0) {
                o = 0;
                for (int i = 0; i < 3; i++) {
                    const int c = s_cidx[nb[i]];
                    if (c >= 0) o |= 1u << c;
                }
            }
            s_other[j][k] = o;
        }
    __syncthreads();

    // 2. the subgame, by popcount layers; the box masks are the same for every lane: keep them in scalar registers
    uint32_t o0[ENDGAME_MAX_FREE], o1[ENDGAME_MAX_FREE];
#pragma unroll
    for (int b = 0; b < ENDGAME_MAX_FREE; b++) {
        o0[b] = b < F ? __builtin_amdgcn_readfirstlane(s_other[b][0]) : SOLVER_NO_BOX;
        o1[b] = b < F ? __builtin_amdgcn_readfirstlane(s_other[b][1]) : SOLVER_NO_BOX;
    }
    const uint32_t full = (1u << F) - 1u;
    const uint16_t *list = g.perm + full;
    const uint32_t *off = g.off + F * ENDGAME_OFF_STRIDE;
    for (int k = F; k >= 0; k--) {
        const uint32_t end = off[k + 1];
        for (uint32_t i = off[k] + tid; i < end; i += ENDGAME_THREADS) {
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

    // 3. outputs
    const RowFacts f = solver_facts(B, s_closed, (int)xr[2 * g.HW]);
    const bool open = f.res == DBAZ_RESULT_NONE;
    const int d0 = (int)sd[0];
    const int v = open ? sgn(f.margin + d0) : f.res;
    for (int a = tid; a < g.A; a += ENDGAME_THREADS) {
        const int c = s_cidx[a];
        qr[a] = (int8_t)(open && c >= 0 ? solver_move_q(s_other[c][0], s_other[c][1], 0u, (int)sd[1u << c]) : -128);
    }
    if (tid == 0) {
        value[r] = (int8_t)v;
        diff[r] = (int8_t)d0;
        n_free[r] = (int16_t)F;
        if (mass) {
            float sum = 0.0f;
            for (int c = 0; open && c < F; c++) { // ascending action order
                const int qq = solver_move_q(s_other[c][0], s_other[c][1], 0u, (int)sd[1u << c]);
                if (sgn(f.margin + qq) == v) sum += pi[r * (size_t)g.A + s_act[c]];
            }
            mass[r] = sum;
        }
    }
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
    delete g;
}

extern "C" int dbaz_endgame_create(int32_t rows, int32_t cols, int32_t device, int32_t max_free, dbaz_endgame **out)
{
    if (!out) return gerr(nullptr, DBAZ_EINVAL, "null argument");
    *out = nullptr;
    if (rows < 1 || cols < 1) return gerr(nullptr, DBAZ_EINVAL, "board %dx%d: rows and cols must be >= 1", rows, cols);
    const long long A = 2ll * (rows + 1ll) * (cols + 1ll);
    if (A > DBAZ_MAX_A) return gerr(nullptr, DBAZ_EINVAL, "board %dx%d has %lld action slots: at most %d are supported", rows, cols, A, DBAZ_MAX_A);
    if (max_free < 0 || max_free > ENDGAME_MAX_FREE)
        return gerr(nullptr, DBAZ_EINVAL, "max_free %d: a position's 2^F subgame table lives in LDS, 1 <= max_free <= %d (0 = %d)", max_free,
                    ENDGAME_MAX_FREE, ENDGAME_MAX_FREE);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return gerr(nullptr, DBAZ_EDEVICE, "no HIP device %d (there is no CPU fallback)", device);

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
    if (e != hipSuccess) {
        const std::string msg = hipGetErrorString(e);
        (void)hipGetLastError();
        dbaz_endgame_destroy(g);
        return gerr(nullptr, DBAZ_EDEVICE, "endgame setup failed: %s", msg.c_str());
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
        return gerr(g, DBAZ_EINVAL, "dbaz_endgame_score: bad argument (n = %d)", n);
    if (n == 0) return DBAZ_OK;
    ENDGAME_HIP(g, hipSetDevice(g->dev));
    k_endgame_score<<<(unsigned)n, ENDGAME_THREADS, (size_t)1 << g->g.max_free, (hipStream_t)stream>>>(g->g, x_dev, pi_dev, value_dev, diff_dev, q_dev,
                                                                                                      pi_dev ? mass_dev : nullptr, n_free_dev);
    ENDGAME_HIP(g, hipGetLastError());
    return DBAZ_OK;
}
