// train_reduce.h -- the f64 column-sum reduction and the BatchNorm finish of the training kernels (device code only; included
// by train.hip and train_net.hip).
//
// Partial-row format: a producer workgroup leaves ONE row of f64 column sums per workgroup (colsum_store: [K][4 CQ] per row;
// the NCHW BatchNorm's bn2d_block_store: [K] per (channel, slice)), a *_fin kernel adds the rows of a column up
// (col_wave_sums, block_col_totals).  No float atomics anywhere: the association of every sum is fixed by the code -- rows
// t, t + THREADS, ... per thread in row order, the xor tree 32, 16, .. 1 over a wave's lanes, the wave totals in the order the
// call site states -- and is part of the kernel's contract: results are bit-reproducible.
#pragma once
#include "train.h"

// column sums of a THREADS-thread workgroup whose thread (rl, cq) = (tid / CQ, tid % CQ) holds K x 4 doubles of channel quad cq:
// one partial row [K][4 CQ] per workgroup, row lanes added in order
template <int K, int CQ, int THREADS>
__device__ __forceinline__ void colsum_store(double (&s)[K][4], double *part /*[blocks][K][4 CQ]*/)
{
    constexpr int RL = THREADS / CQ;
    __shared__ double red[RL][K][4 * CQ + 1];
    const int tid = threadIdx.x, cq = tid % CQ, rl = tid / CQ;
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
        for (int e = 0; e < 4; e++) red[rl][k][cq * 4 + e] = s[k][e];
    __syncthreads();
    if (tid < K * 4 * CQ) {
        const int k = tid / (4 * CQ), c = tid - k * 4 * CQ;
        double v = 0.0;
        for (int r = 0; r < RL; r++) v += red[r][k][c];
        part[((size_t)blockIdx.x * K + k) * 4 * CQ + c] = v;
    }
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// THE strided column total: thread t of THREADS adds p[k * kstride + b * stride] for b = t, t + THREADS, ... < n, then the
// wave's 64 lanes are added (every lane gets v[k]).  The K columns travel together: K loads in flight per pass.
template <int K, int THREADS>
__device__ __forceinline__ void col_wave_sums(const double *p, size_t kstride, size_t stride, int n, int t, double (&v)[K])
{
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = 0.0;
    for (int b = t; b < n; b += THREADS)
#pragma unroll
        for (int k = 0; k < K; k++) v[k] += p[k * kstride + (size_t)b * stride];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = wave_sum(v[k]);
}

template <int THREADS> // one column
__device__ __forceinline__ double col_wave_sum(const double *p, size_t stride, int n, int t)
{
    double v[1];
    col_wave_sums<1, THREADS>(p, 0, stride, n, t, v);
    return v[0];
}

// a wave's K sums (in every lane) -> wt[wave][0..K) of the caller's LDS; barrier.  One level, no last-arriver: a __threadfence
// costs ~20 us in the *_fin kernels (it writes back what the previous kernel left dirty in the XCD's L2).
template <int K, int W, int P>
__device__ __forceinline__ void wave_totals_store(const double (&v)[K], double (&wt)[W][P])
{
    static_assert(K <= P, "a wave's row of the LDS array holds its K totals");
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; k++) wt[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
}

// block level: the per-wave totals of K columns in wt[wave][k].  The shared code ends HERE; how the waves are combined is the
// call site's: waves_in_order below, or its own pairwise line.
template <int K, int THREADS, int P>
__device__ __forceinline__ void block_col_totals(const double *p, size_t kstride, size_t stride, int n, double (&wt)[THREADS / 64][P])
{
    double v[K];
    col_wave_sums<K, THREADS>(p, kstride, stride, n, threadIdx.x, v);
    wave_totals_store(v, wt);
}

// the default combine: wave totals added left to right
template <int W, int P>
__device__ __forceinline__ double waves_in_order(const double (&wt)[W][P], int k)
{
    double t = 0.0;
    for (int w = 0; w < W; w++) t += wt[w][k];
    return t;
}

// f32 split-K partials p[b * stride], b < n, of 16 outputs per 256-thread workgroup: thread (oi, j) = (tid & 15, tid >> 4) adds
// the partials b = j, j + 16, ... of its output (p already points at it) in f64, the 16 lanes are added left to right.
// The total is returned to the threads with j == 0.
__device__ __forceinline__ double splitk16_total(const float *p, size_t stride, int n)
{
    __shared__ double red[16][17];
    const int oi = threadIdx.x & 15, j = threadIdx.x >> 4;
    double t = 0.0;
    for (int b = j; b < n; b += 16) t += (double)p[(size_t)b * stride];
    red[j][oi] = t;
    __syncthreads();
    double v = 0.0;
    if (j == 0)
        for (int r = 0; r < 16; r++) v += red[r][oi];
    return v;
}

// ---- the BatchNorm finish (BatchNorm2d in training mode), one thread per channel
// forward: t0 = sum(y), t1 = sum(y^2) over the M elements of the channel -> batch mean and invstd (biased variance, clamped at 0)
// and the running statistics (unbiased variance; M == 1 keeps the biased one).  run_mean_c / run_var_c may be null.
__device__ __forceinline__ void bn_finish_stats(double t0, double t1, long long M, float eps, float momentum, float *mean_c, float *invstd_c,
                                                float *run_mean_c, float *run_var_c)
{
    const double m = t0 / (double)M;
    double var = t1 / (double)M - m * m;
    if (var < 0.0) var = 0.0;
    *mean_c = (float)m;
    *invstd_c = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean_c) *run_mean_c = (float)((1.0 - momentum) * (double)*run_mean_c + (double)momentum * m);
    if (run_var_c) {
        const double unb = M > 1 ? var * (double)M / (double)(M - 1) : var;
        *run_var_c = (float)((1.0 - momentum) * (double)*run_var_c + (double)momentum * unb);
    }
}

// backward: t0 = sum(g), t1 = sum(g * yhat) -> `sums` (f64, read by the apply pass; the caller's layout), dbeta and dgamma
__device__ __forceinline__ void bn_finish_bwd(double t0, double t1, double *sums, int i0, int i1, float *dbeta_c, float *dgamma_c)
{
    sums[i0] = t0;
    sums[i1] = t1;
    *dbeta_c = (float)t0;
    *dgamma_c = (float)t1;
}
