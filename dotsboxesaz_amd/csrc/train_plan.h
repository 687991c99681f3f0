// train_plan.h -- the host arithmetic that decides the launches of the training step (plain C++, no HIP types).
//
// train_plan_build fixes, for one board, the samples per workgroup of the conv kernel (S) and per chunk of k_wgrad_h3 (Swh), both
// LDS sizes, and refuses the boards the kernels cannot hold BEFORE anything is allocated or launched; the small functions below
// give every grid, chunk count and split-K step the two units launch with.  train.hip and train_net.hip use all of it unchanged;
// the CPU test tests/test_train_plan.py compiles this header with g++ and compares it, field by field over every accepted
// board, with the restatement the GPU tests compute their batch sizes from (oracle/train_plan.py).
#pragma once

#include <stddef.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define TRAIN_PLAN_HD __host__ __device__ inline
#else
#define TRAIN_PLAN_HD inline
#endif

#define TT 512          // threads per workgroup of the conv / wgrad kernels: 8 waves, two per SIMD
#define TC 64           // channels (the two-cout-tile MFMA tiling is written for 64)
#define TL_MAX 64       // conv layers of a tower (2 * blocks)
#define RED_BLOCKS 256  // workgroups of the column-sum kernels

#define WG_MAXLD 13 // k_wgrad_h3: float4 per thread and chunk: 2 images x <= 208 rows x 16 quads / 512 threads
#define WH_SB 288   // k_wgrad_h3: bytes per image row

#define NET_WG 256   // threads per workgroup of train_net.hip's kernels
#define NET_HB 1024  // workgroups of the head row kernels
#define NET_OB 256   // workgroups of k_head_out_bwd
#define NET_SB 2048  // workgroups of k_stem_conv
#define STEM_S 4     // samples a k_stem_conv workgroup normalizes at a time
#define FC_SPLITS 16   // fc weight gradient: K = batch
#define FCF_SPLITS 4   // fc forward: K = 32 HW
#define HW_SPLITS 392  // head-conv weight gradient: K = batch * HW
#define STEM_SPLITS 392 // stem weight gradient: K = batch * HW

constexpr int TRAIN_MAX_POSITIONS = 196;                      // (rows + 1) * (cols + 1) of the largest board: one sample fills k_conv_t's 256 rows
constexpr int TRAIN_CONV_ROWS = 256;                          // rows of a k_conv_t workgroup
constexpr int TRAIN_WH_ROWS = WG_MAXLD * TT / 32;             // 208: rows per k_wgrad_h3 chunk the prefetch registers hold
constexpr size_t TRAIN_WH_LDS_BUDGET = (size_t)150 * 1024;    // k_wgrad_h3: samples are added to a chunk up to here
constexpr size_t TRAIN_LDS_LIMIT = (size_t)160 * 1024;        // what a workgroup can have at all

struct WhGeo { int RK, RA, PW, G, NK; };
TRAIN_PLAN_HD WhGeo wh_geo(int Sw, int H, int W)
{
    WhGeo g;
    g.PW = W + 1;
    g.G = g.PW + 1;
    g.NK = (Sw * H * g.PW + 31) / 32;              // K steps per chunk
    g.RK = g.NK * 32;                              // rows of the dY image
    g.RA = 2 * g.G + Sw * (H + 1) * g.PW;          // rows of the padded A image (the last window ends at row Sw*(H+1)*PW + G)
    return g;
}
static inline size_t wh_lds_bytes(int Sw, int H, int W)
{
    const WhGeo g = wh_geo(Sw, H, W);
    return (size_t)(g.RA + g.RK) * WH_SB + (size_t)g.RK * 4 + (size_t)Sw * H * W * 4;
}

struct TrainPlan {
    int H = 0, W = 0, HW = 0;
    int S = 1;                  // samples per k_conv_t workgroup
    int Swh = 1;                // samples per k_wgrad_h3 chunk
    int pwc = 0;                // the k_wgrad_h3 instantiation: 8 = <8> (W + 1 = 8 at compile time), 0 = <0> (any board)
    size_t conv_lds = 0, wgrad_h3_lds = 0;
};

// The plan of a rows x cols board.  Returns true, or false with the reason in `why`: nothing of a refused board is allocated or launched.
static inline bool train_plan_build(int rows, int cols, TrainPlan &p, char *why, size_t why_len)
{
    p = TrainPlan();
    if (rows < 1 || cols < 1 || ((long long)rows + 1) * ((long long)cols + 1) > TRAIN_MAX_POSITIONS) {
        snprintf(why, why_len, "board %dx%d unsupported: the training tower holds boards of at most %d positions ((rows + 1) * (cols + 1))", rows,
                 cols, TRAIN_MAX_POSITIONS);
        return false;
    }
    p.H = rows + 1; p.W = cols + 1; p.HW = p.H * p.W;
    // long thin boards: the padded A image of k_wgrad_h3 has 2 (W + 2) guard rows and a pad column per line
    const size_t need = wh_lds_bytes(1, p.H, p.W);
    if (need > TRAIN_LDS_LIMIT) {
        snprintf(why, why_len, "board %dx%d unsupported: the weight-gradient kernel needs %zu bytes of LDS for one sample, a workgroup has %zu", rows,
                 cols, need, TRAIN_LDS_LIMIT);
        return false;
    }
    p.S = TRAIN_CONV_ROWS / p.HW;
    const int S4 = (TC + 8) / 4;
    const int zu = (p.S * p.HW * S4 + 15) & ~15;
    p.conv_lds = (size_t)(zu + 3 * S4) * 16 + (size_t)(TT / 64) * 2 * TC * 8 + 16; // image + zero rows + the epilogue's column-sum slots
    // samples per k_wgrad_h3 chunk: as many as the prefetch registers (208 rows) and 150 KB of LDS hold
    p.Swh = 1;
    while ((p.Swh + 1) * p.HW <= TRAIN_WH_ROWS && wh_lds_bytes(p.Swh + 1, p.H, p.W) <= TRAIN_WH_LDS_BUDGET) p.Swh++;
    p.wgrad_h3_lds = wh_lds_bytes(p.Swh, p.H, p.W);
    p.pwc = p.W == 7 ? 8 : 0;
    return true;
}

// ---- the tower (train.hip)
static inline int train_conv_grid(const TrainPlan &p, int n) { return (n + p.S - 1) / p.S; }          // k_conv_t: one workgroup per S samples
static inline int train_wgrad_chunks(const TrainPlan &p, int n) { return (n + p.Swh - 1) / p.Swh; }   // k_wgrad_h3: chunks of Swh samples ...
static inline int train_wgrad_grid(const TrainPlan &p, int cus, int n)                                // ... walked by at most one workgroup per CU
{
    const int nchunks = train_wgrad_chunks(p, n);
    return cus < nchunks ? cus : nchunks;
}
// workgroups of the column-sum kernels over M rows (32 rows per pass of a workgroup)
static inline int red_blocks(long long M)
{
    const long long b = (M + 31) / 32;
    return (int)(b < 1 ? 1 : b > RED_BLOCKS ? RED_BLOCKS : b);
}
// k_bn_apply: workgroups of 256 threads x 4 quads per pass; as few passes as 1 024 workgroups allow, and a grid that
// divides the tensor into WHOLE passes (1 024 workgroups left 3.06 passes at batch 4 096: a fourth latency round for 6 % of the rows)
static inline int bn_apply_passes(long long n4)
{
    const long long per = 256 * 4;
    const long long passes = (n4 + 1024 * per - 1) / (1024 * per);
    return (int)(passes < 1 ? 1 : passes);
}
static inline int bn_apply_grid(long long n4)
{
    const long long per = 256 * 4, passes = bn_apply_passes(n4);
    const long long g = (n4 + per * passes - 1) / (per * passes);
    return (int)(g < 1 ? 1 : g);
}

// ---- stem and heads (train_net.hip)
// k_gemm_f32 split over K: every z slice takes kchunk (a multiple of 32) K values in steps of 32
static inline int gemm_kchunk(int K, int splits) { return ((K + splits - 1) / splits + 31) / 32 * 32; }
static inline int gemm_splits(int K, int splits) // the z extent launch_gemm uses
{
    const int kchunk = gemm_kchunk(K, splits);
    return (K + kchunk - 1) / kchunk;
}
static inline int net_min(long long a, long long b) { return (int)(a < b ? a : b); }
static inline int net_stem_grid(int n) { return net_min(NET_SB, (n + STEM_S - 1) / STEM_S); }                   // k_stem_conv
static inline int net_head_conv_grid(long long M) { return net_min(NET_HB, (M + 127) / 128); }                  // k_head_conv
static inline int net_head_bn_apply_grid(long long M) { return net_min(1024, (M * 8 + NET_WG - 1) / NET_WG); }  // k_head_bn_apply
static inline int net_head_out_grid(int n) { return net_min(1024, (n + 3) / 4); }                               // k_head_out
static inline int net_head_rows_grid(long long M) { return net_min(NET_HB, (M + 31) / 32); }                    // k_head_bn_bwd_sums / _apply
static inline int net_head_bwd_data_grid(long long M) { return net_min(1024, (M + 31) / 32); }                  // k_head_conv_bwd_data
static inline int net_head_wgrad_splits(long long M) { return net_min(HW_SPLITS, (M + 31) / 32); }              // head-conv weight gradient (K = M)
static inline int net_stem_wgrad_splits(long long M) { return net_min(STEM_SPLITS, (M + 31) / 32); }            // stem weight gradient (K = M)
