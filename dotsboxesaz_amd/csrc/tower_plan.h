// tower_plan.h -- which kernel body of the inference tower evaluates which samples of a batch (plain C++, no HIP types).
//
// tower_plan_build fixes, for one board and network shape, the samples per workgroup, the tile counts, the LDS sizes, the
// three tail sizes, the choice of the two-cout-tile main body and of the one-launch remainder kernel; tower_split cuts a batch
// of n samples into full rounds of the main launch and a tail (host and device).  nn.hip uses both unchanged; the CPU test
// tests/test_tower_plan.py compiles this header with g++ and compares it, field by field over every accepted board, with the
// restatement the GPU tests name their cases by (oracle/nn_plan.py).
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define TOWER_PLAN_HD __host__ __device__ __attribute__((always_inline))
#else
#define TOWER_PLAN_HD
#endif

#define MAXT 13 // position tiles (16 rows each) per workgroup
#define MAXROWS 256 // rows of the two-cout-tile body
#define MAXS 16 // samples per workgroup: the columns of head_fc_fused's MFMA, the entries of slot_s
#define WRING_UNITS 512 // 16-byte units per weight-ring slot of the two-cout-tile body: 4 cout tiles x (hi, lo) x 64 lanes

constexpr size_t TOWER_WRING_BYTES = (size_t)2 * WRING_UNITS * 16;  // a two-slot weight ring of 16 KB behind the images
constexpr size_t TOWER_LDS_TOTAL = (size_t)160 * 1024;
constexpr size_t TOWER_LDS_BUDGET = (size_t)158 * 1024;             // of 160 KiB: two ping-pong activation images
constexpr size_t TOWER_LDS_BUDGET_C2 = TOWER_LDS_TOTAL - 1536;      // two-cout-tile body: images + ring (1.1 KB of static LDS besides)
// k_tower_rem: slot_s + rowbase_s in each of its four bodies: 4 352 B, what hipcc reports for every k_tower_rem
constexpr size_t TOWER_REM_STATIC_LDS = 4 * (MAXS + MAXROWS) * sizeof(int);
static_assert(16 * MAXT <= MAXROWS, "rowbase_s[MAXROWS] holds the rows of a one-cout-tile workgroup too");

// the MFMA tile wants 16 | C: narrower nets run zero-padded (padded channels stay exactly 0)
static inline int tower_padded_channels(int channels, int precision)
{
    int cp = channels <= 16 ? 16 : channels <= 32 ? 32 : channels <= 64 ? 64 : 128;
    if (precision == 1 && cp < 32) cp = 32; // K = 32 per f16 MFMA step
    return cp;
}

// dynamic LDS of a workgroup of S samples: two ping-pong activation images; the idle image doubles as staging for conv0
// (padded planes + 27*C weights) and the head convs
static inline size_t tower_lds_bytes(int H, int W, int C, int hc, int vf, int S)
{
    const size_t HW = (size_t)H * W, A = 2 * HW;
    const size_t s4 = (C + 8) / 4;
    const size_t img = ((((size_t)S * HW * s4 + 15) & ~(size_t)15) + 3 * s4) * 4; // floats, incl. zero region
    const size_t need0 = (size_t)S * 3 * (H + 2) * (W + 2) + (size_t)27 * C;
    // head phase: conv1x1 weights (VALU path) + staged head activations + 16 floats of slack + the FC logits of the samples
    const size_t nj = (A + 15) / 16 + (size_t)(vf + 15) / 16;
    const size_t need1 = (size_t)2 * hc * (C + 4) + (size_t)S * 2 * hc * HW + 16 + (size_t)S * (nj * 16 + 1);
    const size_t stage = need0 > need1 ? need0 : need1;
    return (img + (img > stage ? img : stage)) * 4;
}

struct TowerPlan {
    int S = 1, NT = 1, NTT = 7;                 // samples / position tiles per conv workgroup (NTT: compiled tile count)
    int S_small = 0, S_mid = 0, S_big = 0;      // tail launches: samples per workgroup of the <2,2> / <4,4> / <5,5> variants (0: unused)
    // f16x3 with two cout tiles per wave (k_tower<64, NT, 0, 1, true>, 64 channels): 4 tile groups of NT_c2 tiles
    int c2 = 0, S_c2 = 0, NT_c2 = 0;            // (its remainder goes to the one-cout-tile kernels)
    int use_rem = 0;                            // f16x3, NTT == 7: the remainder sizes live in ONE launch (k_tower_rem)
    size_t conv_lds = 0, conv_lds_c2 = 0;
    int S_main() const { return c2 ? S_c2 : S; } // samples per workgroup of the main launch: a round is cus * S_main samples
    int S_huge() const { return c2 ? S : 0; }    // two-cout-tile main launch: its largest tail body is the whole one-cout-tile geometry
};

// The plan of an H x W positions board (A = 2 * H * W actions), C padded channels, hc head channels, vf value-FC outputs.
// Returns nullptr, or the reason the geometry cannot run.
static inline const char *tower_plan_build(int H, int W, int C, int hc, int vf, int precision, TowerPlan &p)
{
    const int HW = H * W;
    auto lds_bytes = [&](int S_) { return tower_lds_bytes(H, W, C, hc, vf, S_); };
    p = TowerPlan();
    // conv workgroup geometry: S whole samples, NT position tiles of 16 rows (<= MAXT)
    int S = (16 * MAXT) / HW;
    if (S < 1) S = 1;
    // the samples of a workgroup are the 16 columns of head_fc_fused's MFMA and the 16 entries of slot_s: boards of at most 12
    // positions (1x1 ... 2x3) would take 17 ... 52, and samples 16.. of a full workgroup then got no logits at all
    if (S > MAXS) S = MAXS;
    while (S > 1 && lds_bytes(S) > TOWER_LDS_BUDGET) S--;
    if (lds_bytes(S) > TOWER_LDS_BUDGET) return "board / channels / head_channels too large for the LDS-resident tower";
    // k_tower_rem carries the static LDS of its four bodies (4 x (slot_s + rowbase_s)) on top of the images: where the remainder
    // launch would be used and the two do not fit into 160 KiB together, the workgroups take one sample less (128 channels with
    // 144 rows: 3x3, 5x5, 2x2 ... boards, whose commit failed in hipFuncSetAttribute before).  Conservative: without the
    // two-cout-tile main launch the remainder bodies hold at most S_big < S samples, so a dynamic-LDS size of its own for that
    // launch, lds_bytes(S_big), would fit as well and leave the main launch its sample
    if (precision == 1 && C >= 32)
        while (S > 1 && (S * HW + 15) / 16 > 8 && lds_bytes(S) + TOWER_REM_STATIC_LDS > TOWER_LDS_TOTAL) S--;
    p.S = S;
    p.NT = (S * HW + 15) / 16;
    p.conv_lds = lds_bytes(S);
    p.NTT = p.NT > 8 ? 7 : (p.NT > 4 ? 4 : 2); // tiles per wave; two waves cover 2*NTT >= NT tiles
    // tail variants: <2,2> holds 64 rows, <4,4> 128 rows, <5,5> 160 rows
    auto imin = [](int a, int b) { return a < b ? a : b; };
    auto imax = [](int a, int b) { return a > b ? a : b; };
    if (p.NTT == 7) {
        // S >= 1, so S_big >= 0; the two below it go negative where the one above is 0 (a single sample of > 160 rows)
        p.S_big = imin(160 / HW, p.S - 1);
        p.S_mid = imax(0, imin(128 / HW, p.S_big - 1));
        p.S_small = imax(0, imin(64 / HW, p.S_mid - 1));
    } else if (p.NTT == 4) {
        p.S_small = imin(64 / HW, p.S - 1);
    }
    p.c2 = (precision == 1 && C == 64) ? 1 : 0;
    if (p.c2) {
        int Sc = MAXROWS / HW;
        if (Sc > 16) Sc = 16;
        while (Sc > 1 && lds_bytes(Sc) + TOWER_WRING_BYTES > TOWER_LDS_BUDGET_C2) Sc--;
        p.S_c2 = Sc;
        p.NT_c2 = ((Sc * HW + 15) / 16 + 3) / 4;           // tiles per wave (4 groups)
        p.conv_lds_c2 = lds_bytes(Sc) + TOWER_WRING_BYTES;
        // worth it only where its 4 x NT_c2 tiles are filled about as well as the one-cout-tile kernel's NT (9x9: 200 of 256
        // rows against 200 of 208)
        const double fill_c2 = (double)Sc * HW / (64.0 * p.NT_c2), fill_1 = (double)p.S * HW / (16.0 * p.NT);
        // (0.9: 3x3 boards, 15 samples in 16 tiles against 13 in 13 -- their steps never fill a round of the main launch, but its
        // remainder bodies keep the residual stream in registers, which is worth 1.3 % there)
        if (fill_c2 < 0.9 * fill_1) p.c2 = 0;
        if (p.NT_c2 < 1 || p.NT_c2 > 4 || lds_bytes(Sc) + TOWER_WRING_BYTES > TOWER_LDS_BUDGET_C2) p.c2 = 0;
    }
    p.use_rem = (precision == 1 && p.NTT == 7 && C >= 32) ? 1 : 0;
    // the two-cout-tile main launch keeps the residual stream in registers; its remainder bodies must round the same way, and
    // those live in k_tower_rem<64, 1>: no remainder launch, no two-cout-tile main launch
    if (!p.use_rem) p.c2 = 0;
    return nullptr;
}

// which launch takes the samples behind the last full round of the main launch: 0 = the main launch itself, 1..4 = one
// round of workgroups with S_small / S_mid / S_big / S_huge samples each (every launch derives this from n on the device)
TOWER_PLAN_HD static inline int tower_split(int cus, int S_main, int S_small, int S_mid, int S_big, int S_huge, int n, int &n_full)
{
    const int per_round = cus * S_main;
    n_full = per_round > 0 ? (n / per_round) * per_round : 0;
    const int tail = n - n_full;
    if (tail <= 0) return 0;
    if (S_small > 0 && tail <= cus * S_small) return 1;
    if (S_mid > 0 && tail <= cus * S_mid) return 2;
    if (S_big > 0 && tail <= cus * S_big) return 3;
    if (S_huge > 0 && tail <= cus * S_huge) return 4; // (main = two cout tiles per wave: 4 = one round of the one-cout-tile kernel)
    return 0;
}
