// table_row.h -- one feature row against one solved table, device code shared by endgame.hip and solver.hip.
// Needs solver.h only.  One wavefront per row, lane j = compact edge j of the table's root (at most 31 < 64): the closed boxes
// from planes 0 / 1 and solver_facts, the ballot of the drawn compact edges, Q of every free lane's successor -- then the caller
// picks (endgame_pick), scores or relabels (row_members, relabel_entry).  The table's kind does not matter: the root is anything
// with free_edges[4], other[][2] and act[] (EndgameSlotHdr, DeepRoot).
#pragma once

#include "solver.h"

__host__ __device__ __forceinline__ int sgn(int v) { return (v > 0) - (v < 0); }

// The board as the row readers need it.  It travels in the kernel arguments, never in a root header: a row's loads do not wait
// for the root's.
struct TablesBoard {
    int32_t rows, cols, HW, A;
};
static inline TablesBoard tables_board(int rows, int cols)
{
    TablesBoard B;
    B.rows = rows; B.cols = cols; B.HW = (rows + 1) * (cols + 1); B.A = 2 * B.HW;
    return B;
}

// action slot a is a real edge of the board (the sentinels are board[0,:,W-1] and board[1,H-1,:])
static __device__ __forceinline__ bool board_real_edge(const TablesBoard &B, int a)
{
    const int W = B.cols + 1;
    const int p = a / B.HW, l = (a % B.HW) / W, c = a % W;
    return a < B.A && (p == 0 ? c < B.cols : l < B.rows);
}

// The free real edges of a row by action index, one ballot per 64 action slots (lane l looks at slots l, 64 + l, ...); returns
// their number.
template <typename T>
static __device__ __forceinline__ int row_free_edges(const TablesBoard &B, const T *__restrict__ xr, int lane, uint64_t (&free_edges)[4])
{
    int n = 0;
#pragma unroll
    for (int w = 0; w < DBAZ_MAX_A / 64; w++) {
        const int a = w * 64 + lane;
        free_edges[w] = __ballot(board_real_edge(B, a) && xr[a] == (T)0);
        n += __popcll(free_edges[w]);
    }
    return n;
}

// the boxes of a row with all four edges drawn, 64 boxes per ballot
template <typename T>
static __device__ __forceinline__ int row_closed_boxes(const TablesBoard &B, const T *__restrict__ xr, int lane)
{
    const int W = B.cols + 1, n_boxes = B.rows * B.cols;
    int closed = 0;
    for (int b0 = 0; b0 < n_boxes; b0 += 64) {
        const int b = b0 + lane;
        bool c = false;
        if (b < n_boxes) {
            const int at = (b / B.cols) * W + b % B.cols;
            c = xr[at] != (T)0 && xr[at + W] != (T)0 && xr[B.HW + at] != (T)0 && xr[B.HW + at + 1] != (T)0;
        }
        closed += __popcll(__ballot(c));
    }
    return closed;
}

// Compact edge of action slot a within a free-edge set: its rank among the set's edges in ascending action order.
static __device__ __forceinline__ uint64_t word_of(const uint64_t (&fe)[4], int w)
{
    return w == 0 ? fe[0] : w == 1 ? fe[1] : w == 2 ? fe[2] : fe[3];
}
static __device__ __forceinline__ int edge_rank(const uint64_t (&fe)[4], int a)
{
    const int w = a >> 6;
    int r = __popcll(word_of(fe, w) & ((1ull << (a & 63)) - 1ull));
#pragma unroll
    for (int i = 0; i < 3; i++)
        if (i < w) r += __popcll(fe[i]);
    return r;
}

// What one wavefront finds out about its row, the same in every lane unless noted.
struct TableRow {
    uint64_t row_free[4]; // SERVED_CHECK only: the row's free real edges by action index
    int n_free;           // SERVED_CHECK only
    bool served, open;
    uint32_t m;           // the drawn compact edges of the root
    RowFacts f;
    bool cand;            // per lane: compact edge `lane` is free and the game is open
    int a, q;             // per lane: the edge's action index; its worth (cand only)
};

// R: the table's root with F compact edges, Tb its table.  SERVED_CHECK: a row is served when its free real edges are a subset
// of the root's (four ballots over the action slots); without it the caller vouches for that and `served` is true.
template <bool SERVED_CHECK, typename Root, typename T>
static __device__ __forceinline__ TableRow table_row(const TablesBoard &board, const Root &R, int F, const int8_t *__restrict__ Tb,
                                                     const T *__restrict__ xr, int lane)
{
    TableRow d;
    d.n_free = 0;
    d.served = true;
    if (SERVED_CHECK) {
        d.n_free = row_free_edges(board, xr, lane, d.row_free);
#pragma unroll
        for (int w = 0; w < DBAZ_MAX_A / 64; w++) d.served = d.served && (d.row_free[w] & ~R.free_edges[w]) == 0ull;
    }
    const bool edge = lane < F;
    d.a = edge ? (int)R.act[lane] : 0;
    const bool drawn = edge && xr[d.a] != (T)0;
    d.m = (uint32_t)__ballot(drawn);
    d.f = solver_facts(board.rows * board.cols, row_closed_boxes(board, xr, lane), (int)xr[2 * board.HW]);
    d.open = d.f.res == DBAZ_RESULT_NONE;
    d.cand = d.served && d.open && edge && !drawn;
    d.q = d.cand ? solver_move_q(R.other[lane][0], R.other[lane][1], d.m, (int)Tb[d.m | (1u << lane)]) : 0;
    return d;
}

// ---- the relabel rule of include/dbaz.h (dbaz_exact_targets), lane c = compact edge c of F ---------------------------------
// O = the edges that keep the result v, as a ballot, and S = the float32 sum of their p in ascending action order, starting
// from 0 -- the same additions in every lane, and k_endgame_score's policy_mass.  Called by a whole wavefront.
struct RowMembers {
    uint32_t set;
    float sum;
};
static __device__ __forceinline__ RowMembers row_members(bool cand, int margin, int q, int v, float p, int F)
{
    RowMembers M;
    M.set = (uint32_t)__ballot(cand && sgn(margin + q) == v);
    M.sum = 0.0f;
    for (int c = 0; c < F; c++) { // ascending action order
        const float pc = __shfl(p, c);
        if ((M.set >> c) & 1u) M.sum += pc;
    }
    return M;
}

// pi of one action slot after the relabel (pi_mode 1 uniform, 2 restrict): 1/|O| or p/S on a member -- one float32 division --
// and 0 anywhere else.  member: the slot is a free edge whose compact edge is in M.set.
static __device__ __forceinline__ float relabel_entry(const RowMembers &M, int pi_mode, bool member, float p)
{
    const bool uniform = pi_mode == 1 || !(M.sum > 0.0f);
    return member ? (uniform ? 1.0f / (float)__popc(M.set) : p / M.sum) : 0.0f;
}
