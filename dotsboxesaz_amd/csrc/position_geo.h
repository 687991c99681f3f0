// position_geo.h -- the subgame of ONE position as a solver geometry ("deep endgames"), host only and without
// HIP types: solver.hip builds a SolverGeo from it, tests/test_position_geo.py compiles it with g++.
//
// D depends only on which edges are free, so a position with F free real edges on any board with
// A <= DBAZ_MAX_A is a game over the 2^F subsets of those edges:
//   compact edge j   the j-th free real edge of the position in ascending action order (bit j of a table index: drawn since)
//   other[j][0..1]   solver_move_q's masks over the COMPACT edges, per bordering box the other edges that are still free:
//                    0 where all three are drawn (the edge completes that box whatever else happens), POSITION_NO_BOX where
//                    there is no such box (the value of SOLVER_NO_BOX, solver.h)
// The real edges come from the board, as in solver_geometry: a sentinel slot is never an edge, whatever the row holds there.
#pragma once

#include <stdint.h>

#include "../../include/dbaz.h"

#define POSITION_MAX_FREE 31          // a table of 2^F bytes, masks of at most 31 bits (SOLVER_MAX_E)
#define POSITION_NO_BOX 0x80000000u   // bit 31 is never set in a mask: a box mask that never matches

struct PositionGeo {
    int32_t F;                               // free real edges of the row; counted to the end, also past POSITION_MAX_FREE
    uint64_t free_edges[4];                  // the free real edges by action index (complete for every F)
    uint8_t act[POSITION_MAX_FREE + 1];      // compact edge -> action index, ascending; the first min(F, 31) hold
    uint32_t other[POSITION_MAX_FREE][2];    // valid only for F <= POSITION_MAX_FREE; entries j >= F are POSITION_NO_BOX
};

// x: one feature row int16 [3*H*W] (planes 0, 1: edges, nonzero = drawn).  Returns 0, or 1 when F > POSITION_MAX_FREE (F and
// free_edges are valid, there is no geometry), or -1 for a board the engine does not support (rows, cols < 1 or A > DBAZ_MAX_A).
static inline int position_geometry(int rows, int cols, const int16_t *x, PositionGeo &p)
{
    p = PositionGeo();
    if (rows < 1 || cols < 1 || 2ll * (rows + 1ll) * (cols + 1ll) > DBAZ_MAX_A) return -1;
    const int H = rows + 1, W = cols + 1, HW = H * W, A = 2 * HW;
    int cidx[DBAZ_MAX_A]; // action -> compact edge, -1: drawn, a sentinel slot, or past the 31st free edge
    int F = 0;
    for (int a = 0; a < A; a++) {
        const int pl = a / HW, l = (a % HW) / W, c = a % W;
        const bool real = pl == 0 ? c < cols : l < rows; // sentinels: board[0,:,W-1] and board[1,H-1,:]
        cidx[a] = -1;
        if (!real || x[a] != 0) continue;
        p.free_edges[a >> 6] |= 1ull << (a & 63);
        if (F < POSITION_MAX_FREE) {
            cidx[a] = F;
            p.act[F] = (uint8_t)a;
        }
        F++;
    }
    p.F = F;
    for (int j = 0; j < POSITION_MAX_FREE; j++) p.other[j][0] = p.other[j][1] = POSITION_NO_BOX;
    if (F > POSITION_MAX_FREE) return 1;
    int used[POSITION_MAX_FREE] = {0};
    for (int l = 0; l < rows; l++)
        for (int c = 0; c < cols; c++) {
            const int ed[4] = {l * W + c, (l + 1) * W + c, HW + l * W + c, HW + l * W + c + 1};
            uint32_t bm = 0; // the box's free edges
            for (int k = 0; k < 4; k++)
                if (cidx[ed[k]] >= 0) bm |= 1u << cidx[ed[k]];
            for (int k = 0; k < 4; k++) {
                const int j = cidx[ed[k]];
                if (j >= 0) p.other[j][used[j]++] = bm & ~(1u << j);
            }
        }
    return 0;
}
