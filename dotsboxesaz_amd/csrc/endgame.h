// endgame.h -- sizes and device-side geometry of the exact endgame solver (endgame.hip).
// Needs solver.h (solver_move_q, solver_facts, popcount_order, SOLVER_NO_BOX) and include/dbaz.h only.
#pragma once

#include "solver.h"

#define ENDGAME_MAX_FREE 16   // 2^16 int8 = 64 KB of LDS per position, subgame masks as uint16
#define ENDGAME_THREADS 512   // SOLVER_THREADS; one lane per real edge during setup needs E < DBAZ_MAX_A <= ENDGAME_THREADS
#define ENDGAME_OFF_STRIDE (ENDGAME_MAX_FREE + 2)

// Real edge i = rank of the edge's action index among the real edges of the board (ascending), as in solver.h, for any board with
// A <= DBAZ_MAX_A.  The per-edge tables live in HBM (E < 256 edges do not fit the kernel arguments):
//   action [E]        real edge -> action index
//   nbr    [E][2][3]  per bordering box the action indices of its three OTHER edges (-1, -1, -1: no such box)
//   perm   [2^17 - 1] for every F = 0 .. 16 the masks of F bits in ascending popcount order, list F at 2^F - 1
//   off    [17][18]   off[F][k] .. off[F][k + 1]: the masks of popcount k within list F
struct EndgameGeo {
    int32_t rows, cols, HW, A, E, max_free;
    const uint8_t *action;
    const int16_t *nbr;
    const uint16_t *perm;
    const uint32_t *off;
};
