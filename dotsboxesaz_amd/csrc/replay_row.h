// replay_row.h -- the byte layout of one packed replay row, RowMeta | x int16[3HW] | visits int32[A] padded to 8 bytes
// (DESIGN.md "replay row"; RowMeta: common.h, self_play.ROW_META).  The one definition for the readers that do not need the
// engine's headers: replay.hip (dataset build) and solver.hip (dbaz_replay_exact_targets).  Rows start 8-byte aligned; x is
// 2-byte aligned and so are the visits (28 + 6 HW is no multiple of 4 on a board with odd HW).
#pragma once

#define ROW_GAME_OFF 0  // int32 RowMeta.game_idx
#define ROW_MOVE_OFF 4  // int16 RowMeta.move_idx
#define ROW_Z_OFF 25    // int8 RowMeta.z
#define ROW_X_OFF 28    // sizeof(RowMeta)

// row_bytes of a board with HW = (rows + 1) * (cols + 1) points
static inline int replay_row_bytes(int HW) { return (int)((ROW_X_OFF + (size_t)3 * HW * 2 + (size_t)2 * HW * 4 + 7) & ~(size_t)7); }
