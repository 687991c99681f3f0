// replay_row.h -- the byte layout of one packed replay row, RowMeta | x int16[3HW] | visits int32[A] padded to 8 bytes
// (DESIGN.md "replay row"; RowMeta: common.h, self_play.ROW_META).  The one definition for the readers that do not need the
// engine's headers: replay.hip (dataset build) and solver.hip (dbaz_replay_exact_targets).  Rows start 8-byte aligned; x is
// 2-byte aligned and so are the visits (28 + 6 HW is no multiple of 4 on a board with odd HW).
#pragma once

#define ROW_GAME_OFF 0  // int32 RowMeta.game_idx
#define ROW_MOVE_OFF 4  // int16 RowMeta.move_idx
#define ROW_Z_OFF 25    // int8 RowMeta.z
#define ROW_FLAGS_OFF 26 // int16 RowMeta.flags ("pad" in the numpy dtypes): 0 on every row made without a playout cap
#define ROW_FLAG_FAST 1  //   bit 0: the row's search was a fast one (playout_cap.h): it moved the game on and is not a training target
#define ROW_FLAG_PRUNED 2 //  bit 1: policy target pruning ran on the row (forced_playouts.h): its visits are the pruned ones
#define ROW_FLAG_GUMBEL 4 //  bit 2: the row's search was a Gumbel search (gumbel.h): its visits are the target pi' in units of 2^-24
#define ROW_FLAG_GUMBEL_FULL 8 // bit 3, beside bit 2: that search ran the full mode (dbaz_selfplay_set_gumbel_mode): the rule below the root too
#define ROW_X_OFF 28    // sizeof(RowMeta)

// row_bytes of a board with HW = (rows + 1) * (cols + 1) points
static inline int replay_row_bytes(int HW) { return (int)((ROW_X_OFF + (size_t)3 * HW * 2 + (size_t)2 * HW * 4 + 7) & ~(size_t)7); }
