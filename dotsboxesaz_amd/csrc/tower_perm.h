// tower_perm.h -- which LDS row each lane of each position tile of the two-cout-tile tower body processes (plain C++, host only).
//
// conv_lds_h3_c2 runs 16 position tiles of 16 rows: wave pair g (= wave >> 1) owns tiles 4g .. 4g + 3.  In natural order
// (tile T, lane j -> row T * 16 + j) every tile mixes border and interior positions, so no tile can skip a tap.  The table
// built here hands the rows out so that tiles 0 and 1 of every pair hold rows of ONE border only; such a tile lacks a whole
// row or column of the 3x3 kernel and the body drops those three taps for it (their B operand would be all zero):
//
//     pair 0: tile 0 top,    tile 1 left        top    (y = 0)     drops taps 0 1 2
//     pair 1: tile 0 top,    tile 1 right       bottom (y = H - 1) drops taps 6 7 8
//     pair 2: tile 0 bottom, tile 1 right       left   (x = 0)     drops taps 0 3 6
//     pair 3: tile 0 bottom, tile 1 left        right  (x = W - 1) drops taps 2 5 8
//
// (a workgroup's waves go to the SIMDs cyclically, so pairs 0 and 2 share two SIMDs and pairs 1 and 3 the other two: with
// this assignment both halves drop 2 1 2 1 0 1 2 1 2 tiles at taps 0..8 and the per-step barrier never waits for a fuller half)
// Rows >= S * HW do not exist (padding): their lanes are invalid in the kernel and may sit in any tile.
#pragma once

#define TOWER_PERM_ROWS 256
#define TOWER_PERM_TILES 16

enum { TP_TOP = 0007, TP_BOTTOM = 0700, TP_LEFT = 0111, TP_RIGHT = 0444 }; // 9-bit tap masks, tap = (dy + 1) * 3 + dx + 1

// the taps tile T (0..15) drops under the pattern
static inline int tower_perm_drop(int T)
{
    static const int edge[4][2] = {{TP_TOP, TP_LEFT}, {TP_TOP, TP_RIGHT}, {TP_BOTTOM, TP_RIGHT}, {TP_BOTTOM, TP_LEFT}};
    return (T & 3) < 2 ? edge[T >> 2][T & 3] : 0;
}

// the taps of position (y, x) whose source pixel lies inside the H x W image
static inline int tower_perm_inside(int H, int W, int y, int x)
{
    int m = 0;
    for (int tap = 0; tap < 9; tap++) {
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) m |= 1 << tap;
    }
    return m;
}

// Fills tab[T * 16 + j] = natural row (sample * H * W + y * W + x) of lane j of tile T for workgroups of S samples of H x W
// positions.  Returns the number of dropped (tile, tap) pairs (24) when the pattern above is met -- tab is then a permutation
// of 0..255 in which no real row of an edge tile has a dropped tap inside the image -- and 0 with the identity table when it
// is not (the rows do not fill exactly 4 tiles per pair, or a border has too few rows and the padding cannot make up for it).
static inline int tower_perm_build(int H, int W, int S, int *tab)
{
    enum { NR = TOWER_PERM_ROWS, NTL = TOWER_PERM_TILES };
    for (int i = 0; i < NR; i++) tab[i] = i;
    if (H < 1 || W < 1 || S < 1) return 0;
    const int HW = H * W, R = S * HW;
    if (R > NR || ((R + 15) / 16 + 3) / 4 != 4) return 0;
    const int cls_mask[4] = {TP_TOP, TP_BOTTOM, TP_LEFT, TP_RIGHT};
    // the borders a row can serve: bit k = none of cls_mask[k]'s taps is inside the image (padding serves all four)
    int caps[NR], owner[NR]; // owner: 0..3 = border class, 4 = unconstrained
    int have[5] = {0, 0, 0, 0, 0};
    for (int r = 0; r < NR; r++) {
        caps[r] = 15;
        if (r < R) {
            const int p = r % HW, in = tower_perm_inside(H, W, p / W, p % W);
            caps[r] = 0;
            for (int k = 0; k < 4; k++)
                if (!(in & cls_mask[k])) caps[r] |= 1 << k;
        }
        owner[r] = 4;
    }
    // 1. rows of one border only, 2. rows of two or more borders (corners) to the class that lacks most, 3. padding
    for (int pass = 0; pass < 3; pass++)
        for (int r = 0; r < NR; r++) {
            if (owner[r] != 4 || caps[r] == 0) continue;
            const bool single = (caps[r] & (caps[r] - 1)) == 0;
            if (pass == 0 ? !single : pass == 1 ? (single || r >= R) : r < R) continue;
            int best = -1;
            for (int k = 0; k < 4; k++)
                if ((caps[r] >> k & 1) && have[k] < 32 && (best < 0 || have[k] < have[best])) best = k;
            if (best >= 0) { owner[r] = best; have[best]++; }
        }
    for (int k = 0; k < 4; k++)
        if (have[k] != 32) return 0;
    // rows of a class -> its tiles.  ds_read_b128 serves lanes {0-3, 12-15} and {4-11} of a 16-row quarter together and a
    // row's bank slot is (2 * row + const) mod 16, so a tile reads without conflicts when the rows of either lane set differ
    // mod 8: every lane set takes, residue by residue, a row of the residue that has most rows left (a preference only)
    static const int cls_tiles[5][8] = {{0, 4}, {8, 12}, {1, 13}, {5, 9}, {2, 3, 6, 7, 10, 11, 14, 15}};
    static const int lane_set[2][8] = {{4, 5, 6, 7, 8, 9, 10, 11}, {0, 1, 2, 3, 12, 13, 14, 15}};
    bool used[NR];
    for (int r = 0; r < NR; r++) used[r] = false;
    for (int k = 0; k < 5; k++) {
        const int ntl = k < 4 ? 2 : 8;
        for (int ti = 0; ti < ntl; ti++)
            for (int h = 0; h < 2; h++) {
                bool res_used[8] = {false, false, false, false, false, false, false, false};
                for (int q = 0; q < 8; q++) {
                    int left[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    for (int r = 0; r < NR; r++)
                        if (owner[r] == k && !used[r]) left[r & 7]++;
                    int br = -1;
                    for (int m = 0; m < 8; m++)
                        if (left[m] > 0 && !res_used[m] && (br < 0 || left[m] > left[br])) br = m;
                    if (br < 0)
                        for (int m = 0; m < 8; m++)
                            if (left[m] > 0 && (br < 0 || left[m] > left[br])) br = m;
                    if (br < 0) { for (int i = 0; i < NR; i++) tab[i] = i; return 0; }
                    int r = 0;
                    while (owner[r] != k || used[r] || (r & 7) != br) r++;
                    used[r] = true;
                    res_used[br] = true;
                    tab[cls_tiles[k][ti] * 16 + lane_set[h][q]] = r;
                }
            }
    }
    // verify: a permutation, and no real row of a tile has a tap inside the image that the tile drops
    int seen[NR], dropped = 0;
    for (int r = 0; r < NR; r++) seen[r] = 0;
    bool ok = true;
    for (int T = 0; T < NTL; T++) {
        const int drop = tower_perm_drop(T);
        for (int tap = 0; tap < 9; tap++) dropped += drop >> tap & 1;
        for (int j = 0; j < 16; j++) {
            const int r = tab[T * 16 + j];
            if (r < 0 || r >= NR || seen[r]++) { ok = false; continue; }
            if (r < R && (tower_perm_inside(H, W, (r % HW) / W, (r % HW) % W) & drop)) ok = false;
        }
    }
    if (!ok) {
        for (int i = 0; i < NR; i++) tab[i] = i;
        return 0;
    }
    return dropped;
}
