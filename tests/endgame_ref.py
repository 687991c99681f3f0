"""The exact endgame solver restated in numpy (helper of test_endgame_cpu.py / test_hip_endgame.py), written from the definition
in include/dbaz.h and DESIGN.md 4.7, not from the kernel.

A position's subgame: its F free real edges in ascending action order are compact edges 0 .. F-1, a mask over them says which
have been drawn since.  D[full] = 0; drawing free edge e that completes c boxes (a box completes when its other three edges are
drawn, in the row or in the mask) is worth c + D[mask | e] when c > 0 (the mover continues) and -D[mask | e] otherwise;
D[mask] = the maximum.  value = sign(margin + D[0]), or get_result of a finished game (early end included)."""
import numpy as np


def board(R, C):
    """(action indices of the real edges ascending, per box the action indices of its four edges)"""
    H, W = R + 1, C + 1
    HW = H * W
    acts = sorted([l * W + c for l in range(H) for c in range(C)] + [HW + l * W + c for l in range(R) for c in range(W)])
    boxes = [[l * W + c, (l + 1) * W + c, HW + l * W + c, HW + l * W + c + 1] for l in range(R) for c in range(C)]
    return acts, boxes


def subgame(F, box_masks):
    """int8 D[2^F] by popcount layers, each vectorised over its masks.  box_masks: per still-open box the mask of its free edges."""
    m = np.arange(1 << F, dtype=np.uint32)
    pc = np.zeros(1 << F, np.uint8)
    for i in range(F):
        pc += ((m >> np.uint32(i)) & 1).astype(np.uint8)
    D = np.zeros(1 << F, np.int8)
    for k in range(F - 1, -1, -1):
        s = m[pc == k]
        best = np.full(len(s), -128, np.int16)
        for e in range(F):
            free = (s >> np.uint32(e)) & 1 == 0
            t = s[free] | np.uint32(1 << e)
            c = np.zeros(len(t), np.int16)
            for bm in box_masks:
                if bm >> e & 1:
                    c += (t & np.uint32(bm)) == bm  # the box is complete after the move
            d = D[t].astype(np.int16)
            best[free] = np.maximum(best[free], np.where(c > 0, c + d, -d))
        D[s] = best.astype(np.int8)
    return D


def endgame_ref(R, C, x_row, pi_row=None):
    """dict(value, diff, q int8 [A], policy_mass float32 or None, n_free, finished) of one feature row [3*H*W]"""
    acts, boxes = board(R, C)
    HW, A, B = (R + 1) * (C + 1), 2 * (R + 1) * (C + 1), R * C
    x = np.asarray(x_row).ravel()
    free = [a for a in acts if x[a] == 0]
    F = len(free)
    idx = {a: j for j, a in enumerate(free)}
    box_masks = [sum(1 << idx[a] for a in b if a in idx) for b in boxes]
    closed = sum(bm == 0 for bm in box_masks)
    D = subgame(F, [bm for bm in box_masks if bm])
    own = int(x[2 * HW])
    mine = (B - own) // 2
    theirs = closed - mine
    opp = B - 2 * theirs
    margin = mine - theirs
    res = 0 if (own == 0 and opp == 0) else 1 if own < 0 else -1 if opp < 0 else None
    q = np.full(A, -128, np.int8)
    mass = np.float32(0)
    if res is None:
        value = int(np.sign(margin + int(D[0])))
        for j, a in enumerate(free):  # ascending a
            c = sum(1 for bm in box_masks if bm == 1 << j)
            d = int(D[1 << j])
            q[a] = c + d if c > 0 else -d
            if pi_row is not None and np.sign(margin + int(q[a])) == value:
                mass = np.float32(mass + np.float32(pi_row[a]))
    else:
        value = res
    return dict(value=value, diff=int(D[0]), q=q, policy_mass=mass if pi_row is not None else None, n_free=F, finished=res is not None)
