"""The exact solver and its evaluator restated in numpy (helper of test_solver_eval_cpu.py / test_hip_solver_eval.py), written
from the definitions in include/dbaz.h, not from the kernels.

Table: D[mask] = best achievable (mover's boxes) - (opponent's boxes) over the boxes still open; bit i of a mask = compact edge i,
the i-th real edge in ascending action order.  D[full] = 0; drawing free edge e that completes c boxes is worth c + D[mask | e]
when c > 0 (the mover continues) and -D[mask | e] otherwise; D[mask] = the maximum.

Evaluator: p one-hot on one of the moves whose worth is that maximum -- the k-th in ascending order, k = 0 for seed 0, otherwise
mix(mask, seed) mod their number -- and v = sign(margin + D[mask]); a finished game gets p = 0 and v = get_result."""
import functools

import numpy as np

M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def geometry(R, C):
    """(action index of compact edge i, per box its four compact edges)"""
    H, W = R + 1, C + 1
    HW = H * W
    acts = sorted([l * W + c for l in range(H) for c in range(C)] + [HW + l * W + c for l in range(R) for c in range(W)])
    idx = {a: i for i, a in enumerate(acts)}
    boxes = [[idx[l * W + c], idx[(l + 1) * W + c], idx[HW + l * W + c], idx[HW + l * W + c + 1]] for l in range(R) for c in range(C)]
    return acts, boxes


def solve(R, C):
    """int8 D[2^E] by popcount layers, every layer vectorised over its masks"""
    acts, boxes = geometry(R, C)
    E = len(acts)
    m = np.arange(1 << E, dtype=np.uint32)
    pc = np.zeros(1 << E, np.uint8)
    for i in range(E):
        pc += ((m >> np.uint32(i)) & 1).astype(np.uint8)
    D = np.zeros(1 << E, np.int8)
    for k in range(E - 1, -1, -1):
        s = m[pc == k]
        best = np.full(len(s), -128, np.int16)
        for e in range(E):
            t = s[(s >> np.uint32(e)) & 1 == 0]
            c = np.zeros(len(t), np.int16)
            for b in boxes:
                if e in b:
                    o = np.uint32(sum(1 << j for j in b if j != e))
                    c += (t & o) == o
            d = D[t | np.uint32(1 << e)].astype(np.int16)
            free = (s >> np.uint32(e)) & 1 == 0
            best[free] = np.maximum(best[free], np.where(c > 0, c + d, -d))
        D[s] = best.astype(np.int8)
    return D


_tables = {}


def table(R, C):
    if (R, C) not in _tables:
        _tables[(R, C)] = solve(R, C)
    return _tables[(R, C)]


def mix(mask, seed):
    """splitmix64 finaliser of mask ^ seed * 0x9E3779B97F4A7C15 (64-bit, wrapping)"""
    x = (int(mask) ^ (int(seed) * 0x9E3779B97F4A7C15)) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def row_facts(R, C, x):
    """(mask, margin, result or None) of one feature row [3*H*W]: planes 0, 1 = edges, plane 2 = the mover's doubled
    boxes_to_close; get_result as dots_boxes_game.py:51-59 (a finished game, early end included)"""
    acts, boxes = geometry(R, C)
    HW = (R + 1) * (C + 1)
    mask = sum(1 << i for i, a in enumerate(acts) if x[a] != 0)
    closed = sum(all(mask >> j & 1 for j in b) for b in boxes)
    own = int(x[2 * HW])
    mine = (R * C - own) // 2
    theirs = closed - mine
    opp = R * C - 2 * theirs
    res = None
    if own == 0 and opp == 0:
        res = 0
    elif own < 0:
        res = 1
    elif opp < 0:
        res = -1
    return mask, mine - theirs, res


def move_values(R, C, D, mask):
    """{compact edge: worth of drawing it} over the free edges of mask"""
    acts, boxes = geometry(R, C)
    out = {}
    for e in range(len(acts)):
        if mask >> e & 1:
            continue
        c = sum(1 for b in boxes if e in b and all(mask >> j & 1 for j in b if j != e))
        d = int(D[mask | 1 << e])
        out[e] = c + d if c > 0 else -d
    return out


_memo = {}


def policy_one(D, R, C, x, seed=0):
    """(picked action or -1, v) of one feature row"""
    mask, margin, res = row_facts(R, C, x)
    if res is not None:
        return -1, float(res)
    key = (R, C, mask, int(seed))
    if key not in _memo:
        q = move_values(R, C, D, mask)
        best = max(q.values())
        opt = [e for e in sorted(q) if q[e] == best]
        k = mix(mask, seed) % len(opt) if seed else 0
        _memo[key] = geometry(R, C)[0][opt[k]]
    return _memo[key], float(np.sign(margin + int(D[mask])))


def policy_ref(D, rows, cols, x, seed=0):
    """x int16 / float [n, 3*H*W] (or [n, 3, H, W]) -> (p float32 [n, A], v float32 [n])"""
    A = 2 * (rows + 1) * (cols + 1)
    x = np.asarray(x).reshape(-1, 3 * (rows + 1) * (cols + 1))
    p = np.zeros((len(x), A), np.float32)
    v = np.zeros(len(x), np.float32)
    for r in range(len(x)):
        a, v[r] = policy_one(D, rows, cols, x[r], seed)
        if a >= 0:
            p[r, a] = 1.0
    return p, v
