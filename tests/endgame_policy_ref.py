"""The endgame solver's evaluator restated in numpy (helper of test_endgame_eval_cpu.py / test_hip_endgame_eval.py), written from
the definition in include/dbaz.h (dbaz_exact_policy), on top of endgame_ref.py.

policy(x, seed): every row is solved from scratch.  p is one-hot on one of the moves whose worth is the maximum -- the k-th in
ascending action order, k = 0 for seed 0, otherwise mix(key, seed) mod their number with key = the XOR over the row's free real
edges a of 1 << (a & 63) -- and v = sign(margin + D[0]).  A finished game gets p = 0 and v = get_result; a row with more than
max_free free edges gets p = 0, v = 0 and solved = False."""
import functools

import numpy as np

from oracle import oracle as O
import endgame_ref as ER
from solver_ref import mix

M64 = (1 << 64) - 1
_rows = {}


@functools.lru_cache(maxsize=None)
def _layers(F):
    """the masks of F bits by popcount"""
    m = np.arange(1 << F, dtype=np.uint32)
    pc = np.zeros(1 << F, np.int64)
    for i in range(F):
        pc += (m >> np.uint32(i)) & 1
    return [m[pc == k] for k in range(F + 1)]


def subgame(F, box_masks):
    """endgame_ref.subgame's recurrence with the completed boxes counted once per mask (the search tests ask for thousands of
    rows): D[full] = 0, D[mask] = max over free e of c + D[mask | e] if c > 0 else -D[mask | e], c = boxes the move completes"""
    m = np.arange(1 << F, dtype=np.uint32)
    done = np.zeros(1 << F, np.int16)  # boxes whose free edges are all drawn in the mask
    for bm in box_masks:
        done += (m & np.uint32(bm)) == bm
    D = np.zeros(1 << F, np.int16)
    layers = _layers(F)
    for k in range(F - 1, -1, -1):
        s = layers[k]
        best = np.full(len(s), -128, np.int16)
        for e in range(F):
            free = (s >> np.uint32(e)) & 1 == 0
            sf = s[free]
            t = sf | np.uint32(1 << e)
            c, d = done[t] - done[sf], D[t]
            best[free] = np.maximum(best[free], np.where(c > 0, c + d, -d))
        D[s] = best
    return D


def solved_row(R, C, x):
    """dict(value, q int8 [A], n_free, finished) of one row, as endgame_ref.endgame_ref defines them; computed once per
    distinct row"""
    x = np.asarray(x).ravel().astype(np.int16)
    key = (R, C, x.tobytes())
    if key in _rows:
        return _rows[key]
    acts, boxes = ER.board(R, C)
    HW, A, B = (R + 1) * (C + 1), 2 * (R + 1) * (C + 1), R * C
    free = [a for a in acts if x[a] == 0]
    idx = {a: j for j, a in enumerate(free)}
    box_masks = [sum(1 << idx[a] for a in b if a in idx) for b in boxes]
    closed = sum(bm == 0 for bm in box_masks)
    open_masks = [bm for bm in box_masks if bm]
    D = subgame(len(free), open_masks)
    own = int(x[2 * HW])
    mine = (B - own) // 2
    theirs = closed - mine
    opp = B - 2 * theirs
    res = 0 if (own == 0 and opp == 0) else 1 if own < 0 else -1 if opp < 0 else None
    q = np.full(A, -128, np.int8)
    if res is None:
        for j, a in enumerate(free):
            c = sum(1 for bm in open_masks if bm == 1 << j)
            d = int(D[1 << j])
            q[a] = c + d if c > 0 else -d
    value = res if res is not None else int(np.sign(mine - theirs + int(D[0])))
    _rows[key] = dict(value=value, q=q, n_free=len(free), finished=res is not None)
    return _rows[key]


def pick_key(R, C, x):
    acts, _ = ER.board(R, C)
    key = 0
    for a in acts:
        if x[a] == 0:
            key ^= 1 << (a & 63)
    return key & M64


def optimal_set(R, C, x):
    """actions whose worth is the maximum, ascending ([] for a finished game)"""
    r = solved_row(R, C, x)
    if r["finished"]:
        return []
    q = r["q"].astype(np.int64)
    legal = np.nonzero(q != -128)[0]
    return [int(a) for a in legal if q[a] == q[legal].max()]


def policy_one(R, C, x, seed=0, max_free=16):
    """(picked action or -1, v, solved) of one feature row"""
    x = np.asarray(x).ravel()
    acts, _ = ER.board(R, C)
    if sum(1 for a in acts if x[a] == 0) > max_free:
        return -1, 0.0, False
    opt = optimal_set(R, C, x)
    v = float(solved_row(R, C, x)["value"])
    if not opt:
        return -1, v, True
    k = mix(pick_key(R, C, x), seed) % len(opt) if seed else 0
    return opt[k], v, True


def policy(R, C, x, seed=0, max_free=16):
    """x int16 / float [n, 3*H*W] (or [n, 3, H, W]) -> (p float32 [n, A], v float32 [n], solved bool [n])"""
    A = 2 * (R + 1) * (C + 1)
    x = np.asarray(x).reshape(-1, 3 * (R + 1) * (C + 1))
    p = np.zeros((len(x), A), np.float32)
    v = np.zeros(len(x), np.float32)
    solved = np.zeros(len(x), bool)
    for r in range(len(x)):
        a, v[r], solved[r] = policy_one(R, C, x[r], seed, max_free)
        if a >= 0:
            p[r, a] = 1.0
    return p, v, solved


def random_games(R, C, n_games, seed):
    """(feature rows int16 of every position of n_games games played until no edge is free, free edges per row): the rows behind
    an early end are finished games with free edges left.  Even games: uniformly random play; odd games: a capture while there is
    one, else a move that leaves no box with three edges while there is one, else any -- late positions of every value."""
    d = O.dims(R, C)
    acts, boxes = ER.board(R, C)
    rs = np.random.RandomState(seed)
    xs = []
    for game in range(n_games):
        s = O.new_state(d)
        for left in range(len(acts), -1, -1):
            x = O.features(d, s).ravel().copy()
            xs.append(x)
            free = [a for a in acts if x[a] == 0]
            if game % 2:
                drawn = {a: [sum(x[o] != 0 for o in b) for b in boxes if a in b] for a in free}
                free = [a for a in free if 3 in drawn[a]] or [a for a in free if 2 not in drawn[a]] or free
            if free:
                O.play_(d, s, int(free[rs.randint(len(free))]))
    xs = np.array(xs, np.int16)
    return xs, (xs[:, acts] == 0).sum(axis=1)


def other_mover(R, C, x):
    """the same boards with the other player to move (plane 2 holds that player's doubled boxes_to_close): random play leaves the
    mover ahead, these are the rows the mover loses"""
    _, boxes = ER.board(R, C)
    HW = (R + 1) * (C + 1)
    closed = sum((x[:, b] != 0).all(axis=1).astype(np.int64) for b in boxes)
    mine = (R * C - x[:, 2 * HW].astype(np.int64)) // 2
    y = x.copy()
    y[:, 2 * HW:] = (R * C - 2 * (closed - mine))[:, None]
    return y
