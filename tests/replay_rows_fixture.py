"""Packed replay rows for the two kernel families that read them (csrc/replay_row.h), on any board, from seeds: numpy only, no GPU.
Helper of test_replay_rows_fixture_cpu.py (what the references alone say about these inputs), test_hip_replay_targets_boards.py
(dbaz_replay_exact_targets) and test_hip_train_data_boards.py (dbaz_dataset_*, dbaz_symmetry_apply).

relabel_case(R, C, max_free): late rows of 16 random games, both movers, with game_idx over the whole signed int32 range, move_idx
below 0 and with gaps, visits past 16 bits, rows without a visit on a free edge, one row that its root cannot serve, in a random
row order -- and the plan of replay_targets_ref.py for them, its facts from targets_ref.solve_rows (pure numpy).
dataset_case(R, C): about 500 synthetic rows whose positions differ in one chosen key bit or in plane 2 only, staged in two calls
and reordered, in the order oracle.train_ref.assemble_dataset expects them.  dataset_big_case(): 40 000 rows of the 1x1 board."""
import numpy as np

import endgame_ref as ER
import replay_targets_ref as RR
import targets_ref as TR
from dotsboxesaz_amd.self_play import row_bytes
from test_hip_deep_endgame import other_mover, random_games

# (R, C, max_free) of test_hip_replay_targets_boards.py: one case per row layout, not per size
RELABEL_CASES = [(3, 3, 12), (2, 7, 12), (6, 6, 12), (6, 6, 18), (8, 8, 12), (8, 8, 18), (10, 10, 12), (15, 7, 12), (1, 1, 4)]
# boards of test_hip_train_data_boards.py: one per key layout, lanes-per-value class and padding of csrc/replay.hip
DATASET_BOARDS = [(1, 1), (2, 4), (3, 5), (4, 5), (6, 7), (5, 9), (7, 7), (8, 8), (10, 10), (15, 7)]

# the 16 games' game_idx: both ends of int32, both sides of 0 and of 2^16, in no order
GAME_IDX = [65536, -2 ** 31, 7, -3, 2 ** 31 - 1, 0, -65537, 65535, -1, 2 ** 31 - 2, -2 ** 31 + 1, 1, -65536, 2 ** 24, 65537, -40000]
SHIFTED_GAME, GAPPED_GAME, FOREIGN_GAME = 3, 9, 5   # move_idx from below 0; move_idx with gaps; the game of the unserved row
PLANE2 = (-32768, -1, 0, 1, 32767)
# (visits on slot 0, visits of the row) of one position's eight rows in dataset order: thirds, elevenths and the like next to odd
# multiples of 2^-24, found by search so that the float32 mean of slot 0 is 0.37501112 when the Kahan sum runs in this order and
# 0.37501115 when it runs in the reverse order -- every other group's mean is the same in any order
TUNED, TUNED_VISITS = 1, [(5, 19), (6, 11), (14, 19), (5, 11), (16, 17), (921, 2 ** 24), (1, 17), (573, 2 ** 24)]

_relabel, _facts, _dataset = {}, {}, {}


def dims(R, C):
    HW = (R + 1) * (C + 1)
    return HW, 3 * HW, 2 * HW  # HW, F (values of x), A


def facts_for(R, C, max_free):
    """replay_targets_ref.plan's facts_for from the numpy solver alone; a position is solved once"""
    memo = _facts.setdefault((R, C, max_free), {})

    def facts(root, xs):
        new = [x for x in xs if x.tobytes() not in memo]
        for x, f in [] if not new else zip(new, TR.solve_rows(R, C, np.array(new, np.int16).reshape(len(new), -1), max_free)):
            memo[x.tobytes()] = f
        return [memo[x.tobytes()] for x in xs]
    return facts


def relabel_case(R, C, max_free):
    """dict(packed uint8 [n, row_bytes], plan: replay_targets_ref.plan of them, foreign: the index of the unserved row or None,
    facts_for, E), built once per case and left unchanged"""
    key = (R, C, max_free)
    if key in _relabel:
        return _relabel[key]
    HW, F, A = dims(R, C)
    acts = np.array(ER.board(R, C)[0])
    E = len(acts)
    xs, left = random_games(R, C, 8, seed=100 * R + C)
    per = len(xs) // 8
    rs = np.random.RandomState(1000 * R + 10 * C + max_free)
    game, move, x = [], [], []
    for g in range(16):
        gx, gl = xs[(g % 8) * per:(g % 8 + 1) * per], left[(g % 8) * per:(g % 8 + 1) * per]
        if g >= 8:
            gx = other_mover(R, C, gx)
        keep = np.nonzero(gl <= max_free + 3)[0]  # row k of a game is its position after k moves
        ply = keep.astype(np.int64)
        if g == SHIFTED_GAME:
            ply = ply - (int(keep[gl[keep] <= max_free][0]) + 2)  # the root at -2, the rows before it further below 0
        if g == GAPPED_GAME:
            ply = 3 * ply + 7 + ply % 2  # steps of 4 and 2
        game += [GAME_IDX[g]] * len(keep)
        move += ply.tolist()
        x.append(gx[keep])
    game, move, x = np.array(game, np.int64), np.array(move, np.int64), np.concatenate(x).astype(np.int16)
    n = len(x)
    assert move.min() < 0 and np.abs(move).max() < 2 ** 15
    free = np.zeros((n, A), bool)
    free[:, acts] = x[:, acts] == 0     # the free real edges
    n_free = free.sum(axis=1)
    # one candidate row after its game's root gets the position of another game with as many free edges: not a subset of its
    # root's free edges, unless the root has every edge free (a board with E <= max_free)
    foreign = None
    mine = np.nonzero(game == GAME_IDX[FOREIGN_GAME])[0]
    root = mine[n_free[mine] <= max_free][0]
    for victim in mine[n_free[mine] <= max_free][2:]:
        donors = [d for d in np.nonzero((n_free == n_free[victim]) & (game != game[victim]))[0] if (free[d] & ~free[root]).any()]
        if donors:
            foreign = int(victim)
            x[victim] = x[donors[0]]
            free[victim] = free[donors[0]]
            break
    visits = rs.randint(0, 50, (n, A)).astype(np.int32)
    for r in range(0, n, 5):  # values whose high half is not 0; 31 of them still sum inside int32
        at = np.nonzero(free[r])[0]
        at = at[rs.rand(len(at)) < 0.6]
        visits[r, at] = rs.randint(65536, 2 ** 24, len(at))
    for r in range(0, n, 7):  # nothing on a free edge, something on every other slot
        visits[r] = np.where(free[r], 0, rs.randint(1, 50, A))
    z = rs.randint(-1, 2, n).astype(np.int8)
    perm = rs.permutation(n)
    packed = RR.pack(R, C, game[perm], move[perm], x[perm], visits[perm], z[perm], seed=R + C + max_free)
    if foreign is not None:
        foreign = int(np.nonzero(perm == foreign)[0][0])
    ff = facts_for(R, C, max_free)
    out = dict(packed=packed, plan=RR.plan(R, C, packed, max_free, ff), foreign=foreign, facts_for=ff, E=E)
    _relabel[key] = out
    return out


# ---------------------------------------------------------------- the dataset kernels' rows
def key_words(R, C, x):
    """The sort key of csrc/replay.hip restated: bit b of [x_0 .. x_{A-1} | the 16 bits of x_A + 32768], most significant first,
    64 bits per word: uint64 [n, KW]"""
    HW, F, A = dims(R, C)
    KW = (A + 16 + 63) // 64
    x = np.asarray(x).reshape(-1, F)
    bits = np.zeros((len(x), 64 * KW), np.uint64)
    bits[:, :A] = (x[:, :A] & 1).astype(np.uint64)
    v16 = x[:, A].astype(np.int64) + 32768
    for b in range(16):
        bits[:, A + b] = ((v16 >> (15 - b)) & 1).astype(np.uint64)
    w = np.uint64(1) << np.arange(63, -1, -1, dtype=np.uint64)
    return (bits.reshape(len(x), KW, 64) * w).sum(axis=2, dtype=np.uint64)


def _row(edges, plane2, HW):
    return np.concatenate([edges, np.full(HW, plane2, np.int64)]).astype(np.int16)


def _visits(rs, n, A):
    """int32 [n, A]: small counts, of very different sizes from row to row, every third row with a few past 16 bits; no row sums to 0"""
    v = rs.randint(0, 50, (n, A)).astype(np.int64)
    v *= rs.choice([1, 1, 3, 7, 101], size=(n, 1))
    v[rs.rand(n, A) < 0.3] = 0
    for r in range(0, n, 3):
        at = rs.choice(A, size=min(A, 6), replace=False)
        v[r, at] = rs.randint(65536, 2 ** 24, len(at))
    v[v.sum(axis=1) == 0, 0] = 1
    assert v.sum(axis=1).max() < 2 ** 31
    return v.astype(np.int32)


def dataset_case(R, C):
    """dict(x, visits, z: the rows in dataset order, so that assemble_dataset(x, visits, z, avg) is the expected dataset;
    rows_a, sel: the first dataset_add_rows call (a pool of packed rows and the indices staged from it), rows_b: the second
    call (no sel), order: dataset_finish's permutation (dataset row k is staged row order[k]); staged: the packed rows in
    staging order; positions int16 [P, F]: the distinct positions, positions[0] the base of the near-duplicates; row_bytes, KW)"""
    if (R, C) in _dataset:
        return _dataset[(R, C)]
    HW, F, A = dims(R, C)
    KW = (A + 16 + 63) // 64
    rs = np.random.RandomState(7000 + 100 * R + C)
    base = rs.randint(0, 2, A)
    pos = [_row(base, 7, HW)]
    for w in range(KW):  # one bit at either end of every key word that holds edge bits
        for slot in {64 * w, min(64 * w + 63, A - 1)}:
            if slot < A:
                e = base.copy()
                e[slot] ^= 1
                pos.append(_row(e, 7, HW))
    pos += [_row(base, p2, HW) for p2 in PLANE2]
    while len(pos) < min(96, 2 ** A - 8):
        pos.append(_row(rs.randint(0, 2, A), int(rs.choice(PLANE2 + (7, 300, -300))), HW))
    pos = np.unique(np.array(pos, np.int16), axis=0)
    pos = np.concatenate([[_row(base, 7, HW)], pos[(pos != _row(base, 7, HW)).any(axis=1)]])
    times = rs.randint(1, 10, len(pos))
    times[:8] = np.maximum(times[:8], 5)
    times[TUNED] = len(TUNED_VISITS)
    which = rs.permutation(np.repeat(np.arange(len(pos)), times))  # staging order: every position scattered through it
    n0, n1 = len(which), len(which) // 2
    sx, sv, sz = pos[which], _visits(rs, n0, A), rs.randint(-1, 2, n0).astype(np.int8)
    # the first call stages rows 0 .. n1 - 1, the second the rest and, among them, ten rows the first has staged already: two rows
    again = [int(np.nonzero((which[:n1] == p))[0][0]) for p in rs.permutation(np.nonzero(times <= 8)[0]) if p != TUNED and (which[:n1] == p).any()][:10]
    second = np.concatenate([np.arange(n1, n0), again])[rs.permutation(n0 - n1 + len(again))]
    take = np.concatenate([np.arange(n1), second])
    sx, sv, sz = sx[take], sv[take], sz[take]
    n = len(take)
    order = rs.permutation(n).astype(np.int32)             # dataset row k is staged row order[k]
    for j, k in enumerate(np.nonzero(which[take][order] == TUNED)[0]):  # the tuned group, in dataset order
        sv[order[k]] = 0
        sv[order[k], :2] = TUNED_VISITS[j][0], TUNED_VISITS[j][1] - TUNED_VISITS[j][0]
    x, visits, z = sx[order], sv[order], sz[order]
    staged = RR.pack(R, C, rs.randint(-9, 9, n), rs.randint(-9, 9, n), sx, sv, sz, seed=R * C)
    pool_at = rs.permutation(n1 + 40)                      # the first call's pool: its rows shuffled among 40 that no call stages
    rows_a = RR.pack(R, C, 0, 0, pos[rs.randint(0, len(pos), n1 + 40)], _visits(rs, n1 + 40, A), 1, seed=1)
    rows_a[pool_at[:n1]] = staged[:n1]
    out = dict(x=x, visits=visits, z=z, rows_a=rows_a, sel=pool_at[:n1].astype(np.int32), rows_b=staged[n1:].copy(), order=order,
               staged=staged, staged_fields=(sx, sv, sz), positions=pos, row_bytes=row_bytes(F, A), KW=KW)
    _dataset[(R, C)] = out
    return out


def dataset_big_case(n=40000):
    """(packed rows, x, visits, z) of the 1x1 board, 88 bytes a row: more rows than one round of k_ds_stage's and k_make_batch's
    block-uniform loops takes (32 768)"""
    if "big" not in _dataset:
        HW, F, A = dims(1, 1)
        rs = np.random.RandomState(11)
        x = np.concatenate([rs.randint(0, 2, (n, A)), np.repeat(rs.choice(PLANE2, n)[:, None], HW, axis=1)], axis=1).astype(np.int16)
        visits, z = _visits(rs, n, A), rs.randint(-1, 2, n).astype(np.int8)
        _dataset["big"] = (RR.pack(1, 1, 0, 0, x, visits, z, seed=5), x, visits, z)
    return _dataset["big"]
