"""The endgame solver as an evaluator (include/dbaz.h dbaz_exact_policy, Endgame.policy): the binding, and the numpy restatement
(endgame_policy_ref.py) against the solved table's evaluator (solver_ref.policy_ref) on boards the table reaches.  Runs without a
GPU."""
import ctypes
import os
import re

import numpy as np

from conftest import REPO
from oracle import oracle as O
from dotsboxesaz_amd import _lib
import endgame_policy_ref as PR
import endgame_ref as ER
import solver_ref as SR

SEEDS = (0, 1, 7)
_cases = {}


def case(R, C):
    """(rows with F <= 16, their F) of the board's random games, built once: 20 games on 3x3, 8 on 2x3 (E = 17: all but the
    empty board)"""
    if (R, C) not in _cases:
        x, left = PR.random_games(R, C, 20 if (R, C) == (3, 3) else 8, seed=10 * R + C)
        _cases[(R, C)] = (x[left <= 16], left[left <= 16])
    return _cases[(R, C)]


def test_binding_and_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dbaz.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+dbaz_exact_policy\s*\(\s*dbaz_endgame\s*\*", src)
    assert "dbaz_exact_policy" in _lib.SYMBOLS
    L = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dbaz_exact_policy")
    assert len(L.dbaz_exact_policy.argtypes) == 8 and L.dbaz_exact_policy.argtypes[3] is ctypes.c_uint64
    assert re.search(r"\bint\s+dbaz_exact_policy_from\s*\(\s*dbaz_endgame\s*\*", src) and "dbaz_exact_policy_from" in _lib.SYMBOLS
    assert len(L.dbaz_exact_policy_from.argtypes) == 10 and L.dbaz_exact_policy_from.argtypes[5] is ctypes.c_uint64
    from dotsboxesaz_amd.endgame import Endgame
    assert callable(Endgame.policy) and callable(Endgame.policy_from)


def test_restated_rows_equal_endgame_ref():
    """the helper's faster subgame gives endgame_ref's numbers"""
    for R, C in ((3, 3), (2, 3)):
        x, left = case(R, C)
        for r in range(0, len(x), 3):
            want, got = ER.endgame_ref(R, C, x[r]), PR.solved_row(R, C, x[r])
            assert np.array_equal(got["q"], want["q"]) and all(got[k] == want[k] for k in ("value", "n_free", "finished")), r


def test_seed_0_equals_the_table_evaluator():
    for R, C in ((3, 3), (2, 3)):
        x, left = case(R, C)
        assert len(x) >= (300 if R == 3 else 130) and set(left) == set(range(17))
        D = SR.table(R, C)
        want_p, want_v = SR.policy_ref(D, R, C, x, 0)
        p, v, solved = PR.policy(R, C, x, 0)
        assert solved.all() and p.dtype == np.float32 and v.dtype == np.float32
        assert np.array_equal(p, want_p) and np.array_equal(v, want_v)
        assert set(v) >= {-1.0, 1.0}
        assert ((p.sum(axis=1) == 0) & (left > 0)).any(), "no early end among the rows"


def test_seeded_picks_are_optimal_and_differ_somewhere():
    for R, C in ((3, 3), (2, 3)):
        x, left = case(R, C)
        D = SR.table(R, C)
        p0, v0, _ = PR.policy(R, C, x, 0)
        differ = 0
        for seed in SEEDS[1:]:
            p, v, solved = PR.policy(R, C, x, seed)
            assert solved.all() and np.array_equal(v, v0) and np.array_equal(p.sum(axis=1), p0.sum(axis=1))
            for r in np.nonzero(p.sum(axis=1))[0]:
                mask, _, res = SR.row_facts(R, C, x[r])
                q = SR.move_values(R, C, D, mask)
                acts = SR.geometry(R, C)[0]
                opt = [acts[e] for e in sorted(q) if q[e] == max(q.values())]
                assert res is None and opt == PR.optimal_set(R, C, x[r])
                a = int(np.argmax(p[r]))
                assert p[r, a] == 1.0 and p[r].sum() == 1.0 and a in opt
                assert a == opt[SR.mix(PR.pick_key(R, C, x[r]), seed) % len(opt)]
            differ += int((p != p0).any(axis=1).sum())
        assert differ > 0


def test_pick_depends_on_the_position_only():
    """two move orders to the same position: the same row, so the same pick; and the key never sees the drawn edges"""
    R, C = 3, 3
    d = O.dims(R, C)
    acts, _ = ER.board(R, C)
    rs = np.random.RandomState(5)
    n = 0
    while n < 6:
        moves = [int(a) for a in rs.permutation(acts)[:rs.randint(10, 16)]]
        s, t = O.new_state(d), O.new_state(d)
        for m in moves:
            O.play_(d, s, m)
        for m in moves[::-1]:
            O.play_(d, t, m)
        xs, xt = O.features(d, s).ravel(), O.features(d, t).ravel()
        if not np.array_equal(xs, xt) or O.get_result(s) is not None:
            continue  # captures fell to the other side, or the game is over
        n += 1
        for seed in SEEDS:
            assert PR.policy_one(R, C, xs, seed) == PR.policy_one(R, C, xt, seed)
        assert PR.pick_key(R, C, xs) == sum(1 << (a & 63) for a in acts if a not in moves)
    # 6x6: action indices above 63 fold onto the low bits by XOR
    x = np.ones(147, np.int16)
    x[[3, 67, 70]] = 0
    assert PR.pick_key(6, 6, x) == (1 << 6)


def test_finished_and_unsolved_rows():
    x, left = PR.random_games(3, 3, 4, seed=2)
    for max_free in (16, 8):
        for seed in SEEDS:
            p, v, solved = PR.policy(3, 3, x, seed, max_free)
            assert np.array_equal(solved, left <= max_free) and (~solved).sum() >= 30
            assert not p[~solved].any() and not v[~solved].any()
            fin = np.array([solved[r] and PR.solved_row(3, 3, x[r])["finished"] for r in range(len(x))])
            assert fin.sum() >= 4 and not p[fin].any()
            assert np.array_equal(v[fin], np.array([PR.solved_row(3, 3, x[r])["value"] for r in np.nonzero(fin)[0]], np.float32))
            assert (p[solved & ~fin].sum(axis=1) == 1).all()
