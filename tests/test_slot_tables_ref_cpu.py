"""The numpy restatement of the search's table evaluator (slot_tables_ref.py) against endgame_policy_ref.policy, which solves every
row from scratch: descendants with F <= 12 of 3x3 and 4x4 roots with F = 14 (runs without a GPU)."""
import numpy as np
import pytest

import endgame_policy_ref as PR
import endgame_ref as ER
from slot_tables_ref import SlotTablesRef


def games_from(R, C, f0, seed):
    """two random games: (their rows with F = f0 -- the roots --, their later rows with F <= 12 and the same with the other mover)"""
    x, left = PR.random_games(R, C, 2, seed=seed)
    per_game = len(x) // 2
    game = np.arange(len(x)) // per_game
    roots = x[left == f0]
    late = x[left <= 12]
    assert len(roots) == 2 and set(game[left <= 12]) == {0, 1}
    return roots, np.concatenate([late, PR.other_mover(R, C, late)])


@pytest.mark.parametrize("R,C", [(3, 3), (4, 4)])
@pytest.mark.parametrize("seed", [0, 7])
def test_lookup_equals_the_solve_from_scratch(R, C, seed):
    roots, rows = games_from(R, C, 14, 10 * R + C)
    ref = SlotTablesRef(R, C, roots, seed, max_free=14)
    assert len(ref.roots) == 2 and all(len(r["free"]) == 14 for r in ref.roots)
    p, v, served = ref.policy(rows)
    want_p, want_v, want_s = PR.policy(R, C, rows, seed, 12)
    assert served.all() and want_s.all()
    assert np.array_equal(p, want_p) and np.array_equal(v, want_v)
    assert (p.sum(axis=1) == 1).any() and (p.sum(axis=1) == 0).any() and set(v) >= {-1.0, 1.0}
    # the roots themselves, and the table's first entry
    rp, rv, rs = ref.policy(roots)
    wp, wv, _ = PR.policy(R, C, roots, seed, 14)
    assert rs.all() and np.array_equal(rp, wp) and np.array_equal(rv, wv)
    assert ref.table(0).dtype == np.int8 and ref.table(0).shape == (1 << 14,) and ref.table(0)[-1] == 0


def test_rows_no_start_serves_and_starts_above_max_free():
    R, C = 3, 3
    roots, rows = games_from(R, C, 14, 33)
    ref = SlotTablesRef(R, C, roots[:1], 0, max_free=14)
    acts, _ = ER.board(R, C)
    free0 = set(a for a in acts if roots[0][a] == 0)
    inside = np.array([set(a for a in acts if r[a] == 0) <= free0 for r in rows])
    p, v, served = ref.policy(rows)
    assert np.array_equal(served, inside) and inside.any() and (~inside).any()
    assert not p[~served].any() and not v[~served].any()
    want_p, want_v, _ = PR.policy(R, C, rows[inside], 0, 12)
    assert np.array_equal(p[inside], want_p) and np.array_equal(v[inside], want_v)
    with pytest.raises(AssertionError):
        ref.evaluator()(rows)
    assert np.array_equal(ref.evaluator(strict=False)(rows)[0], p)
    assert SlotTablesRef(R, C, roots, 0, max_free=13).roots == []  # a start with F > max_free gets no table


def test_which_superset_start_answers_does_not_matter():
    R, C = 3, 3
    x, left = PR.random_games(R, C, 1, seed=5)
    a = SlotTablesRef(R, C, x[left == 14], 7, max_free=14)
    b = SlotTablesRef(R, C, x[left == 12], 7, max_free=14)
    rows = x[left <= 12]
    for got, want in zip(a.policy(rows), b.policy(rows)):
        assert np.array_equal(got, want)
