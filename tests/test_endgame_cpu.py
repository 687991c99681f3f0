"""Exact endgame solver (include/dbaz.h dbaz_endgame_*, dotsboxesaz_amd/endgame.py): argument checks that never reach the
device, the binding and the build, and the numpy yardstick (endgame_ref.py) against the rules and against the table recurrence
(runs without a GPU)."""
import os

import numpy as np
import pytest

from conftest import REPO
from oracle import oracle as O
from dotsboxesaz_amd import _lib, build
from dotsboxesaz_amd.endgame import Endgame, random_rows
import endgame_ref as ER
import solver_ref as SR


def test_bad_arguments_rejected_before_touching_the_device():
    for kw, word in ((dict(rows=6, cols=6, max_free=17), "17"), (dict(rows=6, cols=6, max_free=-1), "-1"),
                     (dict(rows=0, cols=3), "0x3"), (dict(rows=12, cols=12), "338")):
        with pytest.raises(_lib.DbazError) as ei:
            Endgame(**kw)
        assert ei.value.code == _lib.EINVAL and word in str(ei.value), kw


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        g = Endgame(6, 6)
        assert (g.max_free, g.n_edges, g.A) == (16, 84, 98) and Endgame(6, 6, max_free=0).max_free == 16
        g.close()
        return
    with pytest.raises(_lib.DbazError) as ei:
        Endgame(6, 6)
    assert ei.value.code == _lib.EDEVICE


def test_endgame_symbols_are_bound():
    names = sorted(s for s in _lib.SYMBOLS if s.startswith("dbaz_endgame_"))
    assert names == ["dbaz_endgame_create", "dbaz_endgame_destroy", "dbaz_endgame_last_error", "dbaz_endgame_score"]
    L = _lib.load()
    for n in names:
        assert getattr(L, n).argtypes is not None, n
    assert len(L.dbaz_endgame_create.argtypes) == 5 and len(L.dbaz_endgame_score.argtypes) == 10


def test_endgame_is_a_unit_outside_the_network_sources():
    """the nn= build hash (bench.py's roofline.traffic key) covers NN_SOURCES: the endgame solver must not touch them"""
    csrc = os.path.join(REPO, "dotsboxesaz_amd", "csrc")
    assert "endgame.hip" in [u for u, _ in build.UNITS]
    for f in build.NN_SOURCES:
        assert "endgame" not in open(os.path.join(csrc, f)).read().lower(), f


def test_random_rows_have_the_asked_number_of_free_edges():
    free = np.arange(40) % 17
    x = random_rows(4, 4, 40, free, seed=3)
    acts, _ = ER.board(4, 4)
    assert x.dtype == np.int16 and x.shape == (40, 75)
    assert np.array_equal((x[:, acts] == 0).sum(axis=1), free)
    assert (x[:, np.setdiff1d(np.arange(50), acts)] == 1).all()
    assert sum(not ER.endgame_ref(4, 4, r)["finished"] for r in x) >= 30


# ---------------------------------------------------------------- the reference against the rules
def negamax(d, s, memo):
    """true result for the player to move under optimal play by the oracle's rules (early end and draws included)"""
    r = O.get_result(s)
    if r is not None:
        return r
    key = (s.hash_int(), s.b2c2[0], s.b2c2[1], s.to_play)
    if key not in memo:
        best = -2
        for mv in np.nonzero(O.valid_moves(d, s))[0]:
            t = s.copy()
            O.play_(d, t, int(mv))
            v = negamax(d, t, memo)
            best = max(best, v if t.to_play == s.to_play else -v)
            if best == 1:
                break
        memo[key] = best
    return memo[key]


# uniformly random play leaves late positions that the mover nearly always wins (something is there to capture): the seeds are
# picked so that lost and drawn positions are among the 60
@pytest.mark.parametrize("R,C,seed", [(4, 4, 99), (6, 6, 264)])
def test_reference_value_equals_negamax_over_the_rules(R, C, seed):
    d = O.dims(R, C)
    E = 2 * R * C + R + C
    rs = np.random.RandomState(seed)
    memo, got, want, captures = {}, [], [], 0
    while len(want) < 60:
        s = O.new_state(d)
        left = E
        while O.get_result(s) is None:
            if left <= 9:
                captures += any(O.play_(d, s.copy(), int(mv)) for mv in np.nonzero(O.valid_moves(d, s))[0])
                r = ER.endgame_ref(R, C, O.features(d, s).ravel())
                assert r["n_free"] == left and not r["finished"]
                got.append(r["value"])
                want.append(negamax(d, s, memo))
            valid = np.nonzero(O.valid_moves(d, s))[0]
            O.play_(d, s, int(valid[rs.randint(len(valid))]))
            left -= 1
    assert set(want) == {-1, 0, 1} and captures >= 1
    assert got == want, "%d of %d positions differ" % (sum(a != b for a, b in zip(got, want)), len(want))


# ---------------------------------------------------------------- the reference against the table recurrence
def test_reference_equals_the_table_on_2x3():
    R, C = 2, 3
    D = SR.table(R, C)
    d = O.dims(R, C)
    acts, _ = SR.geometry(R, C)
    rs = np.random.RandomState(23)
    rows = finished = 0
    for _ in range(6):
        s = O.new_state(d)
        for _ply in range(len(acts) + 1):  # every row of the game, the rows after its end included
            x = O.features(d, s).ravel()
            mask, margin, res = SR.row_facts(R, C, x)
            r = ER.endgame_ref(R, C, x)
            assert r["n_free"] == len(acts) - bin(mask).count("1") and r["diff"] == int(D[mask])
            assert r["finished"] == (res is not None)
            assert r["value"] == (res if res is not None else np.sign(margin + int(D[mask])))
            want_q = np.full(d.A, -128, np.int8)
            if res is None:
                for e, v in SR.move_values(R, C, D, mask).items():
                    want_q[acts[e]] = v
            assert np.array_equal(r["q"], want_q)
            rows += 1
            finished += res is not None
            free = [a for a in acts if x[a] == 0]
            if free:
                O.play_(d, s, int(free[rs.randint(len(free))]))
    assert rows == 6 * 18 and finished >= 6
