"""The solved table as an evaluator (DBAZ_EVAL_SOLVER, dbaz_attach_solver, dbaz_perfect_policy): the ABI additions, and the
condition under which a one-hot perfect prior plays perfectly through the search -- checked with the oracle's search and
play_game under the numpy restatement of the evaluator (tests/solver_ref.py).  Runs without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from oracle import oracle as O
from dotsboxesaz_amd import _lib
import solver_ref as SR

# the policy entry point takes a dbaz_solver handle but is not named dbaz_solver_*: tests/test_solver_abi.py pins that family
NEW = ("dbaz_attach_solver", "dbaz_perfect_policy")


def test_abi_additions():
    assert _lib.EVAL_SOLVER == 5 and _lib.EVAL_EXTERNAL == 4
    src = open(os.path.join(REPO, "include", "dbaz.h")).read()
    assert re.search(r"#define\s+DBAZ_EVAL_SOLVER\s+5\b", src) and re.search(r"#define\s+DBAZ_ABI_VERSION\s+3\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        from dotsboxesaz_amd import build
        build.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert _lib.load().dbaz_version() == 3
    from dotsboxesaz_amd.engine import Engine
    assert Engine.EVALUATORS["solver"] == 5


def test_mix_is_the_splitmix64_finaliser():
    # splitmix64's first outputs for state 0 are finalise(k * golden ratio), k = 1, 2 (Steele, Lea, Flood 2014; Vigna's
    # splitmix64.c): mix(0, k) is exactly that
    assert SR.mix(0, 1) == 0xE220A8397B1DCDAF and SR.mix(0, 2) == 0x6E789E6AA1B965F4
    assert SR.mix(5, 0) == SR.mix(5, 0) != SR.mix(4, 0)


def test_table_restatement():
    assert [int(SR.table(r, c)[0]) for r, c in ((1, 1), (1, 2), (2, 2), (2, 3))] == [-1, 0, 2, -2]  # values tests/test_hip_solver.py pins


READS = (1, 2, 3, 5, 8, 13, 50, 200)
GAMES = 30


def random_unfinished_start(d, rs, E):
    while True:
        s = O.new_state(d)
        moves = []
        for _ in range(int(rs.randint(0, E))):
            valid = np.nonzero(O.valid_moves(d, s))[0]
            m = int(valid[rs.randint(len(valid))])
            t = s.copy()
            O.play_(d, t, m)
            if O.get_result(t) is not None:
                break
            s = t
            moves.append(m)
        return s


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("R,C", [(2, 2), (2, 3)])
def test_one_hot_prior_plays_perfectly_through_the_search(R, C, seed):
    """Both sides served by the table's evaluator, any read count, move sampled at temperature 1 from the visits, every move
    searched from a fresh root (match play's configuration, self_play.py:230 -- a re-rooted tree restarts the root's visit
    count at 0, so the first read of a move would see no exploration term and take the first legal move): the game ends with
    the theoretical result of its start, and wherever the mover is not lost no visit leaves the prior's move."""
    d = O.dims(R, C)
    D = SR.table(R, C)
    E = 2 * R * C + R + C
    ev = O.Evaluator(lambda dd, s: tuple(a[0] for a in SR.policy_ref(D, R, C, O.features(dd, s).ravel()[None], seed)))
    rs = np.random.RandomState(1000 * R + 10 * C + seed)
    n_roots = n_safe = 0
    for reads in READS:
        pp = O.selfplay_params(reads, noise=(0.0, 0.0), reuse_tree=False, temperature={0: 1.0})
        for g in range(GAMES):
            start = random_unfinished_start(d, rs, E)
            _, v0 = SR.policy_one(D, R, C, O.features(d, start).ravel(), seed)
            got = O.play_game(d, pp, ev, start=start, rng_state=int(rs.randint(1, 2 ** 31)))
            assert got["n_rows"] >= 1 and got["player"][0] == start.to_play
            assert int(got["z"][0]) == int(v0), (reads, g, int(got["z"][0]), v0)
            for r in range(got["n_rows"]):
                a, v = SR.policy_one(D, R, C, got["x"][r], seed)
                if a < 0:
                    continue  # the closing row of the game
                n_roots += 1
                if v >= 0:
                    n_safe += 1
                    others = np.delete(got["visits"][r], a)
                    assert not others.any(), (reads, g, r, a, got["visits"][r])
                # z of every row is the true value of its position: the result never changes hands
                assert int(got["z"][r]) == int(v), (reads, g, r)
    assert n_roots > 1000 and n_safe > 300
