"""The leaf solver's reference (leaf_solve_ref.py) against itself, on the CPU: with L = 0 it is endgame_selfplay_ref's game loop,
the rule it states changes games, and each deliberate mistake in the rule changes at least one of 8 generated games per board --
so the GPU tests that replay the engine's games through it can tell those mistakes from the rule.  Plus the interface: the header
declares the two entry points, _lib.py binds them, the Python layer takes the keywords.

Settings as in the issue's table: formula kind 0, pick seed 3, moves sampled with RandomState(100 + g), tree reuse on.
Observed (games of 8 whose rows differ; a mistaken replay stops at the first row that differs):
  3x3, L 6, 40 reads: the rule against no rule 8; off_by_one 8, root 8, seed 7, sign 8; 559 leaves solved, every F in 1 .. 6
  4x4, L 8, 24 reads: the rule against no rule 7; off_by_one 7, root 7, seed 5, sign 7; 262 leaves solved, every F in 1 .. 8"""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
from oracle import oracle as O
import endgame_selfplay_ref as SR
import leaf_solve_ref as LR

SEED = 3
BOARDS = [(3, 3, 6, 40), (4, 4, 8, 24)]
_games = {}


def games(R, C, L, sims):
    """8 games generated with the rule, and the wrapper that played them"""
    if (R, C) not in _games:
        d = O.dims(R, C)
        w = LR.LeafSolver(R, C, L, SEED, 0)
        _games[(R, C)] = ([LR.generate(d, np.random.RandomState(100 + g), w, sims=sims, reuse=True) for g in range(8)], w)
    return _games[(R, C)]


def same(a, b):
    return a["mismatch"] < 0 and b["mismatch"] < 0 and SR.rows_differ(a, b) < 0 and np.array_equal(a["played"], b["played"])


@pytest.mark.parametrize("R,C,L,sims", BOARDS)
def test_without_a_threshold_the_wrapper_is_the_plain_game_loop(R, C, L, sims):
    d = O.dims(R, C)
    for g in range(3):
        w = LR.LeafSolver(R, C, 0, SEED, 0)
        a = LR.generate(d, np.random.RandomState(100 + g), w, sims=sims, reuse=True)
        b = SR.generate_game(d, np.random.RandomState(100 + g), 0, None, sims=sims, reuse=True)
        assert same(a, b) and w.calls == {"base": b["base_calls"], "solved": 0} and a["base_calls"] == b["base_calls"]
        # and replayed through the unchanged replay_game, the wrapper passed as its base evaluator
        w2 = LR.LeafSolver(R, C, 0, SEED, 0)
        w2.start_game(d)
        c = SR.replay_game(d, dict(b, game_idx=np.zeros(b["n_rows"], np.int64)), w2.evaluate, None, sims=sims, reuse=True)
        assert same(c, b)


@pytest.mark.parametrize("R,C,L,sims", BOARDS)
def test_the_rule_and_every_deliberate_mistake_change_games(R, C, L, sims):
    d = O.dims(R, C)
    played, w = games(R, C, L, sims)
    assert sum(w.by_free) == w.calls["solved"] > 0 and all(w.by_free[f] > 0 for f in range(1, L + 1)) and not any(w.by_free[L + 1:])
    high = w.solved_under_high_roots()
    assert len(high) == 8 and sum(1 for h in high if h > 0) >= 2  # leaves solved under roots the table attach would not serve
    changed = {}
    # the rule itself: a replay without it differs, first at a row whose root has F > L
    n = 0
    for g in played:
        r = SR.replay_game(d, g, 0, None, sims=sims, reuse=True, stop_at_mismatch=True)
        if r["mismatch"] >= 0:
            n += 1
            assert g["n_free"][r["mismatch"]] > L
    changed["none"] = n
    for mistake in LR.MISTAKES:
        n = 0
        for g in played:
            wm = LR.LeafSolver(R, C, L, SEED, 0, mistake=mistake)
            r = LR.replay(d, g, wm, sims=sims, reuse=True, stop_at_mismatch=True)
            n += r["mismatch"] >= 0 or SR.rows_differ(r, g) >= 0
        changed[mistake] = n
    print("%dx%d L %d: games of 8 changed: %s; %d leaves solved, by F %s" % (R, C, L, changed, w.calls["solved"], w.by_free[:L + 1]))
    assert all(v >= 1 for v in changed.values()), changed
    # the right rule replays every game
    for g in played:
        wr = LR.LeafSolver(R, C, L, SEED, 0)
        assert same(LR.replay(d, g, wr, sims=sims, reuse=True, stop_at_mismatch=True), g)


def test_match_play_chooses_the_evaluator_per_move():
    """the solver on model 1 only: the searches of model 0 solve nothing, and swapping the seats (an odd game) swaps the searches"""
    R, C, L, sims = 3, 3, 6, 40
    d = O.dims(R, C)
    for gi in (0, 1):
        w = LR.LeafSolver(R, C, L, SEED, (1, 0), match=True, leaf_models=(1,))
        g = LR.generate(d, np.random.RandomState(7), w, sims=sims, reuse=False, game_idx=gi)
        rows = w.games[-1]
        assert len(rows["solved"]) == g["n_rows"] and w.calls["solved"] > 0
        for i in range(g["n_rows"]):
            model = (int(g["player"][i]) ^ gi) & 1
            assert model == 1 or rows["solved"][i] == 0, (gi, i)
        assert any(rows["solved"][i] > 0 for i in range(g["n_rows"]) if (int(g["player"][i]) ^ gi) & 1)


def test_the_entry_points_are_bound_and_the_python_interface_takes_the_leaf_solver():
    from dotsboxesaz_amd import _lib, self_play
    from dotsboxesaz_amd import coach
    from dotsboxesaz_amd import endgame as E
    from dotsboxesaz_amd.engine import Engine
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dbaz.h")).read(), flags=re.S)
    L = _lib.load()
    for name, count in dict(dbaz_attach_leaf_solver=5, dbaz_get_leaf_solves=2).items():
        assert name in _lib.SYMBOLS and len(getattr(L, name).argtypes) == count
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == count, (name, decl)
    assert _lib.ABI_VERSION == 3  # symbols were added, nothing else changed
    params = inspect.signature(Engine.__init__).parameters
    assert all(k in params for k in ("leaf_endgame", "leaf_free", "leaf_models"))
    assert list(inspect.signature(Engine.attach_leaf_solver).parameters)[1:] == ["endgame", "leaf_free", "model", "seed"]
    assert hasattr(Engine, "leaf_solves")
    for fn in (self_play.generate_games, self_play.compute_elo, self_play.SelfPlay.__init__, coach.Coach.__init__):
        assert "leaf_endgame" in inspect.signature(fn).parameters and "leaf_free" in inspect.signature(fn).parameters
    assert "--leaf-free" in inspect.getsource(E.main)
