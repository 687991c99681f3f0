"""tests/playout_cap_ref.py, the CPU restatement of self-play under a playout cap, checked on its own (no GPU): with the cap off
it is the oracle's play_game row for row, the rule's reads and noise reach the searches, and three deliberate mistakes -- noise
kept on the fast searches, the fast budget not applied, the ply counted from the empty board under a start position -- each change
the rows of most games, so that a device test that compares with this replay would see them."""
import numpy as np
import pytest

from oracle import oracle as O
import playout_cap_ref as PR

SIMS, FAST, P = 40, 6, 0.25
NOISE = (0.8, 0.25)
START = (0, 5, 9)  # three plies of a 3x3 game: the ply of the rule counts from here


def gen(R, C, seed, game, *, cap, noise=NOISE, start=(), mistake=None, reuse=True):
    d = O.dims(R, C)
    return PR.generate_game(d, np.random.RandomState(1000 * seed + game), seed=seed, game_idx=game, sims=SIMS, reuse=reuse, noise=noise,
                            cap=cap, start=start, mistake=mistake)


@pytest.mark.parametrize("R,C,noise,reuse", [(3, 3, (0.0, 0.0), True), (3, 3, NOISE, True), (2, 7, NOISE, False)])
def test_cap_off_is_the_oracles_play_game(R, C, noise, reuse):
    d = O.dims(R, C)
    for game in range(3):
        ref = gen(R, C, 7, game, cap=None, noise=noise, reuse=reuse)
        vecs = iter(ref["vectors"]) if noise[0] > 0 else None
        pp = O.selfplay_params(SIMS, noise=noise, reuse_tree=reuse)
        want = O.play_game(d, pp, O.Evaluator(0), forced_moves=ref["played"], noise=(lambda n, alpha: next(vecs)) if vecs else None)
        assert want["n_rows"] == ref["n_rows"] and want["n_search"] == ref["n_search"]
        assert PR.rows_differ(ref, want) == -1
        assert ref["full"].all() and PR.rows_differ(gen(R, C, 7, game, cap=(1.0, FAST), noise=noise, reuse=reuse), want) == -1


def test_reads_and_kinds_follow_the_rule():
    d = O.dims(3, 3)
    g = gen(3, 3, 7, 5, cap=(P, FAST))
    want_full = np.array([PR.is_full(7, 5, i, P) for i in range(g["n_rows"])])
    assert np.array_equal(g["full"], want_full) and want_full.any() and not want_full.all()
    assert (g["reads"][~want_full] <= FAST).all() and (g["visits"].sum(axis=1) >= g["reads"]).all()
    early_full = want_full & (np.arange(g["n_rows"]) < 12)  # 4 * F! >= 40 while at least 3 edges are free
    assert (g["reads"][early_full] == SIMS).all()
    # the replay of a generated game is that game
    again = PR.replay_game(d, g["played"], g["vectors"], seed=7, game_idx=5, sims=SIMS, reuse=True, noise=NOISE, cap=(P, FAST))
    assert PR.rows_differ(again, g) == -1 and np.array_equal(again["reads"], g["reads"])
    # all fast, noise configured: the game of an engine with mcts_num_read = fast_reads and no noise
    allfast = PR.replay_game(d, g["played"], g["vectors"], seed=7, game_idx=5, sims=SIMS, reuse=True, noise=NOISE, cap=(0.0, FAST))
    plain = PR.replay_game(d, g["played"], None, seed=7, game_idx=5, sims=FAST, reuse=True, noise=(0.0, 0.0), cap=None)
    assert not allfast["full"].any() and PR.rows_differ(allfast, plain) == -1


@pytest.mark.parametrize("mistake", PR.MISTAKES)
def test_a_deliberate_mistake_changes_most_games(mistake):
    """8 generated 3x3 games (seed 7, games 0..7), replayed with the mistake: at least 6 must differ from the right replay"""
    d = O.dims(3, 3)
    start = START if mistake == "ply_from_empty_board" else ()
    changed = 0
    for game in range(8):
        g = gen(3, 3, 7, game, cap=(P, FAST), start=start)
        kw = dict(seed=7, game_idx=game, sims=SIMS, reuse=True, noise=NOISE, cap=(P, FAST), start=start)
        assert PR.rows_differ(PR.replay_game(d, g["played"], g["vectors"], **kw), g) == -1
        wrong = PR.replay_game(d, g["played"], g["vectors"], mistake=mistake, **kw)
        changed += PR.rows_differ(wrong, g) >= 0
    print("%s: %d of 8 games differ" % (mistake, changed))
    assert changed >= 6
