"""Oracle play_game(start=...) vs the reference's SelfPlay.play_games(game_state, idxs) from start positions that are not the
empty board (self_play.py:51-55,76-80; tests/golden/selfplay_start.npz), and the game -> start mapping of an opening book."""
import numpy as np
import pytest

from oracle import oracle as O
from conftest import load_golden
from test_oracle_selfplay import check_rows, golden_games, match_games, params_of

_G = load_golden("selfplay_start.npz")
CASES = [str(c) for c in _G["cases"]]
MATCH_CASES = [str(c) for c in _G["match_cases"]]


def literal_start(gi, n_starts, gps):
    """The mapping written out (dbaz_selfplay_set_start's header comment)."""
    return (gi // gps) % n_starts


def starts_of(g, name):
    """(list of start move sequences, games_per_start) of a fixture case"""
    mv, off = g[name + "_start_moves"], g[name + "_start_offsets"]
    return [mv[off[s]:off[s + 1]] for s in range(len(off) - 1)], int(g[name + "_games_per_start"])


def start_states(g, name, d, n_games):
    starts, gps = starts_of(g, name)
    return [O.state_from_moves(d, starts[literal_start(gi, len(starts), gps)]) for gi in range(n_games)]


def evaluator_of(name):
    return O.Evaluator(1 if name == "st33_uniform" else 0)


@pytest.mark.parametrize("name", CASES)
def test_teacher_forced_from_start(name):
    g = _G
    d, pp = params_of(g, name)
    ev = evaluator_of(name)
    games = golden_games(g, name)
    for gg, st in zip(games, start_states(g, name, d, len(games))):
        it = iter(gg["noise"]) if gg["noise"] is not None else None
        got = O.play_game(d, pp, ev, start=st, forced_moves=gg["moves"], noise=(lambda n, a: next(it)) if it is not None else None)
        assert np.array_equal(got["played"], gg["moves"])
        check_rows(g, name, gg, got)  # incl. move_idx == 0..n-1 from the start position
        assert got["move"][0] == -1 and np.array_equal(got["x"][0], O.features(d, st).ravel())


@pytest.mark.parametrize("name", CASES)
def test_seed_only_from_start(name):
    g = _G
    d, pp = params_of(g, name)
    ev = evaluator_of(name)
    np.random.seed(int(g[name + "_cfg"][7]))
    games = golden_games(g, name)
    for gg, st in zip(games, start_states(g, name, d, len(games))):
        got = O.play_game(d, pp, ev, start=st, choice=lambda p: np.random.choice(p.shape[0], 1, p=p)[0],
                          noise=lambda n, a: np.random.dirichlet(np.full(n, a), 1).ravel())
        assert np.array_equal(got["played"], gg["moves"])
        check_rows(g, name, gg, got)


def test_fixture_start_properties():
    """What the cases were chosen for."""
    g = _G
    d = O.dims(3, 3)
    (mid,), _ = starts_of(g, "st33_mid")
    s = O.state_from_moves(d, mid)
    assert len(mid) == 7 and list(s.b2c2) == [9, 9]  # no box closed yet
    (late,), _ = starts_of(g, "st33_late")
    s = O.state_from_moves(d, late)
    assert len(late) >= 14 and s.just_played == s.to_play == 0 and O.get_result(s) is None
    book, gps = starts_of(g, "st23_book")
    assert [len(b) for b in book] == [0, 3, 6] and gps == 2 and int(g["st23_book_cfg"][6]) == 7
    (m66,), _ = starts_of(g, "st66_mid")
    assert len(m66) == 40
    (uni,), _ = starts_of(g, "st33_uniform")
    assert len(uni) == 10


@pytest.mark.parametrize("name", MATCH_CASES)
def test_match_play_oracle_from_book(name):
    g = _G
    rows, cols, sims, n_games, _seed = [int(x) for x in g[name + "_cfg"]]
    d = O.dims(rows, cols)
    pp = O.selfplay_params(sims, noise=(0.0, 0.0), reuse_tree=False)
    cur = {"model": 0, "game": 0}
    ev = O.Evaluator(lambda dd, s: O.eval_formula(dd, s, 0 if cur["model"] == 0 else 1))
    assert "x_0" not in list(g[name + "_columns"])
    starts, gps = starts_of(g, name)
    assert len(starts) == 2 and gps == 2
    for gi, gg in enumerate(match_games(g, name)):
        cur["game"] = gi
        st = O.state_from_moves(d, starts[literal_start(gi, len(starts), gps)])
        got = O.play_game(d, pp, ev, start=st, forced_moves=gg["moves"],
                          on_move=lambda tp: cur.__setitem__("model", tp ^ (cur["game"] & 1)))
        r = gg["rows"]
        assert np.array_equal(got["move"], g[name + "_move"][r]) and got["move"][0] == -1
        assert np.array_equal(got["player"], g[name + "_player"][r]) and got["player"][0] == st.to_play
        assert np.array_equal(got["pi"].view(np.uint64), g[name + "_pi"][r].view(np.uint64))
        assert np.array_equal(got["z"], g[name + "_z"][r])
        assert np.array_equal(got["q_value"].view(np.uint32), g[name + "_q"][r].view(np.uint32))
        stt = np.stack([got["max_deepness"], got["tree_size"], got["terminal_count"]], axis=1)
        assert np.array_equal(stt, g[name + "_stats"][r])
        assert np.array_equal(np.arange(len(r)), g[name + "_index"][r, 2])
        assert np.array_equal(np.where(got["player"] == 0, 7, 9), g[name + "_index"][r, 0])


def test_start_index_mapping():
    from dotsboxesaz_amd.self_play import start_index
    # (game_idx, n_starts, games_per_start) -> start
    for gi, n, gps, exp in [(0, 1, 1, 0), (5, 1, 1, 0), (0, 3, 1, 0), (4, 3, 1, 1), (5, 3, 2, 2), (6, 3, 2, 0), (7, 3, 2, 0),
                            (8, 3, 2, 1), (100, 5, 1, 0), (103, 5, 1, 3), (100, 7, 3, 5), (147, 7, 3, 0), (1, 2, 2, 0), (2, 2, 2, 1),
                            (65535, 4, 1, 3), (2 ** 31 + 1, 3, 2, ((2 ** 31 + 1) // 2) % 3)]:
        assert int(start_index(gi, n, gps)) == exp == literal_start(gi, n, gps), (gi, n, gps)
    # arrays, first_game_idx > 0, wrap-around
    gi = np.arange(100, 121)
    assert np.array_equal(start_index(gi, 7, 3), [(int(x) // 3) % 7 for x in gi])
    assert list(start_index(np.arange(7), 3, 2)) == [0, 0, 1, 1, 2, 2, 0]
    assert int(start_index(4, 3)) == 1  # games_per_start defaults to 1


def test_start_moves_of_states_and_sequences():
    """SelfPlay.play_games' game_state -> move sequence, without a GPU (stand-in objects)."""
    from dotsboxesaz_amd.self_play import start_moves

    class Recorded:
        _moves, _dim = [3, 0, 7], (3, 3)

    class EdgesOnly:
        board = np.zeros((2, 4, 4), np.uint8)

    assert start_moves(None, 3, 3) == [] and start_moves(Recorded(), 3, 3) == [3, 0, 7]
    assert start_moves(np.array([1, 2], np.int16), 3, 3) == [1, 2]
    with pytest.raises(ValueError):
        start_moves(Recorded(), 2, 3)
    e = EdgesOnly()
    e.board = e.board.copy()
    e.board[1, 3, :] = 1  # the sentinels of an empty board
    assert start_moves(e, 3, 3) == []
    e.board[0, 1, 1] = 255
    with pytest.raises(TypeError):
        start_moves(e, 3, 3)
