"""HIP self-play and match play from given start positions (dbaz_selfplay_set_start: SelfPlay.play_games(game_state, idxs),
self_play.py:51-55,76-80, and opening books) vs the reference's golden games (tests/golden/selfplay_start.npz) and the oracle.
Every comparison is bit for bit."""
import asyncio
import math

import numpy as np
import pytest

from oracle import oracle as O
from conftest import load_golden
from test_oracle_selfplay import golden_games, match_games
from test_oracle_selfplay_start import literal_start, starts_of
from test_hip_selfplay import compare_rows

pytestmark = pytest.mark.gpu

_G = load_golden("selfplay_start.npz")
CASES = [str(c) for c in _G["cases"]]


def random_book(d, rs, n_starts, max_plies):
    """n_starts random legal NON-TERMINAL positions (move sequences of 1..max_plies plies) by the oracle's rules"""
    book = []
    for _ in range(n_starts):
        want = int(rs.randint(1, max_plies + 1))
        moves = []
        s = O.new_state(d)
        while len(moves) < want:
            valid = np.nonzero(O.valid_moves(d, s))[0]
            m = int(valid[rs.randint(len(valid))])
            trial = O.state_from_moves(d, moves + [m])
            if O.get_result(trial) is not None:
                break
            moves.append(m)
            s = trial
        assert O.get_result(O.state_from_moves(d, moves)) is None
        book.append(moves)
    return book


def first_rows(got):
    """{game_idx: index of its move_idx == 0 row}"""
    return {int(got["game_idx"][i]): i for i in np.nonzero(got["move_idx"] == 0)[0]}


# ---------------------------------------------------------------- 1. the reference's rows, teacher-forced
@pytest.mark.parametrize("tt", [True, "force"])
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("n_slots", [1, 4])
def test_golden_games_from_start_teacher_forced(name, n_slots, tt):
    from dotsboxesaz_amd.engine import Engine
    g = _G
    rows, cols, sims, a, c, reuse, n_games, _seed = g[name + "_cfg"]
    temp = {int(k): float(v) for k, v in g[name + "_temp"]}
    e = Engine(int(rows), int(cols), n_slots, mcts_num_read=int(sims), noise=(a, c), temperature=temp, reuse_tree=bool(reuse),
               evaluator="uniform" if name == "st33_uniform" else "formula", transposition_cache=tt)
    starts, gps = starts_of(g, name)
    games = golden_games(g, name)
    assert len(games) == int(n_games)
    e.selfplay_set_start(starts, gps)
    for gi, gg in enumerate(games):
        e.selfplay_script(gi, gg["moves"], gg["noise"])
    e.selfplay_start(len(games), 0)
    e.run()
    cnt = e.counters()
    assert cnt["games_finished"] == len(games) and cnt["error_slots"] == 0
    got = e.fetch_samples()
    all_rows = np.concatenate([gg["rows"] for gg in games])
    assert np.array_equal(got["played"], np.concatenate([gg["moves"] for gg in games]))
    compare_rows(got, all_rows, g, name)  # incl. move_idx counted from the start position
    fr = first_rows(got)
    assert sorted(fr) == list(range(len(games))) and all(got["move"][i] == -1 for i in fr.values())
    e.close()


# ---------------------------------------------------------------- 2. match play from a book
@pytest.mark.parametrize("n_slots", [1, 8])
def test_match_play_golden_from_book(n_slots):
    from dotsboxesaz_amd.engine import Engine
    from dotsboxesaz_amd.self_play import match_winners
    g = _G
    for name in [str(c) for c in g["match_cases"]]:
        rows, cols, sims, n_games, _seed = [int(x) for x in g[name + "_cfg"]]
        e = Engine(rows, cols, n_slots, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=False, evaluator="formula",
                   evaluator2="uniform", match_play=True)
        games = match_games(g, name)
        starts, gps = starts_of(g, name)
        e.selfplay_set_start(starts, gps)
        for gi, gg in enumerate(games):
            e.selfplay_script(gi, gg["moves"])
        e.selfplay_start(n_games, 0)
        e.run()
        cnt = e.counters()
        assert cnt["games_finished"] == n_games and cnt["error_slots"] == 0
        got = e.fetch_samples()
        r = np.concatenate([gg["rows"] for gg in games])
        assert np.array_equal(got["played"], np.concatenate([gg["moves"] for gg in games]))
        assert np.array_equal(got["move"], g[name + "_move"][r])
        assert np.array_equal(got["player"], g[name + "_player"][r])
        assert np.array_equal(got["pi"].view(np.uint64), g[name + "_pi"][r].view(np.uint64))
        assert np.array_equal(got["z"].astype(np.int64), g[name + "_z"][r])
        assert np.array_equal(got["q_value"].view(np.uint32), g[name + "_q"][r].view(np.uint32))
        st = np.stack([got["max_deepness"].astype(np.int32), got["tree_size"], got["terminal_count"]], axis=1)
        assert np.array_equal(st, g[name + "_stats"][r])
        assert np.array_equal(got["move_idx"], g[name + "_index"][r, 2])
        assert np.array_equal(got["game_idx"], g[name + "_index"][r, 1])
        n0, n1 = match_winners(got, (7, 9))
        exp0 = exp1 = 0
        for gi, gg in enumerate(games):
            rr = gg["rows"]
            win = rr[g[name + "_z"][rr] == 1]
            if len(win):
                model = int(g[name + "_player"][win[0]]) ^ (gi & 1)
                exp0 += model == 0
                exp1 += model == 1
        assert (n0, n1) == (exp0, exp1)
        e.close()


# ---------------------------------------------------------------- 3. production path vs oracle
@pytest.mark.parametrize("tt", [True, "force"])
@pytest.mark.parametrize("rows,cols,n_slots,n_games,sims,reuse,S,gps", [
    (3, 3, 64, 200, 40, True, 5, 1), (3, 3, 32, 70, 30, False, 1, 1), (6, 6, 48, 48, 60, True, 7, 3), (2, 3, 16, 40, 50, True, 4, 2),
    (10, 10, 6, 6, 24, True, 2, 1)])
def test_device_sampled_games_from_book_vs_oracle(rows, cols, n_slots, n_games, sims, reuse, S, gps, tt):
    """Moves sampled on the device (Philox), noise off, slots refilled, first_game_idx = 100: every game starts from
    book[start_index(game_idx)] and is replayed by the oracle from that state, teacher-forced with the device's moves."""
    from dotsboxesaz_amd.engine import Engine
    from dotsboxesaz_amd.self_play import start_index
    d = O.dims(rows, cols)
    E = 2 * rows * cols + rows + cols
    book = random_book(d, np.random.RandomState(rows * 100 + cols * 10 + S), S, (2 * E) // 3)
    e = Engine(rows, cols, n_slots, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=reuse, evaluator="formula", seed=1234,
               transposition_cache=tt)
    e.selfplay_set_start(book, gps)
    e.selfplay_start(n_games, 100)
    e.run()
    cnt = e.counters()
    assert cnt["games_finished"] == n_games and cnt["active_slots"] == 0 and cnt["error_slots"] == 0
    got = e.fetch_samples()
    assert sorted(set(got["game_idx"])) == list(range(100, 100 + n_games))
    pp = O.selfplay_params(sims, noise=(0.0, 0.0), reuse_tree=reuse)
    ev = O.Evaluator(0)
    total_search = 0
    for gi in range(100, 100 + n_games):
        si = int(start_index(gi, S, gps))
        assert si == literal_start(gi, S, gps)
        r = np.nonzero(got["game_idx"] == gi)[0]
        start = O.state_from_moves(d, book[si])
        assert np.array_equal(got["x"][r[0]], O.features(d, start).ravel()), gi
        assert got["move"][r[0]] == -1 and np.array_equal(got["move_idx"][r], np.arange(len(r)))
        ref = O.play_game(d, pp, ev, start=start, forced_moves=got["played"][r])
        total_search += ref["n_search"]
        assert ref["n_rows"] == len(r)
        assert np.array_equal(ref["move"], got["move"][r])
        assert np.array_equal(ref["player"], got["player"][r])
        assert np.array_equal(ref["x"], got["x"][r])
        assert np.array_equal(ref["visits"], got["visits"][r])
        assert np.array_equal(ref["pi"].view(np.uint64), got["pi"][r].view(np.uint64))
        assert np.array_equal(ref["z"], got["z"][r].astype(np.int64))
        assert np.array_equal(ref["q_value"].view(np.uint32), got["q_value"][r].view(np.uint32))
        assert np.array_equal(ref["tree_size"], got["tree_size"][r])
        assert np.array_equal(ref["terminal_count"], got["terminal_count"][r])
        assert np.array_equal(ref["max_deepness"], got["max_deepness"][r].astype(np.int32))
        s = O.state_from_moves(d, list(book[si]) + [int(m) for m in got["played"][r]])
        assert O.get_result(s) in (0, 1)
    assert cnt["expansions"] == total_search
    e.close()


# ---------------------------------------------------------------- 4. wave driver
def _fact_reads(n_valid, sims):
    return min(4 * math.factorial(n_valid), sims)  # self_play.py:64-65


def test_selfplay_driver_in_waves_from_book():
    """dbaz_config.selfplay_pending (every search in waves of K simulations): the games start from a 2-start book and are
    replayed move by move by the oracle's wave search from that start."""
    from dotsboxesaz_amd.engine import Engine
    rows, cols, n_slots, n_games, sims, K, reuse = 3, 3, 8, 20, 60, 8, True
    d = O.dims(rows, cols)
    book = random_book(d, np.random.RandomState(8), 2, 12)
    e = Engine(rows, cols, n_slots, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=reuse, evaluator="formula", seed=3,
               max_pending_evals=K, selfplay_pending=True)
    e.selfplay_set_start(book)
    e.selfplay_start(n_games, 0)
    e.run()
    c = e.counters()
    assert c["games_finished"] == n_games and c["error_slots"] == 0
    got = e.fetch_samples()
    e.close()
    ev = O.Evaluator(0)
    for gidx in range(n_games):
        sel = np.nonzero(got["game_idx"] == gidx)[0]
        assert list(got["move_idx"][sel]) == list(range(len(sel))) and got["move"][sel[0]] == -1
        t = O.Tree(d, O.state_from_moves(d, book[literal_start(gidx, 2, 1)]))
        for r in sel:
            st = t.state
            reads = _fact_reads(int(O.valid_moves(d, st).sum()), sims)
            vis = t.search(reads, ev, max_pending=K)
            md, ts, tc, q = t.stats()
            assert np.array_equal(got["visits"][r], vis), (gidx, r)
            assert np.array_equal(got["x"][r], O.features(d, st).ravel()), (gidx, r)
            assert (int(got["max_deepness"][r]), int(got["tree_size"][r]), int(got["terminal_count"][r])) == (md, ts, tc), (gidx, r)
            assert np.float32(got["q_value"][r]).view(np.uint32) == np.float32(q).view(np.uint32), (gidx, r)
            assert got["player"][r] == st.to_play
            s = vis.sum()
            assert np.array_equal(got["pi"][r], vis.astype(np.float64) / (s if s else 1.0))
            t.advance(int(got["played"][r]), reuse)
        assert t.is_terminal
        term = t.state
        zt = O.get_result(term)
        for r in sel:
            assert int(got["z"][r]) == (zt if got["player"][r] == term.just_played else -zt), (gidx, r)


# ---------------------------------------------------------------- 5. network evaluator
def test_resnet_selfplay_from_book_vs_oracle_fed_by_the_hip_network():
    import torch
    from oracle import nn_ref
    from dotsboxesaz_amd.engine import Engine
    rows, cols, n_slots, n_games, sims, blocks = 3, 3, 16, 32, 25, 4
    torch.manual_seed(34)
    m = nn_ref.ResNetZeroRef(rows, cols, 64, blocks)
    nn_ref.randomize_bn(m, 3)
    d = O.dims(rows, cols)
    book = random_book(d, np.random.RandomState(5), 4, 14)
    e = Engine(rows, cols, n_slots, mcts_num_read=sims, noise=(0.0, 0.0), evaluator="resnet", seed=5, nn_precision=1)
    e.load_state_dict(m.state_dict(), "resnet", 64, blocks, 16, 8)
    e.selfplay_set_start(book)
    e.selfplay_start(n_games, 0)
    e.run()
    cnt = e.counters()
    assert cnt["games_finished"] == n_games and cnt["error_slots"] == 0 and cnt["f32_fallback_evals"] == 0
    got = e.fetch_samples()
    memo = {}

    def hip_net(dd, st):
        x = O.features(dd, st)
        key = x.tobytes()
        if key not in memo:
            pv = e.predict(x.astype(np.float32).reshape(1, 3, rows + 1, cols + 1))
            memo[key] = (pv[0][0].copy(), pv[1][0].copy())
        return memo[key]

    ev = O.Evaluator(hip_net)
    pp = O.selfplay_params(sims, noise=(0.0, 0.0), reuse_tree=True)
    for gi in range(n_games):
        r = np.nonzero(got["game_idx"] == gi)[0]
        start = O.state_from_moves(d, book[literal_start(gi, 4, 1)])
        ref = O.play_game(d, pp, ev, start=start, forced_moves=got["played"][r])
        assert ref["n_rows"] == len(r)
        assert np.array_equal(ref["x"], got["x"][r]) and np.array_equal(ref["move"], got["move"][r])
        assert np.array_equal(ref["visits"], got["visits"][r]), gi
        assert np.array_equal(ref["pi"].view(np.uint64), got["pi"][r].view(np.uint64))
        assert np.array_equal(ref["q_value"].view(np.uint32), got["q_value"][r].view(np.uint32))
        assert np.array_equal(ref["tree_size"], got["tree_size"][r])
        assert np.array_equal(ref["terminal_count"], got["terminal_count"][r])
        assert np.array_equal(ref["max_deepness"], got["max_deepness"][r].astype(np.int32))
        assert np.array_equal(ref["z"], got["z"][r].astype(np.int64))
    assert e.counters()["f32_fallback_evals"] == 0
    e.close()


# ---------------------------------------------------------------- 6. shard invariance
def test_book_games_do_not_depend_on_sharding():
    """The mapping uses the absolute game index: games 0..95 on one engine equal games 0..47 and 48..95 of two engines."""
    from dotsboxesaz_amd.engine import Engine
    d = O.dims(3, 3)
    book = random_book(d, np.random.RandomState(6), 5, 12)

    def play(first, n):
        e = Engine(3, 3, 24, mcts_num_read=30, noise=(0.8, 0.25), evaluator="formula", seed=21)
        e.selfplay_set_start(book, 2)
        e.selfplay_start(n, first)
        e.run()
        c = e.counters()
        assert c["games_finished"] == n and c["error_slots"] == 0
        got = e.fetch_samples()
        e.close()
        return got

    whole, lo, hi = play(0, 96), play(0, 48), play(48, 48)
    assert sorted(set(whole["game_idx"])) == list(range(96))
    for k in whole:
        assert np.array_equal(whole[k], np.concatenate([lo[k], hi[k]])), k
    for gi, i in first_rows(whole).items():
        start = O.state_from_moves(d, book[literal_start(gi, 5, 2)])
        assert np.array_equal(whole["x"][i], O.features(d, start).ravel()), gi


# ---------------------------------------------------------------- 7. contract
def test_set_start_contract():
    from dotsboxesaz_amd import _lib
    from dotsboxesaz_amd.engine import Engine
    d = O.dims(3, 3)
    e = Engine(3, 3, 4, mcts_num_read=20, evaluator="formula", seed=2)
    empty_x = O.features(d, O.new_state(d)).ravel()
    start = random_book(d, np.random.RandomState(7), 1, 6)[0]
    start_x = O.features(d, O.state_from_moves(d, start)).ravel()
    assert len(start) >= 1 and not np.array_equal(start_x, empty_x)

    def plays_from(x):
        e.selfplay_start(4, 0)
        e.run()
        c = e.counters()
        assert c["games_finished"] == 4 and c["error_slots"] == 0 and c["active_slots"] == 0
        got = e.fetch_samples()
        fr = first_rows(got)
        assert sorted(fr) == [0, 1, 2, 3]
        for i in fr.values():
            assert np.array_equal(got["x"][i], x) and got["move"][i] == -1

    # consumed by the next selfplay_start
    e.selfplay_set_start([start])
    plays_from(start_x)
    plays_from(empty_x)
    # one flat sequence = one start
    e.selfplay_set_start(start)
    plays_from(start_x)
    # n_starts = 0 clears
    for clear in (None, []):
        e.selfplay_set_start([start])
        e.selfplay_set_start(clear)
        plays_from(empty_x)
    # illegal move: ValueError naming the start
    with pytest.raises(ValueError, match="start 1"):
        e.selfplay_set_start([start, [0, 0]])
    plays_from(empty_x)
    with pytest.raises(ValueError, match="start 0"):
        e.selfplay_set_start([[1000]])
    plays_from(empty_x)
    # a finished start
    finished = [int(m) for m in np.nonzero(O.valid_moves(d, O.new_state(d)))[0]]
    assert O.get_result(O.state_from_moves(d, finished)) is not None
    with pytest.raises(_lib.DbazError) as ei:
        e.selfplay_set_start([start, finished])
    assert ei.value.code == _lib.EINVAL
    plays_from(empty_x)
    # games_per_start = 0
    with pytest.raises(_lib.DbazError) as ei:
        e.selfplay_set_start([start], 0)
    assert ei.value.code == _lib.EINVAL
    plays_from(empty_x)
    # descending offsets, negative n_starts, more starts than the cap
    mv = np.array(start + start, np.int16)
    off = np.array([0, len(start), len(start) - 1], np.int32)
    for n_starts, o in ((2, off), (-1, off), (65537, off)):
        with pytest.raises(_lib.DbazError) as ei:
            e._ck(e._L.dbaz_selfplay_set_start(e.h, mv.ctypes.data, o.ctypes.data, n_starts, 1))
        assert ei.value.code == _lib.EINVAL
        plays_from(empty_x)
    # a failed call leaves the starts of the previous call in place
    e.selfplay_set_start([start])
    with pytest.raises(ValueError):
        e.selfplay_set_start([[0, 0]])
    plays_from(start_x)
    # while games are being played
    e.selfplay_start(4, 0)
    e.step(1)
    with pytest.raises(_lib.DbazError) as ei:
        e.selfplay_set_start([start])
    assert ei.value.code == _lib.ESTATE
    e.run()
    assert e.counters()["games_finished"] == 4
    fr = e.fetch_samples()
    assert all(np.array_equal(fr["x"][i], empty_x) for i in first_rows(fr).values())
    plays_from(empty_x)
    # together with the benchmark's random fast-forward
    e.selfplay_set_start([start])
    e.selfplay_fastforward([2, 2, 2, 2])
    with pytest.raises(_lib.DbazError) as ei:
        e.selfplay_start(4, 0)
    assert ei.value.code == _lib.EINVAL
    plays_from(empty_x)
    # set_positions after a run from a book: the manual-search path starts from what IT is given
    e.selfplay_set_start([start])
    plays_from(start_x)
    e.set_positions(None)
    assert np.array_equal(e.rules_features(e.root_states())[0].ravel(), empty_x)
    plays_from(empty_x)
    e.close()


# ---------------------------------------------------------------- 8. mirror
_PARAMS = {"self_play": {"reuse_mcts_tree": True, "noise": [0.0, 0.0],
                         "mcts": {"mcts_num_read": 20, "mcts_cpuct": [1.25, 19652], "temperature": {0: 1.0, 12: 0.02}}}}


def _mirror_state(n_moves=6):
    from dotsboxesaz_amd.game import BoxesState
    BoxesState.init_static_fields(((3, 3),))
    st = BoxesState()
    rs = np.random.RandomState(3)
    for _ in range(n_moves):
        valid = st.get_valid_moves(as_indices=True)
        st.play_(valid[rs.randint(len(valid))])
    assert st.get_result() is None
    return st


def _check_all_games_start_at(sp, st, n_games):
    got = sp.samples
    fr = first_rows(got)
    assert sorted(fr) == list(range(n_games))
    for i in fr.values():
        assert np.array_equal(got["x"][i], st.get_features().ravel()) and got["move"][i] == -1
        assert got["player"][i] == st.to_play
    df = sp.get_datasets(1)
    assert len(df) == len(got["z"])


def test_mirror_async_play_games_forwards_its_game_state():
    from dotsboxesaz_amd.engine import Engine
    from dotsboxesaz_amd.self_play import SelfPlay
    st = _mirror_state()
    e = Engine(3, 3, 4, mcts_num_read=20, evaluator="formula", seed=4)
    sp = SelfPlay(e, _PARAMS)
    loop = asyncio.new_event_loop()
    try:
        loop.run_until_complete(sp.play_games(st, range(8)))
    finally:
        loop.close()
    _check_all_games_start_at(sp, st, 8)
    e.close()


def test_mirror_play_games_sync_forwards_its_game_state():
    from dotsboxesaz_amd.engine import Engine
    from dotsboxesaz_amd.game import BoxesState
    from dotsboxesaz_amd.self_play import SelfPlay
    st = _mirror_state()
    e = Engine(3, 3, 4, mcts_num_read=20, evaluator="formula", seed=4)
    sp = SelfPlay(e, _PARAMS)
    sp.play_games_sync(range(8), game_state=st)
    _check_all_games_start_at(sp, st, 8)
    # the start is not sticky: the empty board next
    sp2 = SelfPlay(e, _PARAMS)
    sp2.play_games_sync(range(8), game_state=BoxesState())
    _check_all_games_start_at(sp2, BoxesState(), 8)

    class EdgesOnly:  # a position that does not say how it was reached
        board = st.board

    with pytest.raises(TypeError):
        SelfPlay(e, _PARAMS).play_games_sync(range(8), game_state=EdgesOnly())
    BoxesState.init_static_fields(((2, 3),))
    try:
        with pytest.raises(ValueError):
            SelfPlay(e, _PARAMS).play_games_sync(range(8), game_state=BoxesState())
    finally:
        BoxesState.init_static_fields(((3, 3),))
    e.close()


# ---------------------------------------------------------------- 9. Elo matches from an opening book
def test_match_play_each_opening_meets_both_seatings():
    from dotsboxesaz_amd.engine import Engine
    d = O.dims(3, 3)
    book = random_book(d, np.random.RandomState(9), 3, 8)
    e = Engine(3, 3, 8, mcts_num_read=30, noise=(0.0, 0.0), reuse_tree=False, evaluator="formula", evaluator2="uniform",
               match_play=True, seed=9)
    e.selfplay_set_start(book, 2)
    e.selfplay_start(12, 0)
    e.run()
    c = e.counters()
    assert c["games_finished"] == 12 and c["error_slots"] == 0
    got = e.fetch_samples()
    fr = first_rows(got)
    for k in range(6):
        x = O.features(d, O.state_from_moves(d, book[k % 3])).ravel()
        assert np.array_equal(got["x"][fr[2 * k]], x) and np.array_equal(got["x"][fr[2 * k + 1]], x)
        assert got["player"][fr[2 * k]] == got["player"][fr[2 * k + 1]]  # same side to move, the other model on it
    e.close()


def test_compute_elo_from_openings():
    import torch
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd.self_play import compute_elo
    torch.manual_seed(0)
    pa = dnn.resnet_params(3, 3, 32, 2)
    pb = dnn.resnet_params(3, 3, 16, 1)
    for p in (pa, pb):
        p["self_play"] = {"reuse_mcts_tree": True, "noise": [0.8, 0.25],
                          "mcts": {"mcts_num_read": 100, "mcts_cpuct": [1.25, 19652], "temperature": {0: 1.0, 12: 0.02}}}
    elo_params = {"n_games": 24, "self_play_override": {"reuse_mcts_tree": False, "noise": [0.0, 0.0], "mcts": {"mcts_num_read": 30}}}
    book = random_book(O.dims(3, 3), np.random.RandomState(10), 3, 8)
    e0, e1, wins1 = compute_elo(elo_params, [pa, pb], [0, 0], (1000.0, 1000.0), nn_classes=[dnn.ResNetZero, dnn.ResNetZero],
                                rows=3, cols=3, n_slots=8, openings=book)
    assert abs((e0 - 1000.0) + (e1 - 1000.0)) < 1e-9  # zero-sum update
    assert np.isnan(wins1) or 0.0 <= wins1 <= 1.0
    with pytest.raises(ValueError):  # an illegal opening is an error, not the empty board
        compute_elo(elo_params, [pa, pb], [0, 0], (1000.0, 1000.0), nn_classes=[dnn.ResNetZero, dnn.ResNetZero],
                    rows=3, cols=3, n_slots=8, openings=[[0, 0]])
