#!/usr/bin/env python3
"""Generate tests/golden/selfplay_start.npz by IMPORTING the reference: SelfPlay.play_games(game_state, idxs) /
play_game(game_state, idx) from start positions that are not the empty board (self_play.py:51-55,76-80).

Runs only where the reference is installed (see gen_golden.py).  Usage:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_start.py

Per self-play case the keys of selfplay.npz (_cfg _temp _index _move _player _x _pi _z _stats _q _drawn_moves
_drawn_noise) plus _start_moves / _start_offsets / _games_per_start: start s is the position after
start_moves[start_offsets[s]:start_offsets[s+1]], game g begins from start (g // games_per_start) % n_starts.
The match-play case has the keys of match.npz plus the same three.

The start moves are played as np.int64, as the reference itself plays every move (results of np.random.choice /
np.argmax): BoxesState._update_hash shifts `1 << move`, which wraps for numpy integers and turns into a Python big int --
and then breaks UCT_search -- for Python ints on boards with more than 63 actions.
"""
import os

import numpy as np

from gen_golden import BoxesState, formula_eval, make_async_formula, run, set_board  # noqa: F401  (imports the reference)

HERE = os.path.dirname(os.path.abspath(__file__))


def start_of(game_idx, n_starts, games_per_start):
    """The mapping of dbaz_selfplay_set_start, written out here (not imported from the code under test)."""
    return (game_idx // games_per_start) % n_starts


def play_start(moves):
    s = BoxesState()
    for m in moves:
        s.play_(np.int64(m))
    return s


def random_start(rs, plies, accept=None, max_plies=None):
    """A random legal non-terminal position after `plies` plies (or, with max_plies, the first ply count in
    plies..max_plies at which accept(state) holds); accept filters, the draw is repeated until it holds."""
    for _ in range(100000):
        s = BoxesState()
        moves = []
        ok = True
        while len(moves) < (max_plies or plies):
            valid = s.get_valid_moves(as_indices=True)
            if s.get_result() is not None or not len(valid):
                ok = False
                break
            m = np.int64(valid[rs.randint(len(valid))])
            s.play_(m)
            moves.append(int(m))
            if len(moves) >= plies and s.get_result() is None and (accept is None or accept(s)):
                break
        if ok and len(moves) >= plies and s.get_result() is None and (accept is None or accept(s)):
            return moves
    raise RuntimeError("no start position found")


def record_rng():
    drawn_noise, drawn_moves = [], []
    o_dir, o_ch = np.random.dirichlet, np.random.choice

    def rec_dir(alpha, size=None):
        r = o_dir(alpha, size)
        drawn_noise.append(np.asarray(r).ravel().copy())
        return r

    def rec_choice(a, size=None, replace=True, p=None):
        r = o_ch(a, size, replace, p)
        drawn_moves.append(int(np.asarray(r).ravel()[0]))
        return r

    np.random.dirichlet, np.random.choice = rec_dir, rec_choice

    def restore():
        np.random.dirichlet, np.random.choice = o_dir, o_ch
    return drawn_moves, drawn_noise, restore


def put_starts(out, k, starts, gps):
    out[k + "start_moves"] = np.array([m for s in starts for m in s], dtype=np.int16)
    out[k + "start_offsets"] = np.cumsum([0] + [len(s) for s in starts]).astype(np.int32)
    out[k + "games_per_start"] = np.array(gps, dtype=np.int32)


def main():
    import self_play as ref_sp
    from utils.utils import DotDict
    out, cases = {}, []
    rs = np.random.RandomState(20251)

    def run_case(name, rows, cols, sims, noise, reuse, n_games, seed, evaluator, starts, gps=1, temperature=None):
        set_board(rows, cols)
        temperature = {0: 1.0, 12: 0.02} if temperature is None else temperature
        params = DotDict({"self_play": {"reuse_mcts_tree": bool(reuse), "noise": list(noise),
                                        "mcts": {"mcts_num_read": sims, "mcts_cpuct": [1.25, 19652],
                                                 "temperature": dict(temperature), "max_async_searches": 1}}})
        states = [play_start(s) for s in starts]
        assert all(s.get_result() is None for s in states)
        np.random.seed(seed)
        drawn_moves, drawn_noise, restore = record_rng()
        try:
            sp = ref_sp.SelfPlay(evaluator, params)
            if len(starts) == 1:
                run(sp.play_games(states[0], list(range(n_games))))
            else:
                for gi in range(n_games):
                    run(sp.play_game(states[start_of(gi, len(starts), gps)], gi))
        finally:
            restore()
        df = sp.get_datasets(3, with_features=True).reset_index()
        A = 2 * (rows + 1) * (cols + 1)
        F = 3 * (rows + 1) * (cols + 1)
        k = name + "_"
        out[k + "cfg"] = np.array([rows, cols, sims, noise[0], noise[1], int(reuse), n_games, seed], dtype=np.float64)
        out[k + "temp"] = np.array(sorted(temperature.items()), dtype=np.float64)
        out[k + "index"] = df[["generation", "game_idx", "move_idx"]].to_numpy().astype(np.int16)
        out[k + "move"] = df["move"].to_numpy().astype(np.int16)
        out[k + "player"] = df["player"].to_numpy().astype(np.int8)
        out[k + "x"] = df[["x_%d" % i for i in range(F)]].to_numpy().astype(np.int16)
        out[k + "pi"] = df[["pi_%d" % i for i in range(A)]].to_numpy().astype(np.float64)
        out[k + "z"] = df["z"].to_numpy().astype(np.int64)
        out[k + "stats"] = df[["max_deepness", "tree_size", "terminal_count"]].to_numpy().astype(np.int32)
        out[k + "q"] = df["q_value"].to_numpy().astype(np.float32)
        out[k + "drawn_moves"] = np.array(drawn_moves, dtype=np.int16)
        out[k + "drawn_noise"] = (np.stack(drawn_noise) if drawn_noise else np.zeros((0, A)))
        put_starts(out, k, starts, gps)
        # every game's first row shows its start position
        for gi in range(n_games):
            first = df[(df["game_idx"] == gi) & (df["move_idx"] == 0)]
            exp = states[start_of(gi, len(starts), gps)].get_features().ravel()
            assert len(first) == 1 and np.array_equal(first[["x_%d" % i for i in range(F)]].to_numpy()[0], exp)
        cases.append(name)
        print("  ", name, "rows", len(df), "start plies", [len(s) for s in starts])

    set_board(3, 3)
    mid = random_start(rs, 7, accept=lambda s: list(s.boxes_to_close) == [4.5, 4.5])
    st = play_start(mid)
    assert len(mid) == 7 and list(st.boxes_to_close) == [4.5, 4.5]
    run_case("st33_mid", 3, 3, 25, (0.8, 0.25), True, 2, 10, make_async_formula(0), [mid], temperature={0: 1.0, 4: 0.02})

    set_board(3, 3)
    late = random_start(rs, 14, accept=lambda s: s.just_played == s.to_play and s.to_play == 0, max_plies=20)
    st = play_start(late)
    assert len(late) >= 14 and st.just_played == st.to_play == 0 and st.get_result() is None
    run_case("st33_late", 3, 3, 30, (0.0, 0.0), False, 2, 11, make_async_formula(0), [late])

    set_board(2, 3)
    book = [random_start(rs, n) if n else [] for n in (0, 3, 6)]
    assert [len(b) for b in book] == [0, 3, 6]
    run_case("st23_book", 2, 3, 40, (0.8, 0.25), True, 7, 12, make_async_formula(0), book, gps=2)

    set_board(6, 6)
    run_case("st66_mid", 6, 6, 60, (0.8, 0.25), True, 1, 13, make_async_formula(0), [random_start(rs, 40)])

    set_board(3, 3)
    run_case("st33_uniform", 3, 3, 40, (0.8, 0.25), True, 1, 14, make_async_formula(1), [random_start(rs, 10)])

    # match play as gen_golden.gen_match: model 0 hash formula / model 1 uniform, seats by game_idx & 1
    name, rows, cols, sims, n_games, seed, gps = "m33_book", 3, 3, 30, 4, 15, 2
    set_board(rows, cols)
    starts = [random_start(rs, 4), random_start(rs, 9)]
    states = [play_start(s) for s in starts]
    assert all(s.get_result() is None for s in states)
    params = DotDict({"self_play": {"reuse_mcts_tree": False, "noise": [0.0, 0.0],
                                    "mcts": {"mcts_num_read": sims, "mcts_cpuct": [1.25, 19652],
                                             "temperature": {0: 1.0, 12: 0.02}, "max_async_searches": 1}}})
    np.random.seed(seed)
    cur = {"model": 0, "game": 0}

    async def nn(s_, _s=cur):
        return formula_eval(s_, 0 if _s["model"] == 0 else 1)

    drawn, _noise, restore = record_rng()
    try:
        sp = ref_sp.SelfPlay(nn, params)
        sp.set_player_change_callback(lambda player, _s=cur: _s.__setitem__("model", player ^ (_s["game"] & 1)))
        for gi in range(n_games):
            cur["game"] = gi
            run(sp.play_game(states[start_of(gi, len(starts), gps)], gi))
    finally:
        restore()
    df = sp.get_datasets([7, 9], with_features=False).reset_index()
    assert not any(c.startswith("x_") for c in df.columns)
    A = 2 * (rows + 1) * (cols + 1)
    k = name + "_"
    out[k + "cfg"] = np.array([rows, cols, sims, n_games, seed], dtype=np.int32)
    out[k + "index"] = df[["generation", "game_idx", "move_idx"]].to_numpy().astype(np.int16)
    out[k + "move"] = df["move"].to_numpy().astype(np.int16)
    out[k + "player"] = df["player"].to_numpy().astype(np.int8)
    out[k + "pi"] = df[["pi_%d" % i for i in range(A)]].to_numpy().astype(np.float64)
    out[k + "z"] = df["z"].to_numpy().astype(np.int64)
    out[k + "stats"] = df[["max_deepness", "tree_size", "terminal_count"]].to_numpy().astype(np.int32)
    out[k + "q"] = df["q_value"].to_numpy().astype(np.float32)
    out[k + "drawn_moves"] = np.array(drawn, dtype=np.int16)
    out[k + "columns"] = np.array(list(df.columns))
    put_starts(out, k, starts, gps)
    print("  ", name, "rows", len(df), "start plies", [len(s) for s in starts])

    out["cases"] = np.array(cases)
    out["match_cases"] = np.array([name])
    np.savez_compressed(os.path.join(HERE, "selfplay_start.npz"), **out)
    print("selfplay_start.npz", len(cases), "+ 1 cases")


if __name__ == "__main__":
    main()
