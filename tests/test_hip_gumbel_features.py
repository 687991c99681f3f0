"""The Gumbel root search next to the other features of the self-play driver, against tests/gumbel_ref.py (whose side of these cases
test_gumbel_ref_cpu.py checks without a GPU: the gap condition, and that each case reaches what it is there for):

* an endgame table in the search with tree reuse -- a served root that another evaluator's leaf expanded keeps its prior, so m' > 1
  under a table, and endgame_reads makes the R that begin_search stores smaller than m';
* the same tables from a pool that runs dry (the first served move of every game read from the slots' headers) and in wait mode;
* the leaf solver under a Gumbel root;
* games from start positions: g is drawn at the ply counted from the start position;
* more slots than one 16-game workgroup of k_select, and a slot count that is no multiple of 16;
* the transposition cache forced on a formula evaluator.

Formula evaluators throughout; rows are compared as test_hip_gumbel.py compares them (visits within +-1 count per entry: device and
host exp / log), counters where the reference has them."""
import ctypes as C
import warnings

import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd.endgame import DeepTables, Endgame
import endgame_selfplay_ref as ESR
import gumbel_ref as GR
from test_hip_gumbel import game_rows, make, played

pytestmark = pytest.mark.gpu

GUM = (16, GR.C_VISIT, GR.C_SCALE)


def compare_game(rows, g, what):
    """one game of the engine against the reference's; returns the largest difference in counts"""
    worst = 0
    n = min(len(rows["played"]), g["n_rows"])
    for i in range(n):  # row by row: the message names the first ply that differs
        where = (what, "ply", i, "served" if g["served"][i] else "unserved", "reads", int(g["reads"][i]), "m'", int(g["m_eff"][i]))
        assert rows["played"][i] == g["played"][i], where
        assert np.array_equal(rows["x"][i], g["x"][i]) and rows["player"][i] == g["player"][i], where
        assert np.float32(rows["q_value"][i]).tobytes() == np.float32(g["q_value"][i]).tobytes(), where
        for key in ("tree_size", "max_deepness", "terminal_count"):
            assert rows[key][i] == g[key][i], where + (key,)
        diff = int(np.abs(rows["visits"][i].astype(np.int64) - g["visits"][i]).max())
        worst = max(worst, diff)
        assert diff <= 1, where + (rows["visits"][i], g["visits"][i])
    assert len(rows["played"]) == g["n_rows"], what
    assert np.array_equal(rows["z"], g["z"]), what
    assert rows["gumbel"].all(), what
    if "full" in rows:  # the column exists with the playout cap on
        assert np.array_equal(rows["full"], g["full"]), what
    vs = rows["visits"].sum(axis=1, dtype=np.int64).astype(np.float64)
    assert np.array_equal(rows["pi"], rows["visits"] / vs[:, None]), what
    return worst


def compare(name, got, games):
    worst = max(compare_game(game_rows(got, gi), g, (name, "game", gi)) for gi, g in games.items())
    print(name, "largest difference in counts", worst)
    return {k: sum(g[k] for g in games.values()) for k in ("n_search", "n_rows", "base_calls", "table_calls")}


def feature_engine(name, **kw):
    f = GR.FEATURES[name]
    return make(f["R"], f["C"], f["slots"], (f["m"], GR.C_VISIT, GR.C_SCALE), sims=f["sims"], reuse_tree=f["reuse"], **kw)


# ---------------------------------------------------------------- an endgame table in the search, tree reuse on
@pytest.mark.parametrize("name", [n for n in GR.FEATURE_IDS if "table" in GR.FEATURES[n]])
def test_table_in_the_search_against_the_reference(name):
    f = GR.FEATURES[name]
    games, _ = GR.feature_games(name)
    h = Endgame(f["R"], f["C"], max_free=f["table"])
    e = feature_engine(name, endgame=h, endgame_seed=GR.TABLE_SEED, endgame_reads=f["endgame_reads"])
    c, gm, got = played(e, f["games"])
    stats = e.endgame_stats()
    e.close()
    h.close()
    tot = compare(name, got, games)
    assert c["expansions"] == tot["n_search"]
    assert stats == (sum(bool(g["served"].any()) for g in games.values()), tot["table_calls"])
    assert c["nn_evals"] == tot["base_calls"] and c["cache_hits"] == 0
    assert (gm["searches"], gm["rows"]) == (tot["n_rows"], tot["n_rows"])


# ---------------------------------------------------------------- the same tables from a pool
def test_table_pool_that_runs_dry_against_the_reference():
    """4 regions for 24 slots, deny mode: a slot that finds the pool dry searches that move with the formula evaluator.  Which searches
    were denied is the schedule's, so the device is asked, as test_hip_leaf_solve.py asks it: after every step the slots' headers name
    the game a table serves and the free edges F0 of the root it was solved at -- the game's first served move is E - F0 plies
    from the empty board.  The reference replays every game with exactly that served_from."""
    name = "3x3-table"
    f = GR.FEATURES[name]
    E = 2 * f["R"] * f["C"] + f["R"] + f["C"]
    h = DeepTables(f["R"], f["C"], max_free=f["table"])
    e = feature_engine(name, endgame=h, endgame_seed=GR.TABLE_SEED, endgame_tables=4)
    e.selfplay_start(f["games"], 0)
    served_from = {}
    valid, n_free, game = C.c_int32(), C.c_int32(), C.c_int64()
    for _ in range(100000):
        e.step(1)
        for slot in range(f["slots"]):
            e._ck(e._L.dbaz_get_slot_table(e.h, slot, C.byref(valid), C.byref(n_free), C.byref(game), None, None, 0, 0))
            if valid.value:
                assert served_from.setdefault(int(game.value), E - int(n_free.value)) == E - int(n_free.value)  # one table per game
        if e.counters()["active_slots"] == 0:
            break
    c = e.counters()
    assert c["games_finished"] == f["games"] and c["error_slots"] == 0 and c["active_slots"] == 0
    got = e.fetch_samples()
    stats, pool, gm = e.endgame_stats(), e.table_pool(), e.gumbel()
    e.close()
    h.close()
    late = tuple(sorted((gi, served_from.get(gi, ESR.NEVER)) for gi in range(f["games"])))
    games, _ = GR.feature_games(name, served_from=late)
    tot = compare(name + " from a dry pool", got, games)
    denied = 0
    for gi, g in games.items():
        first = int(np.nonzero(g["n_free"] <= f["table"])[0][0])
        sf = served_from.get(gi, g["n_rows"])
        assert first <= sf and g["first_served"] == (sf if gi in served_from else -1), (gi, first, sf)
        denied += sf - first
    print("dry pool: %s, endgame_stats %s, first served moves %s, gap %g" % (pool, stats, served_from, min(g["min_gap"] for g in games.values())))
    assert min(g["min_gap"] for g in games.values()) >= 1e-9  # (these games are not all among the CPU test's)
    assert pool["denied"] == denied > 0 and pool["high_water"] == 4 and pool["in_use"] == 0
    assert stats == (len(served_from), tot["table_calls"]) and tot["table_calls"] > 0
    assert c["expansions"] == tot["n_search"] and c["nn_evals"] == tot["base_calls"]
    assert (gm["searches"], gm["rows"]) == (tot["n_rows"], tot["n_rows"])


@pytest.mark.parametrize("name", ["3x3-table", "3x3-table-reads3"])
def test_table_pool_in_wait_mode_against_the_reference(name):
    """4 regions for 24 slots, wait mode: a slot that finds the pool dry waits, so every root with F <= max_free is served and the rows
    are the per-slot attach's -- the reference's with every eligible root served"""
    f = GR.FEATURES[name]
    games, _ = GR.feature_games(name)
    h = DeepTables(f["R"], f["C"], max_free=f["table"])
    e = feature_engine(name, endgame=h, endgame_seed=GR.TABLE_SEED, endgame_tables=4, endgame_wait=True, endgame_reads=f["endgame_reads"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c, gm, got = played(e, f["games"])
    stats, pool = e.endgame_stats(), e.table_pool()
    e.close()
    h.close()
    tot = compare(name + " from a pool in wait mode", got, games)
    print("wait mode: %s" % (pool,))
    assert pool["denied"] == 0 and pool["high_water"] == 4 and pool["in_use"] == 0
    assert stats == (f["games"], tot["table_calls"]) and c["expansions"] == tot["n_search"] and c["nn_evals"] == tot["base_calls"]


# ---------------------------------------------------------------- the leaf solver under a Gumbel root
@pytest.mark.parametrize("name", [n for n in GR.FEATURE_IDS if "leaf" in GR.FEATURES[n]])
def test_leaf_solver_against_the_reference(name):
    f = GR.FEATURES[name]
    games, w = GR.feature_games(name)
    h = Endgame(f["R"], f["C"], max_free=f["leaf"])
    e = feature_engine(name, leaf_endgame=h, endgame_seed=GR.TABLE_SEED)  # leaf_free None: the handle's max_free
    c, gm, got = played(e, f["games"])
    ls, stats = e.leaf_solves(), e.endgame_stats()
    e.close()
    h.close()
    tot = compare(name, got, games)
    print("%s: %d leaves solved by F %s, %d of them under roots with F > L" % (name, w.calls["solved"], w.by_free[:f["leaf"] + 1],
                                                                             sum(w.solved_under_high_roots())))
    assert ls["by_free"] == w.by_free and ls["total"] == w.calls["solved"] > 0
    assert c["expansions"] == tot["n_search"] and c["nn_evals"] == w.calls["base"] and c["cache_hits"] == 0
    assert stats == (0, 0) and tot["table_calls"] == 0


# ---------------------------------------------------------------- start positions
@pytest.mark.parametrize("name", [n for n in GR.FEATURE_IDS if "starts" in GR.FEATURES[n]])
def test_start_positions_against_the_reference(name):
    """three openings of different lengths, two games each: move_idx, the scripts and the Philox counter of g count plies from the start
    position (Engine.selfplay_set_start), so the first row of every game is ply 0"""
    f = GR.FEATURES[name]
    games, _ = GR.feature_games(name)
    book = GR.feature_book(name)
    d = O.dims(f["R"], f["C"])
    e = feature_engine(name)
    e.selfplay_set_start(book, 2)
    if f["g"] == "script":
        for gi, g in games.items():
            e.selfplay_script(gi, np.full(g["n_rows"], -1, np.int16), g["vectors"])
    c, gm, got = played(e, f["games"])
    e.close()
    tot = compare(name, got, games)
    for gi in games:
        rows = game_rows(got, gi)  # (asserts move_idx 0, 1, ...)
        assert rows["move"][0] == -1
        assert np.array_equal(rows["x"][0], O.features(d, O.state_from_moves(d, book[GR.start_of(gi, 3, 2)])).ravel()), gi
    assert c["expansions"] == tot["n_search"] and (gm["searches"], gm["rows"]) == (tot["n_rows"], tot["n_rows"])


# ---------------------------------------------------------------- more than one workgroup of the sixteen-game form
def test_forty_slots_against_the_reference():
    """40 slots: three 16-game workgroups of k_select<1, false, true>, the last one with 8 games; 80 games, so every slot is refilled"""
    name = "3x3-40-slots"
    f = GR.FEATURES[name]
    games, _ = GR.feature_games(name)
    e = feature_engine(name)
    c, gm, got = played(e, f["games"])
    e.close()
    assert sorted(games) == sorted(f["replay"]) and len(games) == 8
    tot = compare(name, got, games)
    n_rows = len(got["played"])
    assert c["expansions"] > tot["n_search"] and (gm["searches"], gm["rows"]) == (n_rows, n_rows)


# ---------------------------------------------------------------- the transposition cache forced on a formula evaluator
def test_forced_transposition_cache_changes_no_row():
    name = "3x3-script-m4"
    _, R, Cc, sims, m, reuse, cap, g_mode, ev, n_games, c_visit, c_scale = GR.case(name)
    games = GR.case_games(name)
    out = []
    for tt in (True, "force"):
        e = make(R, Cc, 8, (m, c_visit, c_scale), sims=sims, evaluator=ev, reuse_tree=reuse, playout_cap=cap, transposition_cache=tt)
        for gi, g in enumerate(games):
            e.selfplay_script(gi, np.full(g["n_rows"], -1, np.int16), g["vectors"])
        out.append(played(e, n_games))
        e.close()
    (ca, ga, a), (cb, gb, b) = out
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
    assert ca["cache_hits"] == 0 and cb["cache_hits"] > 0 and ga == gb
    assert ca["expansions"] == cb["expansions"] and cb["nn_evals"] + cb["cache_hits"] == ca["nn_evals"]
