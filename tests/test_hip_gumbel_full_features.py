"""The full mode of the Gumbel search next to the other features of the self-play driver, against tests/gumbel_full_ref.py (whose side
of these cases test_gumbel_full_ref_cpu.py checks without a GPU):

* Endgame(3, 3, 8) attached, with tree reuse: nodes that the table's answer expanded carry the exact value as their v^, at the root
  of a served search and below it;
* the leaf solver on 3x3: the same for the leaves it solves;
* games from start positions.

Formula evaluators; rows are compared as test_hip_gumbel_full.py compares them."""
import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd.endgame import Endgame
import gumbel_full_ref as GF
import gumbel_ref as GR
from test_hip_gumbel_full import compare, make, played

pytestmark = pytest.mark.gpu


def feature_engine(name, **kw):
    f = GF.FEATURES[name]
    return make(f["R"], f["C"], f["slots"], (f["m"], GR.C_VISIT, GR.C_SCALE, True), sims=f["sims"], reuse_tree=f["reuse"], **kw)


def totals(games):
    return {k: sum(g[k] for g in games.values()) for k in ("n_search", "n_rows", "base_calls", "table_calls")}


def test_table_in_the_search_against_the_reference():
    name = "3x3-table"
    f = GF.FEATURES[name]
    games, _ = GF.feature_games(name)
    h = Endgame(f["R"], f["C"], max_free=f["table"])
    e = feature_engine(name, endgame=h, endgame_seed=GR.TABLE_SEED)
    c, gm, got = played(e, f["games"])
    stats = e.endgame_stats()
    e.close()
    h.close()
    print(name, "largest difference in counts", compare([games[gi] for gi in range(f["games"])], got))
    tot = totals(games)
    assert c["expansions"] == tot["n_search"]
    assert stats == (sum(bool(g["served"].any()) for g in games.values()), tot["table_calls"]) and tot["table_calls"] > 0
    assert c["nn_evals"] == tot["base_calls"] and (gm["searches"], gm["rows"]) == (tot["n_rows"], tot["n_rows"])


def test_leaf_solver_against_the_reference():
    name = "3x3-leaf"
    f = GF.FEATURES[name]
    games, w = GF.feature_games(name)
    h = Endgame(f["R"], f["C"], max_free=f["leaf"])
    e = feature_engine(name, leaf_endgame=h, endgame_seed=GR.TABLE_SEED)
    c, gm, got = played(e, f["games"])
    ls = e.leaf_solves()
    e.close()
    h.close()
    print(name, "largest difference in counts", compare([games[gi] for gi in range(f["games"])], got))
    assert ls["by_free"] == w.by_free and ls["total"] == w.calls["solved"] > 0
    assert c["expansions"] == totals(games)["n_search"] and c["nn_evals"] == w.calls["base"]


def test_start_positions_against_the_reference():
    name = "3x3-start"
    f = GF.FEATURES[name]
    games, _ = GF.feature_games(name)
    book = GF.feature_book(name)
    d = O.dims(f["R"], f["C"])
    e = feature_engine(name)
    e.selfplay_set_start(book, 2)
    c, gm, got = played(e, f["games"])
    e.close()
    print(name, "largest difference in counts", compare([games[gi] for gi in range(f["games"])], got))
    first = got["move_idx"] == 0
    for gi, x0 in zip(got["game_idx"][first], got["x"][first]):
        assert np.array_equal(x0, O.features(d, O.state_from_moves(d, book[GR.start_of(gi, 3, 2)])).ravel()), gi
    tot = totals(games)
    assert c["expansions"] == tot["n_search"] and (gm["searches"], gm["rows"]) == (tot["n_rows"], tot["n_rows"])
