"""tests/gumbel_match_ref.py on its own (no GPU): the helper plays the games of its CASES with its own moves on the PUCT plies.

* every case has min_gap >= 1e-9 in every game (the bound and its derivation are in gumbel_full_ref's docstring), so the last bit of
  a device log or exp changes no decision of these games; no game is skipped;
* each deliberate mistake changes at least half the games of the case named for it;
* each case reaches what it is there for: both seatings, both rules in one game, interior picks where a model is full, capped reads."""
import numpy as np
import pytest

import gumbel_match_ref as GM

SMALL = [n for n in GM.CASE_IDS if GM.CASES[n]["R"] * GM.CASES[n]["C"] <= 9]


@pytest.mark.parametrize("name", GM.CASE_IDS)
def test_gap_condition_in_every_game(name):
    games = GM.case_games(name)
    assert len(games) == GM.CASES[name]["games"]
    for gi, g in enumerate(games):
        assert g["min_gap"] >= 1e-9, (name, gi, g["min_gap"])
        assert not g["ended_early"] and g["n_gumbel"] > 0


@pytest.mark.parametrize("mistake", GM.MISTAKES)
def test_each_mistake_changes_its_case(mistake):
    name = GM.MISTAKE_CASES[mistake]
    a, b = GM.case_games(name), GM.case_games(name, mistake)
    changed = sum(GM.games_differ(x, y) for x, y in zip(a, b))
    assert 2 * changed >= len(a), (mistake, name, changed)


@pytest.mark.parametrize("name", SMALL)
def test_cases_reach_what_they_are_for(name):
    c = GM.CASES[name]
    S = [GM.norm_spec(s) for s in c["specs"]]
    games = GM.case_games(name)
    for gi, g in enumerate(games):
        model = (g["player"] ^ (gi & 1)) & 1
        assert np.array_equal(model, g["model"])
        assert set(model) == {0, 1}, (name, gi)  # both models search in every game
        for k in (0, 1):
            rows = model == k
            want = 4 * (S[k][1] > 0) + 8 * (S[k][1] > 0 and S[k][4])
            assert (g["flags"][rows] == want).all(), (name, gi, k)
            cap = S[k][0] or c["sims"]
            assert g["reads"][rows].max() <= cap, (name, gi, k)
            if S[k][1] > 0:  # a Gumbel row is the target in units of 2^-24
                assert (np.abs(g["visits"][rows].sum(axis=1) - (1 << 24)) <= g["visits"].shape[1]).all(), (name, gi, k)
    # both seatings: from the empty board model 0 moves first in even games; a book's games 2k and 2k + 1 have opposite seatings
    if "book" not in c:
        assert {int(g["model"][0]) for g in games[0::2]} == {0} and {int(g["model"][0]) for g in games[1::2]} == {1}
    assert all(a["model"][0] != b["model"][0] for a, b in zip(games[0::2], games[1::2]))
    if any(s[1] > 0 and s[4] for s in S):
        assert sum(g["interior_picks"] for g in games) > 0
    else:
        assert sum(g["interior_picks"] for g in games) == 0
    if name == "a":  # each model's own budget shows: 16 on the Gumbel rows, 24 on the PUCT rows
        assert max(g["reads"][g["model"] == 0].max() for g in games) == 16 and max(g["reads"][g["model"] == 1].max() for g in games) == 24
    if name == "f":  # R is the capped count where the table serves the Gumbel model
        assert any((g["reads"][g["model"] == 0] == c["endgame_reads"]).any() for g in games)


def test_deterministic_models_repeat_their_games():
    """case d: g_scale = 0 on both models and a book of 4 openings, 2 games each: games 2k and 2k + 8 are the same game"""
    games = GM.case_games("d")
    for k in range(4):
        assert not GM.games_differ(games[2 * k], games[2 * k + 8]), k
    assert any(GM.games_differ(games[0], games[2 * k]) for k in range(1, 4))
