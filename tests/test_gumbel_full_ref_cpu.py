"""tests/gumbel_full_ref.py on its own (no device): the cases the GPU tests play are far from ties at every decision, interior ones
included; they reach what they are there for -- interior picks deep in the tree and at visited nodes; the full mode changes every
game of every case; and each deliberate mistake of the helper's mistake= switch changes at least half of the games of the cases it
is listed for, so a device that made it could not pass the GPU tests."""
import numpy as np
import pytest

import gumbel_full_ref as GF
import gumbel_ref as GR


@pytest.mark.parametrize("name", GF.CASE_IDS)
def test_cases_are_far_from_ties_and_reach_the_interior(name):
    games = GF.case_games(name)
    gap = min(g["min_gap"] for g in games)
    print(name, "minimum gap", gap, "interior picks", sum(g["interior_picks"] for g in games), "at depth >= 3", sum(g["deep_picks"] for g in games),
          "at visited nodes", sum(g["visited_picks"] for g in games))
    assert gap >= 1e-9
    assert sum(g["deep_picks"] for g in games) > 0 and sum(g["visited_picks"] for g in games) > 0
    for g in games:
        assert (g["flags"] & 12 == 12).all() and g["interior_picks"] > 0
    root_only = GF.case_games(name, full=False)
    assert all(GF.games_differ(a, b) for a, b in zip(games, root_only))
    assert all((b["flags"] & 8 == 0).all() for b in root_only)


@pytest.mark.parametrize("mistake", GF.MISTAKES)
def test_every_mistake_changes_the_games(mistake):
    assert GF.MISTAKE_CASES[mistake]
    for name in GF.MISTAKE_CASES[mistake]:
        games, wrong = GF.case_games(name), GF.case_games(name, mistake)
        changed = sum(GF.games_differ(a, b) for a, b in zip(games, wrong))
        print(mistake, name, changed, "of", len(games))
        assert 2 * changed >= len(games), (mistake, name)


@pytest.mark.parametrize("name", GF.FEATURE_IDS)
def test_feature_cases(name):
    games, w = GF.feature_games(name)
    assert min(g["min_gap"] for g in games.values()) >= 1e-9
    assert sum(g["deep_picks"] for g in games.values()) > 0
    root_only, _ = GF.feature_games(name, full=False)
    assert all(GF.games_differ(games[k], root_only[k]) for k in games)
    f = GF.FEATURES[name]
    if "table" in f:  # served roots under tree reuse, and leaves the table answered
        assert sum(g["table_calls"] for g in games.values()) > 0 and all(g["served"].any() for g in games.values())
    if "leaf" in f:
        assert w.calls["solved"] > 0


def test_the_rule_on_one_node():
    """by hand: two visited children and an unvisited one"""
    P, W, n, sgn, valid = [0.5, 0.25, 0.25], np.array([1.0, -0.5, 0.0], np.float32), [1, 1, 0], [1, -1, 1], [True, True, True]
    q = GR.q_values(W, n, sgn)
    assert q[:2] == [0.5, 0.25]
    vm = GF.v_mix_full(0.1, P, q, n)
    assert vm == (0.1 + 2.0 * ((0.5 * 0.5 + 0.25 * 0.25) / 0.75)) / 3.0
    assert GF.v_mix_full(0.1, P, [0.0] * 3, [0, 0, 0]) == 0.1  # nothing visited: the node's own value
    C_, x, pi = GF.improved_policy(50.0, 1.0, 0.1, P, W, n, sgn, valid)
    assert C_ == [0, 1, 2] and abs(sum(pi) - 1.0) < 1e-15
    sc = GF.nonroot_scores(50.0, 1.0, 0.1, P, W, n, sgn, valid)
    assert [s for _, s, _, _ in sc] == [pi[0] - 1.0 / 3.0, pi[1] - 1.0 / 3.0, pi[2] - 0.0]
