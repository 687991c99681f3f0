"""The tree side of a self-play step outside the network (csrc/tree.hip): the one-pass slot scans of k_order_evals and
k_driver_scan (scan_ranks) and the two forms of k_select -- sixteen games per workgroup where k_select writes the evaluation
lists itself, one game per workgroup on the full-rounds path (eval_round > 0), where k_order_evals writes the list.

The shapes are the smallest at which the scans can go wrong, not the workload's: 65 slots (a partial wave), 1 000 (a partial
chunk of 1 024), 1 025 (one slot into the second chunk), 2 100 (a partial third chunk, and the first size that takes the
eight-chunk instance instead of the two-chunk one: up to 2 048 slots the launchers pick <SCAN_NG_SMALL>, and either instance
then holds all slots in ONE group) and 8 200 (eight slots behind the 8 192 that one group of the eight-chunk instance takes: the
only way into the second group -- the carried bases, the put-off leaves counted in front of the groups, the barrier before the
LDS table is written again, and k_driver_scan compacting drv_list in place across groups).  Nothing here has a tolerance:
a game's rows are a function of (seed, game index) alone, so every comparison is bit for bit."""
import numpy as np
import pytest

SIMS, SEED = 24, 11
CUT = (16, 15)  # eval_round, eval_defer_max: tiny rounds, so that put-off and new leaves share the list in most steps
COUNTERS = ("expansions", "nn_evals", "cache_hits", "terminal_leaves", "games_finished")

_runs = {}


def _play(n_slots, n_games, cut):
    """One seeded self-play run of the 3x3 network of test_full_rounds_only_changes_nothing_but_the_schedule: (rows sorted by
    (game, move), counters).  Runs are kept: the tests share them and leave them unchanged."""
    key = (n_slots, n_games, cut)
    if key not in _runs:
        import torch
        from dotsboxesaz_amd.engine import Engine
        from dotsboxesaz_amd import nn as dnn
        torch.manual_seed(4)
        model = dnn.ResNetZero(dnn.resnet_params(3, 3, 32, 2, 4, 8))
        er, ed = CUT if cut else (-1, 0)
        e = Engine(3, 3, n_slots, mcts_num_read=SIMS, noise=(0.8, 0.25), reuse_tree=True, evaluator="resnet", seed=SEED,
                   eval_round=er, eval_defer_max=ed)
        e.load_state_dict(model.state_dict(), "resnet", **model.shape)
        e.selfplay_start(n_games, 0)
        e.run()
        c = e.counters()
        rows = e.fetch_samples()
        e.close()
        _runs[key] = (rows, c)
    return _runs[key]


def _play_again(n_slots, n_games, cut):
    first = _runs.pop((n_slots, n_games, cut))
    again = _play(n_slots, n_games, cut)
    _runs[(n_slots, n_games, cut)] = first
    return again


def _same_rows(a, b):
    assert len(a["z"]) == len(b["z"])
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _of_games(rows, n_games):
    keep = rows["game_idx"] < n_games
    return {k: v[keep] for k, v in rows.items()}


def _every_game_once(rows, c, n_games):
    assert c["games_finished"] == n_games and c["error_slots"] == 0 and c["active_slots"] == 0
    g, m = rows["game_idx"].astype(np.int64), rows["move_idx"].astype(np.int64)
    assert np.array_equal(np.unique(g), np.arange(n_games))
    # the rows are sorted by (game, move): a game played once has the moves 0, 1, 2, ... each once
    first = np.r_[True, g[1:] != g[:-1]]
    assert np.all(m[first] == 0) and np.all(m[~first] == m[np.nonzero(~first)[0] - 1] + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots", [65, 1000, 1025, 2100, 8200])
def test_ordered_list_with_the_cut_changes_only_the_schedule(n_slots):
    """k_order_evals at every chunk and group shape, 8 200 slots being the one with a second group (the rotation wraps by
    itself: it moves with the step); there the refills of the 37 extra games also run k_driver_scan's second group: the rows of
    n_slots + 37 games and the counters equal those of the same games without the cut, bit for bit; only the step count is
    larger.  A second run with the cut takes the same steps and gives the same rows in the same order."""
    n_games = n_slots + 37
    ref, cr = _play(n_slots, n_games, False)
    got, cg = _play(n_slots, n_games, True)
    _every_game_once(got, cg, n_games)
    assert tuple(cg[k] for k in COUNTERS) == tuple(cr[k] for k in COUNTERS)
    _same_rows(ref, got)
    assert cg["steps"] > cr["steps"]  # leaves were put off
    again, ca = _play_again(n_slots, n_games, True)
    _same_rows(got, again)
    assert ca["steps"] == cg["steps"] and tuple(ca[k] for k in COUNTERS) == tuple(cg[k] for k in COUNTERS)


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots,n_games", [(1025, 1000), (65, 300), (8200, 8195)])
def test_games_are_handed_out_in_slot_order(n_slots, n_games):
    """k_driver_flags + k_driver_scan: more slots than games (25 slots of the second chunk go idle; with 8 200 slots the five
    idle ones lie in the second GROUP), and refills in slot order.  Every game is played once, and its rows equal those of the
    same game played on 40 slots (the first 1 000 games where more are played: the 40-slot run is shared)."""
    got, c = _play(n_slots, n_games, True)
    _every_game_once(got, c, n_games)
    ref, cr = _play(40, 1000, False)
    _every_game_once(ref, cr, 1000)
    n = min(n_games, 1000)
    _same_rows(_of_games(ref, n), _of_games(got, n))


@pytest.mark.gpu
def test_both_forms_of_select_play_the_same_games():
    """65 slots: the sixteen-game form of k_select (no cut: it appends to the list itself; four full workgroups and one game
    in the fifth) beside the one-game form (the cut), the same 102 games, the same rows -- and both those of the 40-slot run."""
    a, ca = _play(65, 102, False)
    b, cb = _play(65, 102, True)
    _every_game_once(a, ca, 102)
    _every_game_once(b, cb, 102)
    _same_rows(a, b)
    ref, _ = _play(40, 1000, False)
    _same_rows(_of_games(ref, 102), a)
