"""The full mode of the Gumbel search with a network evaluator, against tests/gumbel_full_ref.py.

Which k_select a test launches follows from its parameters alone: NPL, the lanes per child, from the board -- 3x3 1, 6x6 2, 8x8 3,
10x10 4 --, and ONE, one game per workgroup, from the full-rounds cut: eval_round=16 on more than 16 slots launches
k_select<NPL, true, 2>, eval_round=-1 the sixteen-game form k_select<NPL, false, 2>.  Every board is played both ways with the same
seed: nothing but the schedule may differ -- a put-off leaf under interior Gumbel picks keeps its path, and the value a transposition
hit copies from its twin is the number the twin's own expansion stored -- and a subset of the games, fixed in gumbel_full_ref.NET, is
replayed on the reference with the engine of the cut run as the evaluator, asked one position at a time.  The transposition cache is
on (the network's default); g comes from Philox and the engine picks its own moves.

visits are compared within +-1 count per entry, everything else bit for bit.  The gap condition is asserted on the replayed games
themselves, interior picks included."""
import numpy as np
import pytest

from oracle import oracle as O
import gumbel_full_ref as GF
import gumbel_ref as GR
from test_hip_gumbel_full import compare, game_rows, played

pytestmark = pytest.mark.gpu

CUT, NO_CUT = dict(eval_round=16, eval_defer_max=15), dict(eval_round=-1)
COUNTERS = ("expansions", "nn_evals", "cache_hits", "games_finished", "terminal_leaves")


def asks(e, R, C):
    """the reference's evaluator: the same engine, one position at a time, memoised (a sample's result does not depend on its batch)"""
    memo = {}

    def hip_net(dd, st):
        x = O.features(dd, st)
        key = x.tobytes()
        if key not in memo:
            pv = e.predict(x.astype(np.float32).reshape(1, 3, R + 1, C + 1))
            memo[key] = (pv[0][0].copy(), pv[1][0].copy())
        return memo[key]
    return hip_net


def net_engine(R, C, n_slots, sims, gumbel, model, precision=None, **kw):
    from dotsboxesaz_amd.engine import Engine
    e = Engine(R, C, n_slots, mcts_num_read=sims, noise=GR.NOISE, reuse_tree=True, evaluator="resnet", seed=GR.SEED, gumbel=gumbel,
               nn_precision=precision, **kw)
    e.load_state_dict(model.state_dict(), "resnet", **model.shape)
    return e


def same_rows(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (what, k)


# R, C, nn_precision (None: the network's own, 1)
CASES = [(3, 3, None), (3, 3, 0), (6, 6, None), (8, 8, None), (10, 10, None)]


@pytest.mark.parametrize("R,C,precision", CASES)
def test_both_forms_of_k_select_against_the_reference(R, C, precision):
    n = GF.NET[(R, C)]
    what = "%dx%d m %d precision %s" % (R, C, n["m"], precision)
    gumbel = (n["m"], GR.C_VISIT, GR.C_SCALE, True)
    model = GF.network(R, C)
    assert n["slots"] > 16 and n["slots"] % 16 and n["m"] < n["sims"]
    runs = []
    for kw in (NO_CUT, CUT):
        e = net_engine(R, C, n["slots"], n["sims"], gumbel, model, precision, **kw)
        c, gm, got = played(e, n["slots"])
        runs.append((c, gm, got))
        if kw is NO_CUT:
            e.close()
    (co, go, off), (cc, gc, cut) = runs
    try:
        same_rows(cut, off, what + ": the cut against no cut")
        assert cc["steps"] > co["steps"]  # leaves were put off
        for k in COUNTERS:
            assert cc[k] == co[k], k
        assert gc == go and gc["full"] and gc["rows"] == gc["searches"] == len(cut["played"])
        assert cc["cache_hits"] > 0 and cc["f32_fallback_evals"] == 0 and co["f32_fallback_evals"] == 0
        d = O.dims(R, C)
        ev = asks(e, R, C)
        games = {gi: GF.play_game(d, g_mode="philox", game_idx=gi, seed=GR.SEED, sims=n["sims"], reuse=True, gumbel=gumbel[:3], base_ev=ev)
                 for gi in n["replay"]}
    finally:
        e.close()
    sub = {k: np.concatenate([game_rows(cut, gi)[k] for gi in n["replay"]]) for k in cut}
    sub["game_idx"] = np.concatenate([np.full(len(game_rows(cut, gi)["played"]), j) for j, gi in enumerate(n["replay"])])
    worst = compare([games[gi] for gi in n["replay"]], sub)
    gap = min(g["min_gap"] for g in games.values())
    print("%s: %d games replayed, largest difference in counts %d, minimum gap %g, interior picks %d (%d at depth >= 3)"
          % (what, len(games), worst, gap, sum(g["interior_picks"] for g in games.values()), sum(g["deep_picks"] for g in games.values())))
    assert gap >= 1e-9, what  # no decision of the replayed games is near a tie that a last bit of log or exp could turn
    assert sum(g["interior_picks"] for g in games.values()) > 0
