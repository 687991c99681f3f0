"""The Gumbel root search with a network evaluator (dbaz_selfplay_set_gumbel on evaluator="resnet"), against tests/gumbel_ref.py.

Which k_select a test launches follows from its parameters alone: NPL, the lanes per child, from the board -- 3x3 (A = 32) 1, 6x6
(98) 2, 8x8 (162) 3, 10x10 (242) 4 --, and ONE, one game per workgroup, from the full-rounds cut: eval_round=16 on more than 16
slots launches k_select<NPL, true, true>, eval_round=-1 the sixteen-game form k_select<NPL, false, true>.  Every board is played
both ways with the same seed: nothing but the schedule may differ -- put-off leaves (S->pending) under a Gumbel root must not run
the root's pre-pass again -- and a subset of the games, fixed here, is replayed on the reference with the engine of the cut run as
the evaluator, asked one position at a time.  g comes from Philox, the engine picks its own moves, the noise setting must not be
mixed in, the tree is reused and the transposition cache is on (and, once more, off: it must be transparent).

Zero priors: the same 3x3 network with the bias of the policy head's last layer at -200 on half of the actions.  Its softmax is
exactly 0 there, so a valid child with P == 0 is no candidate while a sibling has P > 0, and a root without any positive prior
(root_prep's cpsum == 0 branch) has every valid child as a candidate at the logit -1e30: exact ties, the first index wins.

visits are compared within +-1 count per entry (device and host exp / log), everything else bit for bit; the
largest difference seen is printed per case.  The gap condition is asserted on the replayed games themselves."""
import numpy as np
import pytest

from oracle import oracle as O
import endgame_ref as ER
import gumbel_ref as GR
from test_hip_gumbel import game_rows, played
from test_hip_gumbel_features import compare_game

pytestmark = pytest.mark.gpu

CAP = (0.5, 8)
NPL = {(3, 3): 1, (6, 6): 2, (8, 8): 3, (10, 10): 4}
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


def replay(e, R, C, got, game_idxs, what, *, sims, gumbel, cap=None, record=False):
    """the games game_idxs on the reference, the engine e as the evaluator; each game depends on (seed, game_idx) alone"""
    d = O.dims(R, C)
    ev = asks(e, R, C)
    worst, out = 0, []
    for gi in game_idxs:
        kw = dict(g_mode="philox", game_idx=gi, seed=GR.SEED, sims=sims, reuse=True, gumbel=gumbel, cap=cap, base_ev=ev)
        g, roots = GR.play_recording_roots(d, **kw) if record else (GR.play_game(d, **kw), None)
        worst = max(worst, compare_game(game_rows(got, gi), g, (what, "game", gi)))
        out.append((g, roots))
    gap = min(g["min_gap"] for g, _ in out)
    print("%s: %d games replayed, largest difference in counts %d, minimum gap %g, tied roots %d"
          % (what, len(out), worst, gap, sum(g["n_tied_roots"] for g, _ in out)))
    assert gap >= 1e-9, what  # no decision of the replayed games is near a tie that a last bit of log could turn
    return out


_off_rows = {}  # (R, C) -> the rows of the run without the cut, for the run without the transposition cache

# R, C, m, cap, nn_precision (None: the network's own, 1)
CASES = [(3, 3, 16, None, None), (3, 3, 16, None, 0), (3, 3, 4, CAP, None), (6, 6, 16, None, None), (8, 8, 16, None, None), (10, 10, 16, None, None)]


@pytest.mark.parametrize("R,C,m,cap,precision", CASES)
def test_both_forms_of_k_select_against_the_reference(R, C, m, cap, precision):
    """k_select<NPL, true, true> (the cut) and k_select<NPL, false, true> (no cut), NPL = NPL[(R, C)]: the same rows, and the
    reference's"""
    n = GR.NET[(R, C)]
    what = "%dx%d (NPL %d) m %d%s precision %s" % (R, C, NPL[(R, C)], m, " cap" if cap else "", precision)
    gumbel = (m, GR.C_VISIT, GR.C_SCALE)
    model = GR.network(R, C)
    assert n["slots"] > 16 and n["slots"] % 16
    runs = []
    for kw in (NO_CUT, CUT):
        e = net_engine(R, C, n["slots"], n["sims"], gumbel, model, precision, playout_cap=cap, **kw)
        c, gm, got = played(e, n["slots"])
        runs.append((c, gm, e.playout_cap(), got))
        if kw is NO_CUT:
            e.close()
    (co, go, po, off), (cc, gc, pc, cut) = runs
    try:
        same_rows(cut, off, what + ": the cut against no cut")
        assert cc["steps"] > co["steps"]
        for k in COUNTERS:
            assert cc[k] == co[k], k
        assert gc == go and pc == po and gc["rows"] == gc["searches"] == len(cut["played"])
        assert cc["cache_hits"] > 0 and cc["f32_fallback_evals"] == 0 and co["f32_fallback_evals"] == 0
        if cap is not None:
            assert not cut["full"].all() and cut["full"].any()
        replay(e, R, C, cut, n["replay"], what, sims=n["sims"], gumbel=gumbel, cap=cap)
    finally:
        e.close()
    if m == 16 and precision is None:
        _off_rows[(R, C)] = (off, co)


@pytest.mark.parametrize("R,C", [(3, 3), (6, 6)])
def test_transposition_cache_is_transparent(R, C):
    if (R, C) not in _off_rows:
        test_both_forms_of_k_select_against_the_reference(R, C, 16, None, None)
    want, cw = _off_rows[(R, C)]
    n = GR.NET[(R, C)]
    e = net_engine(R, C, n["slots"], n["sims"], (16, GR.C_VISIT, GR.C_SCALE), GR.network(R, C), transposition_cache=False, **NO_CUT)
    c, gm, got = played(e, n["slots"])
    e.close()
    same_rows(got, want, "%dx%d without the transposition cache" % (R, C))
    assert c["cache_hits"] == 0 and c["f32_fallback_evals"] == 0 and c["nn_evals"] == cw["nn_evals"] + cw["cache_hits"]


def test_zero_priors_against_the_reference():
    R = C = 3
    gumbel = (16, GR.C_VISIT, GR.C_SCALE)
    e = net_engine(R, C, 16, 32, gumbel, GR.network(R, C, zero=True))
    try:
        d = O.dims(R, C)
        p = e.predict(O.features(d, O.new_state(d)).astype(np.float32).reshape(1, 3, R + 1, C + 1))[0][0]
        zero = list(GR.NET_ZERO)
        assert (p[zero] == 0).all() and (np.delete(p, zero) > 0).all()  # exactly 0 on Z, positive elsewhere
        c, gm, got = played(e, 16)
        assert c["f32_fallback_evals"] == 0
        out = replay(e, R, C, got, GR.NET_ZERO_REPLAY, "3x3 zero priors", sims=32, gumbel=gumbel, record=True)
    finally:
        e.close()
    assert len(out) >= 4
    kinds = [GR.zero_prior_roots(g, roots, GR.NET_ZERO) for g, roots in out]  # asserts the rule on every root of either kind
    print("3x3 zero priors: (roots with both kinds of child, roots without a positive prior, a change inside the game) per game", kinds)
    assert sum(k[0] for k in kinds) > 0 and sum(k[1] for k in kinds) > 0 and any(k[2] for k in kinds)
    assert sum(g["n_tied_roots"] for g, _ in out) > 0
    # and the engine's own rows say the same of the games that were not replayed
    acts, _ = ER.board(R, C)
    vis = got["visits"]
    for i in range(len(vis)):
        valid = [int(a) for a in acts if got["x"][i][a] == 0]
        pos = [a for a in valid if a not in GR.NET_ZERO]
        z = [a for a in valid if a in GR.NET_ZERO]
        if pos:
            assert not vis[i][z].any() and got["played"][i] not in z, i
        else:
            assert got["played"][i] == z[0] and len(set(vis[i][z])) == 1 and vis[i].sum() == vis[i][z].sum(), i
