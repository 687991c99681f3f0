"""endgame_selfplay_ref.py, the oracle replay of self-play with a table inside the search, pinned on the CPU: without a table it is
O.play_game; its threshold, its reused subtree at the first served move and its choice of evaluator per SEARCH ROOT change the
rows of most games (so the GPU comparison in test_hip_endgame_selfplay.py would notice either mistake); and with fresh roots it
has the property the other endgame tests check -- the solved result and optimal moves from the first served row on."""
import numpy as np
import pytest

from oracle import oracle as O
import endgame_policy_ref as PR
import endgame_selfplay_ref as SR


def same(a, b):
    return SR.rows_differ(a, b) < 0


@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("R,C,sims", [(3, 3, 40), (4, 4, 24), (2, 3, 50)])
def test_without_a_table_the_replay_is_play_game(R, C, sims, reuse):
    d = O.dims(R, C)
    pp = O.selfplay_params(sims, noise=(0.0, 0.0), reuse_tree=reuse)
    for g in range(6):
        ref = O.play_game(d, pp, O.Evaluator(0), rng_state=1000 + 17 * g)
        got = SR.replay_game(d, ref, 0, SR.Table(R, C, -1), sims=sims, reuse=reuse)
        assert got["n_rows"] == ref["n_rows"] and got["mismatch"] < 0
        assert np.array_equal(got["played"], ref["played"]) and np.array_equal(got["x"], ref["x"])
        assert np.array_equal(got["player"], ref["player"]) and np.array_equal(got["visits"], ref["visits"])
        assert np.array_equal(got["pi"].view(np.uint64), ref["pi"].view(np.uint64))
        assert np.array_equal(got["q_value"].view(np.uint32), ref["q_value"].view(np.uint32))
        for k in ("tree_size", "terminal_count", "max_deepness", "z"):
            assert np.array_equal(got[k], ref[k]), k
        assert same(got, ref)
        # the counts: every search, root expansions included, and an evaluator call for each that did not end in a finished game
        assert got["n_search"] == ref["n_search"] and got["table_calls"] == 0 and got["first_served"] == -1 and not got["served"].any()
        if not reuse:  # (a reused tree keeps its terminal_count only until the next re-root: no such sum)
            assert got["base_calls"] == got["n_search"] - got["terminal_count"].sum()
        plain = SR.replay_game(d, ref, 0, None, sims=sims, reuse=reuse)
        assert same(plain, ref) and plain["base_calls"] == got["base_calls"]


# games generated WITH the table: (board, max_free, reads, seed of the moves).  The seeds are fixed so that the conditions below
# hold; they are conditions on these inputs, computed by the reference alone.
CASES = [(4, 4, 12, 24, 5), (3, 3, 8, 40, 11)]
_games = {}


def generated(R, C, M, sims, seed, reuse=True):
    key = (R, C, M, sims, seed, reuse)
    if key not in _games:
        d, rs = O.dims(R, C), np.random.RandomState(seed)
        _games[key] = [SR.generate_game(d, rs, 0, SR.Table(R, C, M, seed=3), sims=sims, reuse=reuse) for _ in range(8)]
    return _games[key]


@pytest.mark.parametrize("R,C,M,sims,seed", CASES)
def test_threshold_and_reused_subtree_change_the_rows(R, C, M, sims, seed):
    d = O.dims(R, C)
    games = generated(R, C, M, sims, seed)
    changed = {"table off": 0, "max_free + 1": 0, "max_free - 1": 0, "fresh root at the first served move": 0, "leaf's own F": 0}
    for g in games:
        assert g["first_served"] >= 0 and g["base_calls"] > 0
        # the served searches are exactly those of the rows with F <= max_free, and the first of them has a reused, expanded root
        assert np.array_equal(g["served"], g["n_free"] <= M) and g["n_free"][g["first_served"]] == M
        assert np.array_equal(SR.free_edges(R, C, g["x"]), g["n_free"])
        again = SR.replay_game(d, g, 0, SR.Table(R, C, M, seed=3), sims=sims, reuse=True)
        assert same(again, g) and (again["base_calls"], again["table_calls"]) == (g["base_calls"], g["table_calls"])
        changed["table off"] += not same(SR.replay_game(d, g, 0, None, sims=sims, reuse=True), g)
        changed["max_free + 1"] += not same(SR.replay_game(d, g, 0, SR.Table(R, C, M + 1, seed=3), sims=sims, reuse=True), g)
        changed["max_free - 1"] += not same(SR.replay_game(d, g, 0, SR.Table(R, C, M - 1, seed=3), sims=sims, reuse=True), g)
        changed["fresh root at the first served move"] += not same(
            SR.replay_game(d, g, 0, SR.Table(R, C, M, seed=3), sims=sims, reuse=True, fresh_at_first_served=True), g)
        # the evaluator chosen by the LEAF's free edges instead of the root's: a leaf with F <= max_free under an earlier root
        table = SR.SlotTablesRef(R, C, g["x"][g["first_served"]][None], 3, M)

        def by_leaf(dd, st, table=table):
            x = O.features(dd, st).ravel()
            a, v, served = table.one(x)
            if not served or a < 0:
                return O.eval_formula(dd, st, 0)
            p = np.zeros(dd.A, np.float32)
            p[a] = 1.0
            return p, np.float32(v)
        changed["leaf's own F"] += not same(SR.replay_game(d, g, by_leaf, None, sims=sims, reuse=True), g)
    print("%dx%d max_free %d, %d reads: games of 8 whose rows change: %s" % (R, C, M, sims, changed))
    assert any(g["root_expanded"][g["first_served"]] and g["tree_size"][g["first_served"]] > 1 for g in games)
    assert sum(g["table_calls"] > 0 for g in games) >= 4  # (a late 3x3 search may end every read in a finished game)
    for what, n in changed.items():
        assert n >= 4, (what, n)


@pytest.mark.parametrize("R,C,M,sims,seed", CASES)
def test_fresh_roots_keep_the_solved_result_and_play_optimal_moves(R, C, M, sims, seed):
    games = generated(R, C, M, sims, seed, reuse=False)
    kept = 0
    for g in games:
        f = g["first_served"]
        assert f >= 0 and g["mismatch"] < 0
        for i in range(f, g["n_rows"]):
            value = PR.solved_row(R, C, g["x"][i])["value"]
            assert int(g["z"][i]) == value, i
            if value >= 0:
                pi = g["pi"][i]
                assert pi.max() == 1.0 and (pi != 0).sum() == 1 and int(pi.argmax()) in PR.optimal_set(R, C, g["x"][i]), i
                assert int(g["played"][i]) == int(pi.argmax())
                kept += 1
    assert kept >= 8 * 2  # (a condition on the generated games: rows the property speaks about)


def test_dry_pool_and_read_cap_and_match_models():
    """served_from, endgame_reads and models: the rows before the first served move are the plain game's, the cap applies to
    served searches only, and in match play only the moves of a model in endgame_models are served"""
    R, C, M, sims = 4, 4, 12, 24
    d = O.dims(R, C)
    g = generated(R, C, M, sims, 5)[0]
    f = g["first_served"]
    late = SR.replay_game(d, g, 0, SR.Table(R, C, M, seed=3), sims=sims, reuse=True, served_from=f + 2, stop_at_mismatch=True)
    assert late["mismatch"] in (f, f + 1) and not late["served"].any()
    never = SR.replay_game(d, g, 0, SR.Table(R, C, M, seed=3), sims=sims, reuse=True, served_from=SR.NEVER)
    plain = SR.replay_game(d, g, 0, None, sims=sims, reuse=True)
    assert same(never, plain) and never["table_calls"] == 0
    capped = SR.generate_game(d, np.random.RandomState(2), 0, SR.Table(R, C, M, seed=3), sims=sims, reuse=True, endgame_reads=3)
    assert (capped["reads"][capped["served"]] == 3).all() and (capped["reads"][~capped["served"]] == sims).all()
    both = [0, 0]
    for game_idx in range(6):
        m = SR.generate_game(d, np.random.RandomState(4 + game_idx), None, SR.Table(R, C, M, seed=3), sims=sims, reuse=True,
                             models=(1, 0, (0,)), game_idx=game_idx)
        model = m["player"] ^ (game_idx & 1)
        assert np.array_equal(m["served"], (m["n_free"] <= M) & (model == 0))
        both[0] += int(m["served"].sum())
        both[1] += int((~m["served"] & (m["n_free"] <= M)).sum())
        rows = dict(m, game_idx=np.full(m["n_rows"], game_idx))
        again = SR.replay_game(d, rows, None, SR.Table(R, C, M, seed=3), sims=sims, reuse=True, models=(1, 0, (0,)))
        assert same(again, m) and again["table_calls"] == m["table_calls"]
    assert both[0] >= 6 and both[1] >= 6  # late moves of either model
