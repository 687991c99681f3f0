"""Exact endgames at the leaves (dbaz_attach_leaf_solver; select_one's SEL_LEAF_SOLVE branch in both forms of k_select, k_select_multi,
k_expand_backup(_multi) in csrc/tree.hip; k_endgame_leaves in csrc/endgame.hip; the launch next to endgame_eval_leaves in
csrc/engine.hip), bit for bit against the oracle.

Every game the engine played -- moves sampled on the device, no noise -- is replayed move by move through leaf_solve_ref.py: the
oracle's tree, the evaluator of every search no table serves wrapped so that an unfinished leaf with F <= L gets the (p, v) of its
own solved table, whatever the root.  Every compared row must equal the oracle's in x, player, visits, pi, q, TreeStats and z, and
the device's counters the replay's: a solved leaf is no evaluation (nn_evals), no cache hit, and is counted per F."""
import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.endgame import DeepTables, Endgame
import endgame_selfplay_ref as SR
import leaf_solve_ref as LR

pytestmark = pytest.mark.gpu

SEED = 3  # endgame_seed: which of several optimal moves gets the prior
CLASSES = ((16, 16), (14, 15), (11, 13), (0, 10))  # the launch plan: one launch per class of F that L reaches


def game_rows(got, gi):
    r = np.nonzero(got["game_idx"] == gi)[0]
    assert list(got["move_idx"][r]) == list(range(len(r))), gi
    return {k: v[r] for k, v in got.items()}


def assert_rows(ref, rows, what):
    """every compared field of a replayed game, bit for bit"""
    assert ref["mismatch"] < 0 and ref["n_rows"] == len(rows["played"]), what
    assert np.array_equal(ref["x"], rows["x"]), what
    assert np.array_equal(ref["player"], rows["player"]), what
    for i in range(ref["n_rows"]):  # row by row: the message names the first move that differs
        assert np.array_equal(ref["visits"][i], rows["visits"][i]), (what, i, "visits", bool(ref["served"][i]), int(ref["n_free"][i]))
    assert np.array_equal(ref["pi"].view(np.uint64), np.ascontiguousarray(rows["pi"], np.float64).view(np.uint64)), what
    assert np.array_equal(ref["q_value"].view(np.uint32), np.ascontiguousarray(rows["q_value"], np.float32).view(np.uint32)), what
    assert np.array_equal(ref["tree_size"], rows["tree_size"]), what
    assert np.array_equal(ref["terminal_count"], rows["terminal_count"]), what
    assert np.array_equal(ref["max_deepness"], rows["max_deepness"].astype(np.int64)), what
    assert np.array_equal(ref["z"], rows["z"].astype(np.int64)), what
    assert SR.rows_differ(ref, rows) < 0, what


def same_rows(got, want, what):
    assert set(got) == set(want), what
    for k in got:
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, k)


def finished(e, n_games):
    c = e.counters()
    assert c["games_finished"] == n_games and c["error_slots"] == 0 and c["active_slots"] == 0 and c["pool_resets"] == 0
    got = e.fetch_samples()
    assert sorted(set(got["game_idx"])) == list(range(n_games))  # every game finished once
    return c, got


def replay(got, games, d, w, table, what, *, sims, reuse, **kw):
    """replays `games` through the wrapper w (one for all of them: it sums the calls); returns the sums"""
    tot = dict(games=0, table=0, n_search=0, served_games=0)
    for gi in games:
        rows = game_rows(got, gi)
        ref = LR.replay(d, rows, w, table, sims=sims, reuse=reuse, **kw)
        assert_rows(ref, rows, (what, "game", int(gi)))
        tot["games"] += 1
        tot["table"] += ref["table_calls"]
        tot["n_search"] += ref["n_search"]
        tot["served_games"] += bool(ref["served"].any())
    return tot


def reached(L):
    return [c for c in CLASSES if c[0] <= L]


def assert_leaf_preconditions(w, L, n_games, what):
    """the case solves leaves where no table attach would: under roots with F > L in a quarter of the games, and in every class of
    F whose launch the threshold asks for"""
    high = w.solved_under_high_roots()
    assert len(high) == n_games and 4 * sum(1 for h in high if h > 0) >= n_games, (what, high)
    for lo, hi in reached(L):
        assert sum(w.by_free[max(lo, 1):min(hi, L) + 1]) > 0, (what, (lo, hi), w.by_free)


# ---------------------------------------------------------------- 1. formula self-play, the leaf solver alone
FORMULA = [(3, 3, 6, 16, 32, 40), (4, 4, 8, 32, 32, 24), (2, 7, 7, 16, 16, 24),
           (4, 6, 12, 16, 16, 24),  # 70 actions: two key words
           (6, 6, 16, 8, 16, 30)]
_replayed = {}  # (R, C, reuse) -> the rows and the replay's sums: the transposition table changes no row


@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("tt", [True, "force"])
@pytest.mark.parametrize("R,C,L,n_slots,n_games,sims", FORMULA)
def test_formula_selfplay_with_the_leaf_solver_vs_oracle(R, C, L, n_slots, n_games, sims, tt, reuse):
    from dotsboxesaz_amd.engine import Engine
    what = "%dx%d leaf solver L %d, %d reads, tt=%s, reuse=%s" % (R, C, L, sims, tt, reuse)
    h = Endgame(R, C, max_free=16 if (R + C) % 2 else L)  # the handle's max_free: the threshold itself, or above it
    e = Engine(R, C, n_slots, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=reuse, evaluator="formula", seed=1234, transposition_cache=tt,
               leaf_endgame=h, leaf_free=L if (R + C) % 2 else None, endgame_seed=SEED)
    e.selfplay_start(n_games, 0)
    e.run()
    c, got = finished(e, n_games)
    ls, stats = e.leaf_solves(), e.endgame_stats()
    e.close()
    h.close()
    if (R, C, reuse) in _replayed:
        want, w, tot = _replayed[(R, C, reuse)]
        same_rows(got, want, what)
    else:
        w = LR.LeafSolver(R, C, L, SEED, 0)
        tot = replay(got, range(n_games), O.dims(R, C), w, None, what, sims=sims, reuse=reuse)
        _replayed[(R, C, reuse)] = (got, w, tot)
    print("%s: %d games, %d leaves solved by F %s, %d of them under roots with F > L; base calls %d; device: nn_evals %d, cache_hits %d"
          % (what, n_games, w.calls["solved"], w.by_free[:L + 1], sum(w.solved_under_high_roots()), w.calls["base"], c["nn_evals"], c["cache_hits"]))
    assert_leaf_preconditions(w, L, n_games, what)
    assert c["expansions"] == tot["n_search"]
    assert c["nn_evals"] + c["cache_hits"] == w.calls["base"]
    assert (c["cache_hits"] > 0) == (tt == "force")
    assert ls["by_free"] == w.by_free and ls["total"] == w.calls["solved"]
    assert stats == (0, 0) and tot["table"] == 0


# ---------------------------------------------------------------- 2. next to a table
def table_engine(kind, M, L, n_slots, tables=None, R=4, C=4, sims=24):
    from dotsboxesaz_amd.engine import Engine
    if kind == "endgame":
        h = Endgame(R, C, max_free=M)
        leaf = h if L <= M else Endgame(R, C, max_free=L)  # the same handle serves both attaches where it can
    else:
        h, leaf = DeepTables(R, C, max_free=M), Endgame(R, C, max_free=L)
    e = Engine(R, C, n_slots, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=True, evaluator="formula", seed=1234, transposition_cache="force",
               endgame=h, endgame_seed=SEED, endgame_tables=tables, leaf_endgame=leaf, leaf_free=L)
    return e, {h, leaf}


@pytest.mark.parametrize("kind,M,L,tables", [("endgame", 12, 11, None), ("endgame", 8, 12, None), ("deep", 12, 11, 32)])
def test_leaf_solver_next_to_a_table_vs_oracle(kind, M, L, tables):
    R, C, sims, n_games = 4, 4, 24, 32
    what = "4x4 %s(%d)%s + leaf solver L %d" % (kind, M, " pooled" if tables else "", L)
    e, handles = table_engine(kind, M, L, 32, tables)
    e.selfplay_start(n_games, 0)
    e.run()
    c, got = finished(e, n_games)
    ls, stats, pool = e.leaf_solves(), e.endgame_stats(), e.table_pool()
    e.close()
    for h in handles:
        h.close()
    w = LR.LeafSolver(R, C, L, SEED, 0)
    tot = replay(got, range(n_games), O.dims(R, C), w, SR.Table(R, C, M, SEED), what, sims=sims, reuse=True)
    print("%s: %d table calls in %d games, %d leaves solved by F %s, %d base calls; device: %s, nn_evals %d, cache_hits %d"
          % (what, tot["table"], tot["served_games"], w.calls["solved"], w.by_free[:L + 1], w.calls["base"], stats, c["nn_evals"], c["cache_hits"]))
    assert stats == (tot["served_games"], tot["table"]) and tot["table"] > 0
    assert ls["by_free"] == w.by_free and ls["total"] == w.calls["solved"] > 0
    assert c["expansions"] == tot["n_search"] and c["nn_evals"] + c["cache_hits"] == w.calls["base"]
    if tables:
        assert pool["denied"] == 0 and pool["in_use"] == 0


def test_leaf_solver_under_a_dry_pool_vs_oracle():
    """One region for 8 slots, deny mode: a denied slot searches without a table and still gets its leaves with F <= 11 solved.
    Which searches were denied is the schedule's, and with L one below the tables' threshold the rows cannot tell: a denied
    search differs from a served one in its root expansion alone.  So the device is asked: the run goes step by step, and a
    slot's header (dbaz_get_slot_table), read after every step, names the game its table serves and the free edges F0 of the
    root it was solved at -- a game's first served move is 40 - F0.  Replayed with exactly that move, every count is equal."""
    import ctypes as C
    R, C_, M, L, sims, n_games, n_slots = 4, 4, 12, 11, 24, 16, 8
    d, E = O.dims(R, C_), 2 * R * C_ + R + C_
    e, handles = table_engine("deep", M, L, n_slots, 1)
    e.selfplay_start(n_games, 0)
    served_from = {}  # game -> its first served move
    valid, n_free, game = C.c_int32(), C.c_int32(), C.c_int64()
    for _ in range(100000):
        e.step(1)
        for slot in range(n_slots):
            e._ck(e._L.dbaz_get_slot_table(e.h, slot, C.byref(valid), C.byref(n_free), C.byref(game), None, None, 0, 0))
            if valid.value:
                assert served_from.setdefault(int(game.value), E - int(n_free.value)) == E - int(n_free.value)  # one table per game
        if e.counters()["active_slots"] == 0:
            break
    c, got = finished(e, n_games)
    ls, stats, pool = e.leaf_solves(), e.endgame_stats(), e.table_pool()
    e.close()
    for h in handles:
        h.close()
    table = SR.Table(R, C_, M, SEED)
    w = LR.LeafSolver(R, C_, L, SEED, 0)
    tot = dict(table=0, n_search=0, denied=0, solved_when_denied=0, served_late=0)
    for gi in range(n_games):
        rows = game_rows(got, gi)
        n, left = len(rows["played"]), SR.free_edges(R, C_, rows["x"])
        first = int(np.nonzero(left <= M)[0][0]) if left.min() <= M else n
        g = served_from.get(gi, n)
        assert first <= g <= n and (g == n or left[g] <= M), (gi, first, g, n)
        ref = LR.replay(d, rows, w, table, sims=sims, reuse=True, served_from=g if g < n else SR.NEVER)
        assert_rows(ref, rows, ("dry pool", gi, "first served move", g))
        assert ref["first_served"] == (g if g < n else -1), (gi, g, ref["first_served"])
        tot["table"] += ref["table_calls"]
        tot["n_search"] += ref["n_search"]
        tot["denied"] += g - first  # every search from the first eligible root to the first served one asked and got nothing
        tot["solved_when_denied"] += sum(w.games[-1]["solved"][first:g])
        tot["served_late"] += first < g < n
    print("dry pool of 1 table, %d slots, %d games: %s, endgame_stats %s, leaves solved %d by F %s; first served moves %s; the replay: %s"
          % (n_slots, n_games, pool, stats, ls["total"], ls["by_free"][:L + 1], served_from, tot))
    assert stats == (len(served_from), tot["table"]) and tot["table"] > 0
    assert ls["by_free"] == w.by_free and ls["total"] == w.calls["solved"] > 0
    assert pool["denied"] == tot["denied"] > 0 and pool["high_water"] == 1 and pool["in_use"] == 0
    assert c["expansions"] == tot["n_search"] and c["nn_evals"] + c["cache_hits"] == w.calls["base"]
    # the case's preconditions: a denied slot gets its leaves solved, a game gets its table later than it first asked, one never
    assert tot["solved_when_denied"] > 0 and tot["served_late"] > 0 and len(served_from) < n_games


# ---------------------------------------------------------------- 3. waves
@pytest.mark.parametrize("K", [3, 8])
def test_selfplay_in_waves_with_the_leaf_solver_vs_oracle(K):
    from dotsboxesaz_amd.engine import Engine
    R, C, L, sims, n_games = 4, 4, 10, 24, 16
    what = "4x4 leaf solver L %d in waves of %d" % (L, K)
    h = Endgame(R, C, max_free=L)
    e = Engine(R, C, 8, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=True, evaluator="formula", seed=3, max_pending_evals=K,
               selfplay_pending=True, leaf_endgame=h, endgame_seed=SEED)
    e.selfplay_start(n_games, 0)
    e.run()
    c, got = finished(e, n_games)
    ls = e.leaf_solves()
    e.close()
    h.close()
    w = LR.LeafSolver(R, C, L, SEED, 0)
    tot = replay(got, range(n_games), O.dims(R, C), w, None, what, sims=sims, reuse=True, K=K)
    print("%s: %d leaves solved by the replay, %d on the device; base calls %d, nn_evals %d, cache_hits %d"
          % (what, w.calls["solved"], ls["total"], w.calls["base"], c["nn_evals"], c["cache_hits"]))
    assert_leaf_preconditions(w, L, n_games, what)
    assert c["expansions"] == tot["n_search"]
    # a leaf that an earlier simulation of its wave already holds is answered once on the device (counted in cache_hits, whichever
    # way the first was answered) and once per simulation by the oracle's wave search: only the sum is comparable
    assert c["nn_evals"] + c["cache_hits"] + ls["total"] == w.calls["base"] + w.calls["solved"]
    assert 0 < ls["total"] <= w.calls["solved"] and c["nn_evals"] <= w.calls["base"]
    assert all(a <= b for a, b in zip(ls["by_free"], w.by_free))


# ---------------------------------------------------------------- 4. the network evaluator, transposition table on
def network(R, C):
    import torch
    from oracle import nn_ref
    torch.manual_seed(R * 10 + 2)
    m = nn_ref.ResNetZeroRef(R, C, 64, 2)
    nn_ref.randomize_bn(m, 3)
    return m


def network_engine(R, C, n_slots, sims, L, precision, **kw):
    from dotsboxesaz_amd.engine import Engine
    h = Endgame(R, C, max_free=L)
    e = Engine(R, C, n_slots, mcts_num_read=sims, noise=(0.0, 0.0), evaluator="resnet", seed=5, nn_precision=precision, leaf_endgame=h,
               endgame_seed=SEED, **kw)
    e.load_state_dict(network(R, C).state_dict(), "resnet", 64, 2, 16, 8)
    return e, h


def asks(e, R, C):
    """the oracle's base evaluator: the same engine, one position at a time, memoised (a sample's result does not depend on its
    batch, utils/proxies.py:35-43)"""
    memo = {}

    def hip_net(dd, st):
        x = O.features(dd, st)
        key = x.tobytes()
        if key not in memo:
            pv = e.predict(x.astype(np.float32).reshape(1, 3, R + 1, C + 1))
            memo[key] = (pv[0][0].copy(), pv[1][0].copy())
        return memo[key]
    return hip_net


@pytest.mark.parametrize("R,C,L,n_slots,n_games,sims,precision", [(3, 3, 6, 16, 32, 40, 0), (3, 3, 6, 16, 32, 40, 1), (6, 6, 16, 8, 4, 40, 1)])
def test_network_selfplay_with_the_leaf_solver_vs_oracle(R, C, L, n_slots, n_games, sims, precision):
    what = "%dx%d network, precision %d, leaf solver L %d, %d reads" % (R, C, precision, L, sims)
    e, h = network_engine(R, C, n_slots, sims, L, precision)
    e.selfplay_start(n_games, 0)
    e.run()
    c, got = finished(e, n_games)
    ls = e.leaf_solves()
    assert c["f32_fallback_evals"] == 0
    w = LR.LeafSolver(R, C, L, SEED, asks(e, R, C))
    tot = replay(got, range(n_games), O.dims(R, C), w, None, what, sims=sims, reuse=True)
    print("%s: %d games replayed, %d leaves solved by F %s, base calls %d; device: leaves %d, nn_evals %d, cache_hits %d"
          % (what, tot["games"], w.calls["solved"], w.by_free[:L + 1], w.calls["base"], ls["total"], c["nn_evals"], c["cache_hits"]))
    assert w.calls["solved"] > 0 and w.calls["base"] > 0 and sum(w.solved_under_high_roots()) > 0
    assert c["nn_evals"] + c["cache_hits"] == w.calls["base"] and ls["by_free"] == w.by_free and c["expansions"] == tot["n_search"]
    e.close()
    h.close()


def test_full_rounds_cut_with_the_leaf_solver():
    """solved leaves go through k_select<NPL, true> while other slots hold put-off leaves: a solved leaf is never deferred, and
    nothing but the schedule may change"""
    R, C, L, sims, n_games = 3, 3, 6, 40, 77
    runs = []
    for er, ed in ((16, 15), (-1, 0), (16, 15)):
        e, h = network_engine(R, C, 40, sims, L, 1, reuse_tree=True, eval_round=er, eval_defer_max=ed)
        e.selfplay_start(n_games, 0)
        e.run()
        c, got = finished(e, n_games)
        runs.append((got, c, e.leaf_solves()))
        if len(runs) == 1:  # 8 of the games against the oracle, while the engine can still be asked
            w = LR.LeafSolver(R, C, L, SEED, asks(e, R, C))
            tot = replay(got, range(0, n_games, 10), O.dims(R, C), w, None, "3x3 network with the cut", sims=sims, reuse=True)
            assert tot["games"] == 8 and w.calls["solved"] > 0 and sum(w.solved_under_high_roots()) > 0
        e.close()
        h.close()
    (cut, cc, lc), (off, co, lo), (again, ca, la) = runs
    same_rows(off, cut, "eval_round -1")
    same_rows(again, cut, "the cut again")
    for k in ("expansions", "nn_evals", "cache_hits", "terminal_leaves", "games_finished"):
        assert cc[k] == co[k] == ca[k], k
    assert lc == lo == la and lc["total"] > 0
    assert cc["steps"] > co["steps"] and cc["steps"] == ca["steps"]  # the cut did put leaves off
    assert cc["cache_hits"] > 0 and cc["f32_fallback_evals"] == 0


# ---------------------------------------------------------------- 5. match play: the solver on one model only
def test_match_play_with_the_leaf_solver_on_one_model_vs_oracle():
    """model 0 (uniform) evaluates every leaf, model 1 (hash formula) solves those with F <= L; the model of a move is
    root_to_play ^ (game & 1), the tree is reused, so either model's searches descend through nodes the other one expanded"""
    from dotsboxesaz_amd.engine import Engine
    R, C, L, sims, n_games = 4, 4, 10, 24, 32
    what = "4x4 match play, leaf solver L %d on model 1" % L
    h = Endgame(R, C, max_free=12)
    e = Engine(R, C, 16, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=True, match_play=True, evaluator="uniform", evaluator2="formula", seed=9,
               leaf_endgame=h, leaf_free=L, leaf_models=(1,), endgame_seed=SEED)
    e.selfplay_start(n_games, 0)
    e.run()
    c, got = finished(e, n_games)
    ls = e.leaf_solves()
    e.close()
    h.close()
    w = LR.LeafSolver(R, C, L, SEED, (1, 0), match=True, leaf_models=(1,))
    tot = replay(got, range(n_games), O.dims(R, C), w, None, what, sims=sims, reuse=True)
    print("%s: %d leaves solved by F %s, %d base calls; device nn_evals %d" % (what, w.calls["solved"], w.by_free[:L + 1], w.calls["base"], c["nn_evals"]))
    assert c["expansions"] == tot["n_search"] and c["nn_evals"] == w.calls["base"] and c["cache_hits"] == 0
    assert ls["by_free"] == w.by_free and ls["total"] > 0
    for g in w.games:  # per move by the searching model: player ^ (game & 1)
        assert len(g["solved"]) > 0
    for gi in range(n_games):
        rows, g = game_rows(got, gi), w.games[gi]
        for i in range(len(rows["played"])):
            assert ((int(rows["player"][i]) ^ gi) & 1) == 1 or g["solved"][i] == 0, (gi, i)


# ---------------------------------------------------------------- 6. an explicit search on 6x6
def start_with_free(d, rs, n_edges, free):
    """a random legal move sequence that leaves `free` free edges and the game unfinished"""
    while True:
        s, moves = O.new_state(d), []
        for _ in range(n_edges - free):
            valid = np.nonzero(O.valid_moves(d, s))[0]
            m = int(valid[rs.randint(len(valid))])
            O.play_(d, s, m)
            moves.append(m)
            if O.get_result(s) is not None:
                break
        if len(moves) == n_edges - free and O.get_result(s) is None:
            return moves


def test_explicit_search_on_6x6_vs_oracle():
    """16 unfinished positions with 17 .. 20 free edges, one search(64) with L = 16: every root is above the threshold, the leaves
    below it are solved (F = 16: the 64 KB class; 14-15 and 11-13 below)"""
    from dotsboxesaz_amd.engine import Engine
    R, C, L, reads = 6, 6, 16, 64
    d, rs = O.dims(R, C), np.random.RandomState(11)
    starts = [start_with_free(d, rs, 84, 17 + i % 4) for i in range(16)]
    h = Endgame(R, C, max_free=16)
    e = Engine(R, C, 16, mcts_num_read=reads, evaluator="formula", leaf_endgame=h, leaf_free=L, endgame_seed=SEED)
    e.set_positions(starts)
    e.search(reads)
    r, ls, c = e.roots(), e.leaf_solves(), e.counters()
    e.close()
    h.close()
    assert c["error_slots"] == 0
    w = LR.LeafSolver(R, C, L, SEED, 0)
    w.start_game(d)
    for slot, moves in enumerate(starts):
        t = O.Tree(d, O.state_from_moves(d, moves))
        vis = t.search(reads, O.Evaluator(w.evaluate))
        _, tv, _, _ = t.root_arrays()
        assert np.array_equal(r["visits"][slot], vis), slot
        assert np.array_equal(r["total_value"][slot].view(np.uint32), np.asarray(tv, np.float32).view(np.uint32)), slot
    print("6x6 explicit search: %d leaves solved by F %s, %d base calls" % (w.calls["solved"], w.by_free, w.calls["base"]))
    assert ls["by_free"] == w.by_free and w.by_free[16] > 0 and sum(w.by_free[14:16]) > 0 and w.calls["base"] > 0
    assert c["nn_evals"] == w.calls["base"]


# ---------------------------------------------------------------- 7. off, and the refusals
def formula_engine(n_slots, **kw):
    from dotsboxesaz_amd.engine import Engine
    return Engine(4, 4, n_slots, mcts_num_read=24, noise=(0.0, 0.0), reuse_tree=True, evaluator="formula", seed=77, **kw)


def play(e, n_games=32):
    e.selfplay_start(n_games, 0)
    e.run()
    return finished(e, n_games)


def test_detached_is_never_attached_and_the_slot_count_changes_nothing():
    h = Endgame(4, 4, max_free=10)
    plain = formula_engine(32)
    c0, want = play(plain)
    plain.close()
    e = formula_engine(32, leaf_endgame=h, endgame_seed=SEED)
    c1, with_solver = play(e)
    solved = e.leaf_solves()
    assert solved["total"] > 0 and c1["nn_evals"] < c0["nn_evals"]
    assert with_solver["visits"].shape != want["visits"].shape or not np.array_equal(with_solver["visits"], want["visits"])
    e.attach_leaf_solver(None)
    assert e.leaf_solves() == solved  # the counters stay
    c2, got = play(e)
    same_rows(got, want, "detached after a run")
    assert e.leaf_solves() == solved
    e.close()
    e = formula_engine(32, leaf_endgame=h, endgame_seed=SEED)
    e.attach_leaf_solver(None)
    c2, got = play(e)
    same_rows(got, want, "detached before the first run")
    assert e.leaf_solves()["total"] == 0
    for k in ("steps", "expansions", "nn_evals", "cache_hits", "terminal_leaves"):
        assert c2[k] == c0[k], k
    e.close()
    small = formula_engine(8, leaf_endgame=h, endgame_seed=SEED)
    c3, got8 = play(small)
    same_rows(got8, with_solver, "8 slots against 32")
    assert small.leaf_solves() == solved
    small.close()
    h.close()


def test_refusals_change_nothing():
    from dotsboxesaz_amd.engine import Engine
    h, other, small = Endgame(4, 4, max_free=10), Endgame(3, 3, max_free=10), Endgame(4, 4, max_free=6)

    def refused(code, fn, *a, **kw):
        with pytest.raises(_lib.DbazError) as err:
            fn(*a, **kw)
        assert err.value.code == code, (err.value.code, str(err.value))

    for ev in ("external", "solver"):
        x = Engine(3, 3, 4, evaluator=ev)
        refused(_lib.EINVAL, x.attach_leaf_solver, other)
        x.close()
    e = formula_engine(8)
    refused(_lib.EINVAL, e.attach_leaf_solver, h, model=2)
    refused(_lib.EINVAL, e.attach_leaf_solver, h, model=-1)
    refused(_lib.EINVAL, e.attach_leaf_solver, h, model=1)  # no match play
    refused(_lib.EINVAL, e.attach_leaf_solver, other)  # another board
    refused(_lib.EINVAL, e.attach_leaf_solver, h, leaf_free=11)
    refused(_lib.EINVAL, e.attach_leaf_solver, h, leaf_free=0)  # (the Python layer: None means the handle's max_free)
    import ctypes as C
    assert e._L.dbaz_attach_leaf_solver(e.h, 0, h.h, -1, C.c_uint64(0)) == _lib.EINVAL
    deep = DeepTables(4, 4, max_free=12)
    refused(_lib.EINVAL, e.attach_leaf_solver, deep)  # (the Python layer: the C side cannot tell the handle types apart)
    deep.close()
    c0, want = play(e)
    assert e.leaf_solves()["total"] == 0
    # while games are being played, and between dbaz_search_begin and the end of that search
    e.attach_leaf_solver(small, seed=SEED)
    e.selfplay_start(32, 0)
    e.step(3)
    refused(_lib.ESTATE, e.attach_leaf_solver, h, seed=SEED + 1)
    refused(_lib.ESTATE, e.attach_leaf_solver, None)
    e.run()
    c1, got = finished(e, 32)
    solved = e.leaf_solves()
    e.close()
    ref = formula_engine(8, leaf_endgame=small, endgame_seed=SEED)  # the refused calls changed neither threshold nor seed nor handle
    c2, want_small = play(ref)
    same_rows(got, want_small, "after the refusals")
    assert ref.leaf_solves() == solved and solved["total"] > 0 and not any(solved["by_free"][7:])
    ref.set_positions(None)
    ref._ck(ref._L.dbaz_search_begin(ref.h, None, None))
    refused(_lib.ESTATE, ref.attach_leaf_solver, h)
    ref.close()
    m = Engine(4, 4, 8, match_play=True, evaluator="uniform", evaluator2="formula")
    m.attach_leaf_solver(h, 10, model=1)  # match play: model 1 is a model
    m.close()
    for g in (h, other, small):
        g.close()


# ---------------------------------------------------------------- 8. the stateless solver gives what the search used
def test_search_equals_an_external_search_fed_by_the_stateless_policy():
    """4x6 positions with at most 12 free edges: every leaf of their searches is solved.  The same searches with the leaves handed
    to the host (dbaz_select's leaf features) and answered by Endgame.policy(x, seed) give the same roots, bit for bit."""
    from dotsboxesaz_amd.engine import Engine
    R, C, L = 4, 6, 12
    d, rs = O.dims(R, C), np.random.RandomState(5)
    starts = [start_with_free(d, rs, 58, 12 - i % 8) for i in range(16)]
    h = Endgame(R, C, max_free=L)
    a = Engine(R, C, 16, mcts_num_read=20, evaluator="formula", leaf_endgame=h, endgame_seed=SEED)
    b = Engine(R, C, 16, mcts_num_read=20, evaluator="external")
    for e in (a, b):
        e.set_positions(starts)
    a.search(20)
    b.search_external(lambda x: h.policy(np.asarray(x).reshape(len(x), -1), SEED)[:2], 20)
    ra, rb = a.roots(), b.roots()
    for k in ra:
        assert np.array_equal(np.ascontiguousarray(ra[k]).view(np.uint8), np.ascontiguousarray(rb[k]).view(np.uint8)), k
    ca, ls = a.counters(), a.leaf_solves()
    assert ca["nn_evals"] == 0 and ls["total"] > 0 and not any(ls["by_free"][13:]) and ls["by_free"][12] > 0 and sum(ls["by_free"][1:11]) > 0
    a.close()
    b.close()
    h.close()
