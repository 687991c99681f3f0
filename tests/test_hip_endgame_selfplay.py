"""Self-play with an exact endgame table inside the search, bit for bit against the oracle (dbaz_attach_endgame, dbaz_attach_tables,
dbaz_attach_tables_pool; select_one's SEL_ENDGAME branch, k_select<NPL, true>, k_select_multi / k_expand_backup_multi, k_order_evals
and the network launch between select and expand in csrc/tree.hip; k_slot_requests, k_pool_decide / k_pool_grant in csrc/solver.hip).

Every game the engine played -- moves sampled on the device, no noise -- is replayed move by move by endgame_selfplay_ref.py: one
oracle tree per game, the evaluator chosen per move by the SEARCH ROOT (F <= max_free: the game's table, restated in numpy by
slot_tables_ref.py; otherwise the model's own evaluator), so a reused subtree holds nodes of both.  Every compared row must equal
the oracle's in x, player, visits, pi, q, TreeStats and z.  This pins what include/dbaz.h promises of a served leaf: it is not on
the evaluation lists, neither counted in nor deferred by the full-rounds cut, skips the transposition probe and is not counted in
nn_evals -- next to the network, the transposition table, the cut and the waves, which no other endgame test runs."""
import warnings

import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd.endgame import DeepTables, Endgame
import endgame_selfplay_ref as SR

pytestmark = pytest.mark.gpu

SEED = 3  # endgame_seed: which of several optimal moves gets the prior


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


def replay(got, games, d, base_ev, table, what, *, sims, reuse, min_reads=20, **kw):
    """replays `games` and checks the case's own preconditions; returns the sums over the replayed games"""
    tot = dict(games=0, served_games=0, served_searches=0, long_served=0, reused_first=0, base=0, table=0, n_search=0)
    for gi in games:
        rows = game_rows(got, gi)
        ref = SR.replay_game(d, rows, base_ev, table, sims=sims, reuse=reuse, **kw)
        assert_rows(ref, rows, (what, "game", int(gi)))
        s = ref["served"]
        tot["games"] += 1
        tot["served_games"] += bool(s.any())
        tot["served_searches"] += int(s.sum())
        long = bool((s & (ref["reads"] >= min_reads)).any())
        tot["long_served"] += long
        f = ref["first_served"]
        tot["reused_first"] += bool(long and f >= 0 and ref["root_expanded"][f] and rows["tree_size"][f] > 1)
        tot["base"] += ref["base_calls"]
        tot["table"] += ref["table_calls"]
        tot["n_search"] += ref["n_search"]
    # the case's preconditions: enough games with a served search of a real length, one of them on a reused, expanded root
    assert 4 * tot["long_served"] >= tot["games"], (what, tot)
    assert tot["reused_first"] >= 1 or not reuse, (what, tot)
    assert tot["table"] > 0 and tot["base"] > 0, (what, tot)
    return tot


def report(what, tot, c, stats):
    print("%s: %d games replayed, %d served searches in %d games, %d table and %d base evaluator calls; device: leaves_served %d, nn_evals %d, "
          "cache_hits %d" % (what, tot["games"], tot["served_searches"], tot["served_games"], tot["table"], tot["base"], stats[1], c["nn_evals"],
                             c["cache_hits"]))


def finished(e, n_games):
    c = e.counters()
    assert c["games_finished"] == n_games and c["error_slots"] == 0 and c["active_slots"] == 0 and c["pool_resets"] == 0
    got = e.fetch_samples()
    assert sorted(set(got["game_idx"])) == list(range(n_games))  # every game finished once
    return c, got


def handle(kind, R, C, M):
    return Endgame(R, C, max_free=M) if kind == "endgame" else DeepTables(R, C, max_free=M)


# ---------------------------------------------------------------- 1. the formula evaluator under every kind of attach
FORMULA = [(3, 3, "endgame", 8, None, 16, 48, 40), (4, 4, "endgame", 12, None, 32, 64, 24), (2, 7, "endgame", 10, None, 16, 32, 24),
           (6, 6, "endgame", 12, None, 8, 8, 30),  # 98 actions: two key words
           (4, 4, "deep", 12, None, 32, 64, 24), (4, 4, "deep", 12, "n_slots", 32, 64, 24),
           (4, 4, "deep", 18, None, 8, 8, 24)]  # past 16: the HBM layer kernels; a numpy table of 2^18 entries per game


def formula_case(R, C, kind, M, tables, n_slots, n_games, sims, tt, reuse, endgame_reads=0):
    from dotsboxesaz_amd.engine import Engine
    what = "%dx%d %s(%d)%s, %d reads, tt=%s, reuse=%s%s" % (R, C, kind, M, " pooled" if tables else "", sims, tt, reuse,
                                                            ", endgame_reads=%d" % endgame_reads if endgame_reads else "")
    h = handle(kind, R, C, M)
    e = Engine(R, C, n_slots, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=reuse, evaluator="formula", seed=1234, transposition_cache=tt,
               endgame=h, endgame_seed=SEED, endgame_reads=endgame_reads, endgame_tables=n_slots if tables else None)
    e.selfplay_start(n_games, 0)
    e.run()
    c, got = finished(e, n_games)
    stats = e.endgame_stats()
    pool = e.table_pool()
    e.close()
    h.close()
    tot = replay(got, range(n_games), O.dims(R, C), 0, SR.Table(R, C, M, SEED), what, sims=sims, reuse=reuse, endgame_reads=endgame_reads,
                 min_reads=min(20, endgame_reads) if endgame_reads else 20)
    report(what, tot, c, stats)
    # expansions counts every search: the reads of every move and the expansion of every root the tree did not hold (mcts.py:207-208)
    assert c["expansions"] == tot["n_search"]
    assert stats == (tot["served_games"], tot["table"])
    # nn_evals counts the leaves the model's own evaluator answered, formula leaves included (count_sim in csrc/tree.hip): neither
    # a finished game, nor a transposition hit, nor a served leaf
    assert c["nn_evals"] + c["cache_hits"] == tot["base"]
    assert (c["cache_hits"] > 0) == (tt == "force")
    if tables:
        assert pool["denied"] == 0 and pool["in_use"] == 0 and 1 <= pool["high_water"] <= n_slots
    return got


@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("tt", [True, "force"])
@pytest.mark.parametrize("R,C,kind,M,tables,n_slots,n_games,sims", FORMULA)
def test_formula_selfplay_with_a_table_vs_oracle(R, C, kind, M, tables, n_slots, n_games, sims, tt, reuse):
    formula_case(R, C, kind, M, tables, n_slots, n_games, sims, tt, reuse)


def test_endgame_reads_cap_vs_oracle():
    """served searches run min(rule, 3) reads, every other search the rule's (the replay caps the same searches)"""
    formula_case(4, 4, "endgame", 12, None, 32, 64, 24, "force", True, endgame_reads=3)


# ---------------------------------------------------------------- 2. the network evaluator, transposition table on
def network(R, C):
    import torch
    from oracle import nn_ref
    torch.manual_seed(R * 10 + 2)
    m = nn_ref.ResNetZeroRef(R, C, 64, 2)
    nn_ref.randomize_bn(m, 3)
    return m


def network_engine(R, C, n_slots, sims, M, precision, **kw):
    from dotsboxesaz_amd.engine import Engine
    h = Endgame(R, C, max_free=M)
    e = Engine(R, C, n_slots, mcts_num_read=sims, noise=(0.0, 0.0), evaluator="resnet", seed=5, nn_precision=precision, endgame=h,
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


_net_rows = {}


@pytest.mark.parametrize("R,C,M,n_slots,n_games,sims,precision", [(3, 3, 8, 16, 32, 25, 0), (3, 3, 8, 16, 32, 25, 1), (6, 6, 12, 8, 4, 40, 1)])
def test_network_selfplay_with_a_table_vs_oracle(R, C, M, n_slots, n_games, sims, precision):
    what = "%dx%d network, precision %d, Endgame(%d), %d reads" % (R, C, precision, M, sims)
    e, h = network_engine(R, C, n_slots, sims, M, precision)
    e.selfplay_start(n_games, 0)
    e.run()
    c, got = finished(e, n_games)
    stats = e.endgame_stats()
    assert c["cache_hits"] > 0 and c["f32_fallback_evals"] == 0
    games = range(n_games) if n_games <= 16 else range(0, n_games, 2)
    tot = replay(got, games, O.dims(R, C), asks(e, R, C), SR.Table(R, C, M, SEED), what, sims=sims, reuse=True)
    report(what, tot, c, stats)
    if len(games) == n_games:
        assert c["nn_evals"] + c["cache_hits"] == tot["base"] and stats[1] == tot["table"] and stats[0] == tot["served_games"]
        assert c["expansions"] == tot["n_search"]
    else:  # half of the games replayed: each of the device's sums covers the replayed games' at least
        assert c["nn_evals"] + c["cache_hits"] > tot["base"] and stats[1] > tot["table"] and stats[0] >= tot["served_games"]
    e.close()
    h.close()
    _net_rows[(R, C, precision)] = got


@pytest.mark.parametrize("precision", [0, 1])
def test_table_keeps_the_transposition_cache_transparent(precision):
    """the same 3x3 network without the transposition table: the rows of the cached run"""
    if (3, 3, precision) not in _net_rows:
        test_network_selfplay_with_a_table_vs_oracle(3, 3, 8, 16, 32, 25, precision)
    want = _net_rows[(3, 3, precision)]
    e, h = network_engine(3, 3, 16, 25, 8, precision, transposition_cache=False)
    e.selfplay_start(32, 0)
    e.run()
    c, got = finished(e, 32)
    assert c["cache_hits"] == 0 and c["f32_fallback_evals"] == 0 and e.endgame_stats()[1] > 0
    e.close()
    h.close()
    assert set(got) == set(want)
    for k in got:
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k


# ---------------------------------------------------------------- 3. the full-rounds cut with a table
def test_full_rounds_cut_with_a_table():
    """served leaves go through k_select<NPL, true> while other slots hold put-off leaves: nothing but the schedule may change"""
    R, C, M, sims, n_games = 3, 3, 8, 25, 77
    runs = []
    for er, ed in ((16, 15), (-1, 0), (16, 15)):
        e, h = network_engine(R, C, 40, sims, M, 1, reuse_tree=True, eval_round=er, eval_defer_max=ed)
        e.selfplay_start(n_games, 0)
        e.run()
        c, got = finished(e, n_games)
        runs.append((got, c, e.endgame_stats()))
        if len(runs) == 1:  # 8 of the games against the oracle, while the engine can still be asked
            tot = replay(got, range(0, n_games, 10), O.dims(R, C), asks(e, R, C), SR.Table(R, C, M, SEED), "3x3 network with the cut", sims=sims,
                         reuse=True)
            assert tot["games"] == 8
            report("3x3 network, eval_round 16, eval_defer_max 15", tot, c, e.endgame_stats())
        e.close()
        h.close()
    (cut, cc, sc), (off, co, so), (again, ca, sa) = runs
    for other, what in ((off, "eval_round -1"), (again, "the cut again")):
        assert set(cut) == set(other)
        for k in cut:
            assert np.array_equal(np.ascontiguousarray(cut[k]).view(np.uint8), np.ascontiguousarray(other[k]).view(np.uint8)), (what, k)
    for k in ("expansions", "nn_evals", "cache_hits", "terminal_leaves", "games_finished"):
        assert cc[k] == co[k] == ca[k], k
    assert sc == so == sa and sc[1] > 0
    assert cc["steps"] > co["steps"] and cc["steps"] == ca["steps"]
    assert cc["cache_hits"] > 0 and cc["f32_fallback_evals"] == 0


# ---------------------------------------------------------------- 4. waves
@pytest.mark.parametrize("R,C,M,sims,K,reuse", [(4, 4, 12, 24, 8, True), (4, 4, 12, 24, 3, True), (3, 3, 8, 40, 64, False)])
def test_selfplay_in_waves_with_a_table_vs_oracle(R, C, M, sims, K, reuse):
    from dotsboxesaz_amd.engine import Engine
    what = "%dx%d Endgame(%d) in waves of %d, reuse=%s" % (R, C, M, K, reuse)
    h = Endgame(R, C, max_free=M)
    e = Engine(R, C, 8, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=reuse, evaluator="formula", seed=3, max_pending_evals=K,
               selfplay_pending=True, endgame=h, endgame_seed=SEED)
    e.selfplay_start(16, 0)
    e.run()
    c, got = finished(e, 16)
    stats = e.endgame_stats()
    e.close()
    h.close()
    tot = replay(got, range(16), O.dims(R, C), 0, SR.Table(R, C, M, SEED), what, sims=sims, reuse=reuse, K=K)
    report(what, tot, c, stats)
    assert c["expansions"] == tot["n_search"] and stats[0] == tot["served_games"]
    # a leaf that an earlier simulation of its wave already holds is evaluated once on the device (counted in cache_hits, whichever
    # evaluator answered the first) and once per simulation by the oracle's wave search: only the sum of the three is comparable
    assert c["nn_evals"] + c["cache_hits"] + stats[1] == tot["base"] + tot["table"]
    assert 0 < stats[1] <= tot["table"] and c["nn_evals"] <= tot["base"]


def test_network_selfplay_in_waves_with_a_table_vs_oracle():
    R, C, M, sims, K = 3, 3, 8, 25, 8
    e, h = network_engine(R, C, 8, sims, M, 1, max_pending_evals=K, selfplay_pending=True)
    e.selfplay_start(16, 0)
    e.run()
    c, got = finished(e, 16)
    stats = e.endgame_stats()
    assert c["f32_fallback_evals"] == 0 and stats[1] > 0
    tot = replay(got, range(0, 16, 4), O.dims(R, C), asks(e, R, C), SR.Table(R, C, M, SEED), "3x3 network in waves of 8", sims=sims, reuse=True, K=K)
    report("3x3 network in waves of 8", tot, c, stats)
    e.close()
    h.close()


# ---------------------------------------------------------------- 5. a pool of tables that runs dry
def test_dry_pool_selfplay_vs_oracle():
    """A slot that finds the pool dry searches that move with its model's evaluator and asks again at its next move: for every
    game some first served move g -- from the first move with F <= max_free to never -- reproduces all rows, and the denials the
    device counted lie between the smallest and the largest such g, summed over the games."""
    from dotsboxesaz_amd.engine import Engine
    R, C, M, sims, n_games = 4, 4, 12, 24, 64
    d = O.dims(R, C)
    h = DeepTables(R, C, max_free=M)
    e = Engine(R, C, 32, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=True, evaluator="formula", seed=1234, transposition_cache="force",
               endgame=h, endgame_seed=SEED, endgame_tables=4)
    e.selfplay_start(n_games, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # run() says that the pool ran dry: that is the case under test
        e.run()
    c, got = finished(e, n_games)
    stats, pool = e.endgame_stats(), e.table_pool()
    e.close()
    h.close()
    table = SR.Table(R, C, M, SEED)
    lo = hi = unique_late = never_eligible = 0
    tot = dict(base=0, table=0)
    for gi in range(n_games):
        rows = game_rows(got, gi)
        n, left = len(rows["played"]), SR.free_edges(R, C, rows["x"])
        if left.min() > M:  # the game ended before any root had F <= max_free: the plain oracle
            ref = SR.replay_game(d, rows, 0, None, sims=sims, reuse=True)
            assert_rows(ref, rows, ("never eligible", gi))
            never_eligible += 1
            tot["base"] += ref["base_calls"]
            continue
        first = int(np.nonzero(left <= M)[0][0])
        # g = never first.  Its rows before any g are those of every later g, so where it first differs from the device's rows, say at
        # row i, every g > i differs there too: those replays are decided without running them
        matching, refs = [], {}
        never = SR.replay_game(d, rows, 0, table, sims=sims, reuse=True, served_from=SR.NEVER, stop_at_mismatch=True)
        if never["mismatch"] < 0 and SR.rows_differ(never, rows) < 0:
            matching.append(n)
            refs[n] = never
        last = n - 1 if never["mismatch"] < 0 else min(never["mismatch"], n - 1)
        for g in range(first, last + 1):
            ref = SR.replay_game(d, rows, 0, table, sims=sims, reuse=True, served_from=g, stop_at_mismatch=True)
            if ref["mismatch"] < 0 and SR.rows_differ(ref, rows) < 0:
                matching.append(g)
                refs[g] = ref
        assert matching, ("no first served move reproduces the game", gi, first, never["mismatch"])
        lo += min(matching) - first
        hi += max(matching) - first
        unique_late += len(matching) == 1 and matching[0] > first
        ref = refs[min(matching)]
        assert_rows(ref, rows, ("dry pool", gi, min(matching)))
        tot["base"] += ref["base_calls"]
        tot["table"] += ref["table_calls"]
    print("dry pool of 4 tables, 32 slots, 64 games: %s, tables solved %d, leaves served %d; denials by the replay %d .. %d, %d games with one "
          "possible first served move later than their first eligible one, %d never eligible; %d table and %d base calls with the earliest "
          "matching moves, cache_hits %d" % (pool, stats[0], stats[1], lo, hi, unique_late, never_eligible, tot["table"], tot["base"], c["cache_hits"]))
    assert unique_late >= 8  # (a condition on the inputs: games that pin a denial to one move)
    assert lo <= pool["denied"] <= hi and pool["denied"] > 0
    assert pool["high_water"] == 4 and pool["in_use"] == 0 and pool["n_tables"] == 4
    assert c["cache_hits"] > 0 and stats[1] > 0


# ---------------------------------------------------------------- 6. match play: served and unserved searches alternate in one tree
@pytest.mark.parametrize("tables", [None, 16])
def test_match_play_with_a_table_vs_oracle(tables):
    """model 0 (uniform) has the tables, model 1 (hash formula) has none; the model of a move is root_to_play ^ (game & 1), the tree is
    reused from move to move, so the searches of one model descend through nodes the other one's evaluator expanded"""
    from dotsboxesaz_amd.engine import Engine
    R, C, M, sims, n_games = 4, 4, 12, 24, 32
    what = "4x4 match play, DeepTables(12)%s" % (" pooled" if tables else "")
    h = DeepTables(R, C, max_free=M)
    e = Engine(R, C, 16, mcts_num_read=sims, noise=(0.0, 0.0), reuse_tree=True, match_play=True, evaluator="uniform", evaluator2="formula", seed=9,
               endgame=h, endgame_models=(0,), endgame_seed=SEED, endgame_tables=tables)
    e.selfplay_start(n_games, 0)
    e.run()
    c, got = finished(e, n_games)
    stats, pool = e.endgame_stats(), e.table_pool()
    e.close()
    h.close()
    tot = replay(got, range(n_games), O.dims(R, C), None, SR.Table(R, C, M, SEED), what, sims=sims, reuse=True, models=(1, 0, (0,)))
    report(what, tot, c, stats)
    assert c["expansions"] == tot["n_search"] and stats == (tot["served_games"], tot["table"])
    assert c["nn_evals"] == tot["base"] and c["cache_hits"] == 0
    if tables:
        assert pool["denied"] == 0 and pool["in_use"] == 0
