"""The pool of tables in wait mode (dbaz_attach_tables_pool_wait, Engine(endgame_tables=N, endgame_wait=True)): a slot that finds
the pool dry waits for a region instead of searching that move without a table -- the standing requests in k_pool_decide and
k_slot_requests<true> (csrc/solver.hip), the settle step of csrc/table_pool.h, the waiting slots that k_select and k_select_multi
leave alone (csrc/tree.hip), and the step stamp with which a pass wakes a slot next to the selection of its own step.

What is pinned: for every pool size the rows, the tables solved and the leaves served are those of the per-slot attach, byte for
byte -- in lockstep, staggered and in waves, with a read cap, with the playout cap and forced playouts on top, in match play and
with more slots than one ranking round of k_pool_grant -- and those of the CPU oracle; nothing is denied; the pool's invariants hold
while slots wait; a waiting slot's tree does not move; the refusals change nothing.  Every comparison asserts that slots did wait.
Formula and uniform evaluators on a 3x3 board (24 edges, max_free = 10: the last ten moves of every game need a table).

The oracle replays (endgame_selfplay_ref.py) are of games without root noise, as everywhere in the suite: the device's Dirichlet
stream has no host counterpart.  The comparisons between two engines keep the noise."""
import warnings

import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.endgame import DeepTables, Endgame
import endgame_selfplay_ref as SR

pytestmark = pytest.mark.gpu

R, C, M, E = 3, 3, 10, 24
N_SLOTS, N_GAMES, SIMS, SEED = 8, 24, 16, 2


def same_rows(ra, rb, what=""):
    assert set(ra) == set(rb)
    for k in ra:
        assert np.array_equal(np.ascontiguousarray(ra[k]).view(np.uint8), np.ascontiguousarray(rb[k]).view(np.uint8)), (what, k)


def same_roots(ra, rb, what=""):
    for k in ra:
        assert np.array_equal(np.ascontiguousarray(ra[k]).view(np.uint8), np.ascontiguousarray(rb[k]).view(np.uint8)), (what, k)


def start_with_free(d, rs, free):
    """a random legal move sequence that leaves `free` free edges and the game unfinished"""
    while True:
        s, moves = O.new_state(d), []
        for _ in range(E - free):
            valid = np.nonzero(O.valid_moves(d, s))[0]
            m = int(valid[rs.randint(len(valid))])
            O.play_(d, s, m)
            moves.append(m)
            if O.get_result(s) is not None:
                break
        if len(moves) == E - free and O.get_result(s) is None:
            return moves


def play(tables, n_tables, wait=False, mode="lockstep", n_slots=N_SLOTS, n_games=N_GAMES, setup=None, **kw):
    """one whole self-play run -> (rows, endgame_stats, table_pool, table_pool_waits, counters)"""
    from dotsboxesaz_amd.engine import Engine
    args = dict(mcts_num_read=SIMS, noise=(0.8, 0.25), temperature={0: 1.0}, evaluator="formula", endgame=tables, endgame_seed=SEED, seed=5)
    args.update(kw)
    if mode == "waves":
        args.update(max_pending_evals=4, selfplay_pending=True)
    e = Engine(R, C, n_slots, endgame_tables=n_tables, endgame_wait=wait, **args)
    if mode == "stagger":
        e.selfplay_stagger(1 + np.arange(n_slots) % 7)
    if setup:
        setup(e)
    e.selfplay_start(n_games, 0)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*dry.*")  # nothing is denied: run() has nothing to say about the pool
        e.run()
    c = e.counters()
    assert c["games_finished"] == n_games and c["error_slots"] == 0 and c["active_slots"] == 0
    out = (e.fetch_samples(), e.endgame_stats(), e.table_pool(), e.table_pool_waits(), c)
    e.close()
    return out


def check_waited(what, n_tables, stats, pool, waits):
    print("%s: %s %s, tables solved %d, leaves served %d" % (what, pool, waits, stats[0], stats[1]))
    assert pool["denied"] == 0 and pool["n_tables"] == n_tables and pool["high_water"] == n_tables and pool["in_use"] == 0
    assert waits["wait_mode"] == 1 and waits["waited"] > 0 and waits["waiting"] == 0


def against_per_slot(what, pools, **kw):
    """the waiting pools of the sizes `pools` against the per-slot attach of the same configuration; returns the per-slot rows"""
    tables = DeepTables(R, C, max_free=M)
    rows, stats, pool, waits, c = play(tables, None, **kw)
    assert pool == dict(n_tables=0, in_use=0, high_water=0, denied=0) and waits == dict(wait_mode=0, waiting=0, waited=0)
    assert stats[0] >= kw.get("n_games", N_GAMES) // 2 and stats[1] > 0
    for n_tables in pools:
        rows_w, stats_w, pool_w, waits_w, c_w = play(tables, n_tables, True, **kw)
        check_waited("%s, pool of %d" % (what, n_tables), n_tables, stats_w, pool_w, waits_w)
        same_rows(rows_w, rows, (what, n_tables))
        assert stats_w == stats
        for k in ("expansions", "nn_evals", "moves_played", "terminal_leaves"):  # no read was spent while waiting
            assert c_w[k] == c[k], k
        assert c_w["steps"] > c["steps"]  # the price: steps in which slots idle
    tables.close()
    return rows


# ---------------------------------------------------------------- 1. the rows of the per-slot attach, for any pool size
@pytest.mark.parametrize("mode", ["lockstep", "stagger", "waves"])
def test_waiting_pool_of_any_size_equals_the_per_slot_attach(mode):
    against_per_slot(mode, (1, 3), mode=mode)


# ---------------------------------------------------------------- 2. and of the CPU oracle
def game_rows(got, gi):
    r = np.nonzero(got["game_idx"] == gi)[0]
    assert list(got["move_idx"][r]) == list(range(len(r))), gi
    return {k: v[r] for k, v in got.items()}


def assert_oracle(got, n_games, what, endgame_reads=0, models=None, base_ev=0):
    """every game replayed move by move on one oracle tree, the searches under a root with F <= M served by the game's table"""
    d, table = O.dims(R, C), SR.Table(R, C, M, SEED)
    tot = dict(table=0, base=0, served_games=0, n_search=0)
    for gi in range(n_games):
        rows = game_rows(got, gi)
        ref = SR.replay_game(d, rows, base_ev, table, sims=SIMS, reuse=True, endgame_reads=endgame_reads, models=models)
        assert ref["mismatch"] < 0 and SR.rows_differ(ref, rows) < 0, (what, gi, SR.rows_differ(ref, rows))
        for i in range(ref["n_rows"]):
            assert np.array_equal(ref["visits"][i], rows["visits"][i]), (what, gi, i)
        served = ref["served"]
        assert models is not None or np.array_equal(served, ref["n_free"] <= M)
        if endgame_reads:
            assert (ref["reads"][served] <= endgame_reads).all() and (ref["reads"][~served] > endgame_reads).all()
        tot["table"] += ref["table_calls"]
        tot["base"] += ref["base_calls"]
        tot["served_games"] += bool(served.any())
        tot["n_search"] += ref["n_search"]
    return tot


def test_waiting_pool_of_one_vs_oracle():
    tables = DeepTables(R, C, max_free=M)
    rows, stats, pool, waits, c = play(tables, 1, True, noise=(0.0, 0.0))
    tables.close()
    check_waited("pool of 1 against the oracle", 1, stats, pool, waits)
    tot = assert_oracle(rows, N_GAMES, "pool of 1")
    assert stats == (tot["served_games"], tot["table"]) and tot["served_games"] == N_GAMES
    assert c["expansions"] == tot["n_search"] and c["nn_evals"] + c["cache_hits"] == tot["base"]


# ---------------------------------------------------------------- 3. the read cap, which the deny-mode pool has to refuse
def test_endgame_reads_with_a_waiting_pool():
    against_per_slot("endgame_reads=3", (2,), endgame_reads=3)
    # without noise: against the oracle, which caps the same searches; and through the rows themselves
    tables = DeepTables(R, C, max_free=M)
    rows, stats, pool, waits, c = play(tables, 2, True, noise=(0.0, 0.0), endgame_reads=3)
    tables.close()
    check_waited("endgame_reads=3 against the oracle", 2, stats, pool, waits)
    tot = assert_oracle(rows, N_GAMES, "endgame_reads=3", endgame_reads=3)
    assert stats == (tot["served_games"], tot["table"]) and c["expansions"] == tot["n_search"]
    # The tree is reused: the visits of a row are what the played child's subtree held (its own visit aside) plus the reads of the
    # row's search.  Every move draws one edge, so row i has F = 24 - i, and the rule alone would give min(4 * F!, 16) >= 4 reads.
    capped = want = 0
    for gi in range(N_GAMES):
        g = game_rows(rows, gi)
        assert np.array_equal(SR.free_edges(R, C, g["x"]), E - np.arange(len(g["played"])))
        want += max(len(g["played"]) - (E - M), 0)
        for i in range(1, len(g["played"])):
            kept = max(int(g["visits"][i - 1][g["played"][i - 1]]) - 1, 0)
            reads = int(g["visits"][i].sum()) - kept
            if E - i <= M:
                assert 0 <= reads <= 3, (gi, i, reads)
                capped += 1
            else:
                assert reads == SIMS, (gi, i, reads)
    assert capped == want >= N_GAMES


# ---------------------------------------------------------------- 4. more slots than one ranking round of k_pool_grant
def test_more_waiting_slots_than_one_ranking_round():
    n = 1100  # TABLE_POOL_GROUP = 1024: the standing requests of slots 1024 .. 1099 are ranked in the second round
    against_per_slot("1100 slots", (40,), n_slots=n, n_games=n, mcts_num_read=4, evaluator="uniform", noise=(0.0, 0.0))


# ---------------------------------------------------------------- 5. invariants while slots wait; reproducibility
def play_in_pieces(tables, check):
    from dotsboxesaz_amd.engine import Engine
    e = Engine(R, C, N_SLOTS, mcts_num_read=SIMS, noise=(0.8, 0.25), temperature={0: 1.0}, evaluator="formula", endgame=tables, endgame_seed=SEED,
               seed=5, endgame_tables=3, endgame_wait=True)
    e.selfplay_start(N_GAMES, 0)
    pieces = seen_waiting = still = 0
    before = {}
    while e.counters()["active_slots"] > 0:
        e.run(max_steps=40)
        pieces += 1
        assert pieces < 400
        if not check:
            continue
        hdr = [e.slot_table(s) for s in range(N_SLOTS)]
        p, w = e.table_pool(), e.table_pool_waits()
        held = [h["table_index"] for h in hdr if h["valid"]]
        assert len(set(held)) == len(held) and all(0 <= t < 3 for t in held)  # pairwise distinct regions of the pool
        assert len(held) == p["in_use"] <= 3 and p["denied"] == 0
        assert all(h["table_index"] == -1 for h in hdr if not h["valid"])
        assert w["waiting"] + len(held) <= N_SLOTS
        assert w["waiting"] == 0 or p["in_use"] == 3  # work-conserving: nobody waits next to a free region
        # who waits: an unfinished game in its last M moves whose slot holds no region (between two run() calls no request is undecided)
        st = e.root_states()
        free = e.rules_valid_moves(st).sum(1)
        waiting = [s for s in range(N_SLOTS) if st["result"][s] == _lib.RESULT_NONE and free[s] <= M and not hdr[s]["valid"]]
        assert len(waiting) == w["waiting"], (waiting, w)
        seen_waiting += len(waiting)
        r = e.roots()
        now = {}
        for s in waiting:
            now[s] = (st["edges"][s].tobytes(), int(r["root_nv"][s]), r["visits"][s].copy(), r["total_value"][s].copy())
            if s in before and before[s][0] == now[s][0]:  # the same root 40 steps later: not one visit more
                assert before[s][1] == now[s][1] and np.array_equal(before[s][2], now[s][2])
                assert np.array_equal(before[s][3].view(np.uint32), now[s][3].view(np.uint32))
                still += 1
        before = now
    c = e.counters()
    out = (e.fetch_samples(), e.endgame_stats(), e.table_pool(), e.table_pool_waits(), {k: c[k] for k in ("games_finished", "error_slots", "expansions",
                                                                                                             "moves_played", "steps")})
    e.close()
    return out, seen_waiting, still


def test_waiting_pool_keeps_its_invariants_and_is_reproducible():
    tables = DeepTables(R, C, max_free=M)
    first, seen_waiting, still = play_in_pieces(tables, True)
    print("pool of 3 in pieces of 40 steps: %s %s, %d waiting slots seen, %d of them twice on one root" % (first[2], first[3], seen_waiting, still))
    assert seen_waiting > 0 and still > 0
    check_waited("in pieces", 3, first[1], first[2], first[3])
    assert first[4]["games_finished"] == N_GAMES and first[4]["error_slots"] == 0
    second, _, _ = play_in_pieces(tables, False)
    whole = play(tables, 3, True)
    tables.close()
    same_rows(first[0], second[0], "second run")
    assert first[1:] == second[1:]
    same_rows(first[0], whole[0], "in one piece")  # where the host looks at the run changes nothing
    assert first[1:4] == whole[1:4]


# ---------------------------------------------------------------- 6. playout cap and forced playouts on top
def test_playout_cap_and_forced_playouts_with_a_waiting_pool():
    rows = against_per_slot("playout cap, forced playouts", (2,), playout_cap=(0.5, 6), forced_playouts=(2.0, True))
    assert "full" in rows and "pruned" in rows and 0 < rows["full"].sum() < len(rows["full"]) and rows["pruned"].any()


# ---------------------------------------------------------------- 7. match play
def test_match_play_with_a_waiting_pool():
    d, rs = O.dims(R, C), np.random.RandomState(4)
    book = [start_with_free(d, rs, M + i % 3) for i in range(8)]
    against_per_slot("match play", (2,), match_play=True, evaluator="uniform", evaluator2="formula", endgame_models=(0,), reuse_tree=False,
                     noise=(0.0, 0.0), setup=lambda e: e.selfplay_set_start(book, 1))


# ---------------------------------------------------------------- 8. refusals
def test_refusals_change_nothing():
    from dotsboxesaz_amd.engine import Engine

    def code(fn):
        with pytest.raises(_lib.DbazError) as ei:
            fn()
        return ei.value.code

    d, rs = O.dims(R, C), np.random.RandomState(7)
    starts = [start_with_free(d, rs, M - i % 4) for i in range(N_SLOTS)]
    tables = DeepTables(R, C, max_free=M)
    g = Endgame(R, C, max_free=M)

    def roots(e):
        e.set_positions(starts)
        e.search(20)
        return e.roots()

    def short_run(e):
        e.selfplay_start(N_SLOTS, 0)
        e.run()
        return e.fetch_samples()

    # a bare handle: every refused wait attach leaves it without tables
    e = Engine(R, C, N_SLOTS, mcts_num_read=SIMS, evaluator="formula")
    before = roots(e)
    for bad in (lambda: e.attach_endgame_pool_wait(tables, 0), lambda: e.attach_endgame_pool_wait(tables, -3),
                lambda: e.attach_endgame_pool_wait(tables, N_SLOTS + 1), lambda: e.attach_endgame_pool_wait(tables, 4, reads=-1),
                lambda: e.attach_endgame_pool_wait(g, 4), lambda: e.attach_endgame_pool_wait(tables, 4, model=1)):
        assert code(bad) == _lib.EINVAL
    assert e.table_pool()["n_tables"] == 0 and e.table_pool_waits() == dict(wait_mode=0, waiting=0, waited=0)
    same_roots(before, roots(e), "after refused wait attaches on a bare handle")
    assert code(lambda: Engine(R, C, N_SLOTS, evaluator="formula", endgame=tables, endgame_wait=True)) == _lib.EINVAL  # no pool to wait for
    # a deny-mode pooled handle refuses the wait attach, and goes on denying and searching
    e.attach_endgame_pool(tables, 4, seed=SEED)
    pooled = roots(e)
    figures = e.table_pool()
    assert figures == dict(n_tables=4, in_use=4, high_water=4, denied=4)
    assert code(lambda: e.attach_endgame_pool_wait(tables, 4, seed=SEED)) == _lib.EINVAL
    assert code(lambda: e.attach_endgame_pool_wait(tables, 4, seed=SEED, reads=3)) == _lib.EINVAL
    assert e.table_pool() == figures and e.table_pool_waits() == dict(wait_mode=0, waiting=0, waited=0)  # not even the headers were dropped
    same_roots(pooled, roots(e), "after a refused wait attach on a deny-mode handle")
    e.close()
    # a per-slot handle and an Endgame handle refuse it
    for h in (tables, g):
        e2 = Engine(R, C, N_SLOTS, mcts_num_read=SIMS, evaluator="formula", endgame=h, endgame_seed=SEED)
        per_slot = roots(e2)
        assert code(lambda: e2.attach_endgame_pool_wait(tables, 4, seed=SEED)) == _lib.EINVAL
        assert e2.table_pool()["n_tables"] == 0 and e2.table_pool_waits()["wait_mode"] == 0
        same_roots(per_slot, roots(e2), "after a refused wait attach on a handle with one region per slot")
        e2.close()
    # a wait-mode handle: the deny attach, the per-slot attach, another n_tables and explicit searches are refused
    w = Engine(R, C, N_SLOTS, mcts_num_read=SIMS, noise=(0.8, 0.25), temperature={0: 1.0}, evaluator="formula", seed=5)
    w.attach_endgame_pool_wait(tables, 2, seed=SEED, reads=3)
    assert w.table_pool_waits() == dict(wait_mode=1, waiting=0, waited=0)
    rows = short_run(w)
    waits = w.table_pool_waits()
    assert waits["waited"] > 0 and waits["waiting"] == 0 and w.table_pool()["denied"] == 0
    for bad in (lambda: w.attach_endgame_pool(tables, 2, seed=SEED), lambda: w.attach_endgame(tables, 0, seed=SEED),
                lambda: w.attach_endgame_pool_wait(tables, 3, seed=SEED), lambda: w.attach_endgame_pool_wait(tables, 2, reads=-1),
                lambda: w.attach_endgame_pool_wait(g, 2)):
        assert code(bad) == _lib.EINVAL
    w.set_positions(starts)
    for bad in (lambda: w.search(20), lambda: w.search_timed(1.0, 20), lambda: w.search_external(lambda x: None, 20)):
        assert code(bad) == _lib.ESTATE
    assert w.table_pool_waits() == dict(wait_mode=1, waiting=0, waited=waits["waited"]) and w.table_pool()["in_use"] == 0
    same_rows(rows, short_run(w), "a short run after the refusals")
    # a re-attach, set_positions and selfplay_start clear every wait along with the regions
    w.selfplay_start(N_SLOTS, 0)
    w.run(max_steps=E - M + (E - M) * SIMS + 40)  # past the first moves with F <= M: two slots hold the regions, the others wait
    assert w.table_pool_waits()["waiting"] > 0 and w.table_pool()["in_use"] == 2
    w.attach_endgame_pool_wait(tables, 2, seed=SEED, reads=3)
    assert w.table_pool_waits()["waiting"] == 0 and w.table_pool()["in_use"] == 0
    w.selfplay_start(N_SLOTS, 0)
    w.run(max_steps=E - M + (E - M) * SIMS + 40)
    assert w.table_pool_waits()["waiting"] > 0
    w.set_positions(starts)
    assert w.table_pool_waits()["waiting"] == 0 and w.table_pool()["in_use"] == 0
    same_rows(rows, short_run(w), "a short run after the waits were cleared")
    assert w.counters()["error_slots"] == 0
    w.close()
    g.close()
    tables.close()
