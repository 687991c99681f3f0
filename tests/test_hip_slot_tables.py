"""Deep tables inside the search on the GPU (dbaz_attach_tables: k_slot_requests / k_slot_solve in csrc/solver.hip, the launch plan
of csrc/slot_tables_plan.h, k_endgame_eval and the routing unchanged): the slot tables byte for byte against DeepTables.solve, the
search against an external-evaluator engine fed by the numpy restatement (slot_tables_ref.py), the two kinds of attach against
each other at max_free = 16, roots above max_free against a plain engine, self-play in lockstep and staggered, scheduling
independence, the read cap, waves, match play and the attach errors.  Formula and uniform evaluators only; every self-play here
searches each move from a fresh root without noise (DESIGN 4.7's condition)."""
import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.endgame import DeepTables, Endgame, score_game_tails
import endgame_ref as ER
from slot_tables_ref import SlotTablesRef

pytestmark = pytest.mark.gpu


def start_with_free(d, rs, n_edges, free):
    """a random legal move sequence that leaves `free` free edges and the game unfinished (test_hip_endgame_eval.py's method);
    free = 0: the game is unfinished until its last edge"""
    while True:
        s, moves = O.new_state(d), []
        for _ in range(n_edges - max(free, 1)):
            valid = np.nonzero(O.valid_moves(d, s))[0]
            m = int(valid[rs.randint(len(valid))])
            O.play_(d, s, m)
            moves.append(m)
            if O.get_result(s) is not None:
                break
        if len(moves) == n_edges - max(free, 1) and O.get_result(s) is None:
            if free == 0:
                moves.append(int(np.nonzero(O.valid_moves(d, s))[0][0]))
            return moves


def n_edges(R, C):
    return 2 * R * C + R + C


def rows_of(R, C, starts):
    d = O.dims(R, C)
    return np.array([O.features(d, O.state_from_moves(d, m)).ravel() for m in starts], np.int16)


def free_words(R, C, x):
    """position_geometry's free_edges of a feature row: the free real edges by action index, four 64-bit words"""
    acts, _ = ER.board(R, C)
    w = [0, 0, 0, 0]
    for a in acts:
        if x[a] == 0:
            w[a >> 6] |= 1 << (a & 63)
    return np.array(w, np.uint64)


def same_roots(ra, rb, slots=slice(None), what=""):
    for k in ra:
        assert np.array_equal(np.ascontiguousarray(ra[k][slots]).view(np.uint8), np.ascontiguousarray(rb[k][slots]).view(np.uint8)), (what, k)


_starts = {}


def starts_below(R, C, max_free):
    """64 starts with F <= max_free, built once: four at max_free, the others cycling through max_free - 1 .. 3"""
    if (R, C, max_free) not in _starts:
        d, rs = O.dims(R, C), np.random.RandomState(7 * R + C + max_free)
        frees = [max_free] * 4 + [max_free - 1 - i % (max_free - 3) for i in range(60)]
        _starts[(R, C, max_free)] = ([start_with_free(d, rs, n_edges(R, C), f) for f in frees], np.array(frees))
    return _starts[(R, C, max_free)]


def starts_above(R, C, max_free, n=64, seed=3):
    d, rs = O.dims(R, C), np.random.RandomState(seed)
    frees = [max_free + 1 + i % 6 for i in range(n)]
    return [start_with_free(d, rs, n_edges(R, C), f) for f in frees], np.array(frees)


# ---------------------------------------------------------------- 1. the tables byte for byte
@pytest.mark.parametrize("R,C,M,depths", [(4, 4, 20, [20, 19, 18, 17, 16, 9, 4, 3, 1, 0, 21, 22, 23]),
                                          (6, 6, 18, [18, 17, 16, 9, 4, 3, 1, 0, 19, 20, 21]),
                                          (2, 7, 18, [18, 17, 16, 9, 4, 3, 1, 0, 19, 20, 21])])
def test_slot_tables_equal_deep_tables_byte_for_byte(R, C, M, depths):
    from dotsboxesaz_amd.engine import Engine
    d, rs = O.dims(R, C), np.random.RandomState(R * 10 + C)
    frees = np.array([depths[i % len(depths)] for i in range(64)])
    starts = [start_with_free(d, rs, n_edges(R, C), f) for f in frees]
    x = rows_of(R, C, starts)
    pool = DeepTables(R, C, max_free=M, n_tables=64)
    e = Engine(R, C, 64, mcts_num_read=4, evaluator="formula", endgame=pool)
    e.set_positions(starts)
    e.search(1)
    assert e.counters()["error_slots"] == 0
    # F = 0 is a finished game: such a root is never searched, so it asks for no table; every other root with F <= M has one
    wants = np.nonzero((frees <= M) & (frees > 0))[0]
    assert e.endgame_stats()[0] == len(wants)
    pool.solve(x[wants])  # the attach did not need the pool; the reference tables are solved into it afterwards
    assert np.array_equal(pool.n_free, frees[wants])
    for i, slot in enumerate(wants):
        t = e.slot_table(int(slot))
        assert t["valid"] and t["n_free"] == frees[slot], slot
        assert np.array_equal(t["free_edges"], free_words(R, C, x[slot])), slot
        assert t["table"].dtype == np.int8 and t["table"].shape == (1 << frees[slot],)
        assert np.array_equal(t["table"], pool.table(i)[:1 << frees[slot]]), (slot, frees[slot])
    for slot in np.nonzero((frees > M) | (frees == 0))[0]:
        t = e.slot_table(int(slot))
        assert not t["valid"] and len(t["table"]) == 0, slot
    # a second search of the same positions keeps every table: nothing is solved again
    e.search(1)
    assert e.endgame_stats()[0] == len(wants)
    e.close()
    pool.close()


# ---------------------------------------------------------------- 2. the search equals the external search fed by the restatement
def check_search(R, C, M, starts, seed, noise, all_reads=(1, 7, 50)):
    from dotsboxesaz_amd.engine import Engine
    ref = SlotTablesRef(R, C, rows_of(R, C, starts), seed, M)
    pool = DeepTables(R, C, max_free=M)
    a = Engine(R, C, 64, mcts_num_read=50, noise=noise, evaluator="formula", endgame=pool, endgame_seed=seed)
    b = Engine(R, C, 64, mcts_num_read=50, noise=noise, evaluator="external")
    rs = np.random.RandomState(R + C)
    served = 0
    for i, reads in enumerate(all_reads):
        nz = rs.dirichlet([noise[0]] * a.A, 64) if noise[0] > 0 else None
        a.set_positions(starts)
        b.set_positions(starts)
        a.search(reads, nz)
        b.search_external(ref.evaluator(), reads, nz)
        ra, rb = a.roots(), b.roots()
        same_roots(ra, rb, what=reads)
        assert (ra["visits"].sum(axis=1) == reads).all()
        served += 64
        assert a.endgame_stats()[0] == 64 * (i + 1) and a.endgame_stats()[1] >= served
    c = a.counters()
    assert c["nn_evals"] == 0 and c["error_slots"] == 0
    a.close()
    b.close()
    pool.close()


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("noise", [(0.0, 0.0), (0.8, 0.25)])
def test_search_equals_external_search_fed_by_the_restatement(seed, noise):
    starts, frees = starts_below(4, 4, 18)
    assert (frees == 18).sum() == 4 and set(frees[4:]) == set(range(3, 18))
    check_search(4, 4, 18, starts, seed, noise)


def test_search_equals_external_search_at_20_free_edges():
    d, rs = O.dims(4, 4), np.random.RandomState(20)
    frees = [20] * 4 + [19 - i % 6 for i in range(60)]
    starts = [start_with_free(d, rs, 40, f) for f in frees[:16]]
    starts = starts + [starts[4 + i % 12] for i in range(48)]  # 16 distinct roots, four of them at F = 20
    check_search(4, 4, 20, starts, 7, (0.0, 0.0), all_reads=(7, 50))


# ---------------------------------------------------------------- 3. the two kinds agree where both apply
@pytest.mark.parametrize("R,C", [(4, 4), (2, 7), (9, 9)])  # 9x9: 200 action slots, four ballot words of the float-plane evaluator
def test_deep_attach_equals_endgame_attach_at_16(R, C):
    from dotsboxesaz_amd.engine import Engine
    starts, frees = starts_below(R, C, 16)
    g, pool = Endgame(R, C, max_free=16), DeepTables(R, C, max_free=16)
    a = Engine(R, C, 64, mcts_num_read=50, evaluator="formula", endgame=g, endgame_seed=5)
    b = Engine(R, C, 64, mcts_num_read=50, evaluator="formula", endgame=pool, endgame_seed=5)
    for e in (a, b):
        e.set_positions(starts)
        e.search(30)
    same_roots(a.roots(), b.roots(), what="search")
    assert a.endgame_stats() == b.endgame_stats() and a.endgame_stats()[0] == 64
    for slot in range(64):
        ta, tb = a.slot_table(slot), b.slot_table(slot)
        assert ta["valid"] and tb["valid"] and ta["n_free"] == tb["n_free"] == frees[slot] and ta["game"] == tb["game"]
        assert np.array_equal(ta["free_edges"], tb["free_edges"]) and np.array_equal(ta["table"], tb["table"]), slot
    a.close()
    b.close()
    rows = []
    for h in (g, pool):
        e = Engine(R, C, 32, mcts_num_read=24, noise=(0.8, 0.25), temperature={0: 1.0}, evaluator="uniform", endgame=h, endgame_seed=3, seed=13)
        e.selfplay_start(64, 0)
        e.run()
        assert e.counters()["games_finished"] == 64 and e.counters()["error_slots"] == 0
        rows.append((e.fetch_samples(), e.endgame_stats()))
        e.close()
    (ra, sa), (rb, sb) = rows
    # at least one table per game that came to a searched root with F <= 16: every game on the small boards; a 9x9 game may end
    # early (one side past half of the 81 boxes) with more edges than that still free
    acts, _ = ER.board(R, C)
    late_searched = (np.asarray(ra["x"]).reshape(len(ra["z"]), -1)[:, acts] == 0).sum(axis=1) <= 16
    late = len(np.unique(ra["game_idx"][late_searched & (ra["played"] >= 0)]))
    assert sa == sb and sa[0] >= late and late >= (1 if (R, C) == (9, 9) else 64) and set(ra) == set(rb)
    for k in ra:
        assert np.array_equal(np.ascontiguousarray(ra[k]).view(np.uint8), np.ascontiguousarray(rb[k]).view(np.uint8)), k
    g.close()
    pool.close()


# ---------------------------------------------------------------- 4. nothing else changes
def test_roots_above_max_free_are_untouched_and_mixed_populations():
    from dotsboxesaz_amd.engine import Engine
    R, C, M, reads = 4, 4, 18, 30
    above, _ = starts_above(R, C, M)
    pool = DeepTables(R, C, max_free=M)
    a = Engine(R, C, 64, mcts_num_read=50, evaluator="formula", endgame=pool, endgame_seed=1)
    plain = Engine(R, C, 64, mcts_num_read=50, evaluator="formula")
    ext = Engine(R, C, 64, mcts_num_read=50, evaluator="external")
    a.set_positions(above)
    plain.set_positions(above)
    a.search(reads)
    plain.search(reads)
    same_roots(a.roots(), plain.roots(), what="above")
    assert a.endgame_stats() == (0, 0)
    ca, cp = a.counters(), plain.counters()
    assert ca["expansions"] == cp["expansions"] and ca["terminal_leaves"] == cp["terminal_leaves"]
    assert not any(a.slot_table(s)["valid"] for s in range(64))
    # mixed: even slots start below max_free, odd slots above
    below, _ = starts_below(R, C, M)
    mixed = [below[i] if i % 2 == 0 else above[i] for i in range(64)]
    ref = SlotTablesRef(R, C, rows_of(R, C, mixed[0::2]), 1, M)
    for e in (a, plain, ext):
        e.set_positions(mixed)
    a.search(reads)
    plain.search(reads)
    ext.search_external(ref.evaluator(strict=False), reads)
    ra = a.roots()
    same_roots(ra, ext.roots(), slice(0, 64, 2), "mixed, below")
    same_roots(ra, plain.roots(), slice(1, 64, 2), "mixed, above")
    assert a.endgame_stats()[0] == 32
    for e in (a, plain, ext):
        e.close()
    pool.close()


# ---------------------------------------------------------------- 5. self-play
def check_selfplay_rows(R, C, M, got, stats, n_games):
    sc = score_game_tails(got, rows=R, cols=C, max_free=M, tables=32)
    n_free, solved = sc["n_free"].astype(np.int64), sc["solved"]
    assert np.array_equal(solved, n_free <= M) and solved.any()
    assert len(np.unique(got["game_idx"])) == n_games
    z, value = np.asarray(got["z"]).astype(np.int64), sc["value"].astype(np.int64)
    assert np.array_equal(z[solved], value[solved])
    keep = solved & (value >= 0)
    pi = np.asarray(got["pi"], np.float64).reshape(len(z), -1)
    assert keep.sum() > 100 and (pi[keep].max(axis=1) == 1.0).all() and ((pi[keep] != 0).sum(axis=1) == 1).all()
    assert sc["played_optimal"][keep].all() and (sc["policy_mass"][keep] == 1.0).all()
    # one table per game; a game that ends by majority before any of its rows has F <= M never asks for one.  Those games are
    # counted from the rows themselves: the smallest F of the game's rows is above M
    games = np.asarray(got["game_idx"])
    early = sum(1 for g in np.unique(games) if n_free[games == g].min() > M)
    assert stats[0] == n_games - early and len(np.unique(games[solved])) == n_games - early and early < n_games // 2 and stats[1] > 0
    assert (n_free[solved] > 16).any()  # rows only a deep table serves


@pytest.mark.parametrize("stagger", [False, True])
def test_selfplay_keeps_the_result_and_solves_once_per_game(stagger):
    from dotsboxesaz_amd.engine import Engine
    R, C, M = 5, 5, 18
    pool = DeepTables(R, C, max_free=M)
    e = Engine(R, C, 64, mcts_num_read=24, noise=(0.0, 0.0), temperature={0: 1.0}, reuse_tree=False, evaluator="uniform", endgame=pool,
               endgame_seed=3, seed=11)
    if stagger:
        e.selfplay_stagger(1 + np.arange(64) % 24)  # the slots' move boundaries fall into different steps
    e.selfplay_start(128, 0)  # not staggered: the games run in lockstep, all 64 slots ask for their table in one pass
    e.run()
    c = e.counters()
    assert c["games_finished"] == 128 and c["error_slots"] == 0
    got, stats = e.fetch_samples(), e.endgame_stats()
    check_selfplay_rows(R, C, M, got, stats, 128)
    if not stagger:  # start positions that already have F <= max_free: one table per game
        d, rs = O.dims(R, C), np.random.RandomState(R)
        book = [start_with_free(d, rs, n_edges(R, C), M - i % 4) for i in range(16)]
        e.selfplay_set_start(book, 2)
        e.selfplay_start(128, 0)
        e.run()
        c = e.counters()
        assert c["games_finished"] == 128 and c["error_slots"] == 0
        got2, stats2 = e.fetch_samples(), e.endgame_stats()
        assert stats2[0] - stats[0] == 128
        check_selfplay_rows(R, C, M, got2, (128, 1), 128)
        first = np.nonzero(got2["move_idx"] == 0)[0]
        assert len(first) == 128 and np.array_equal(np.asarray(got2["z"])[first].astype(np.int64), score_game_tails(
            got2, rows=R, cols=C, max_free=M, tables=32)["value"][first].astype(np.int64))
    e.close()
    pool.close()


# ---------------------------------------------------------------- 6. scheduling independence
def test_rows_do_not_depend_on_the_number_of_slots():
    from dotsboxesaz_amd.engine import Engine
    R, C, M = 4, 4, 18
    pool = DeepTables(R, C, max_free=M)
    rows = []
    for n_slots in (24, 96):
        e = Engine(R, C, n_slots, mcts_num_read=20, noise=(0.8, 0.25), temperature={0: 1.0}, evaluator="formula", endgame=pool, endgame_seed=2,
                   seed=5)
        e.selfplay_start(96, 0)
        e.run()
        assert e.counters()["games_finished"] == 96 and e.counters()["error_slots"] == 0
        rows.append(e.fetch_samples())
        assert e.endgame_stats()[0] >= 96
        e.close()
    pool.close()
    assert set(rows[0]) == set(rows[1]) and len(rows[0]["z"]) > 96 * 20
    for k in rows[0]:
        assert np.array_equal(np.ascontiguousarray(rows[0][k]).view(np.uint8), np.ascontiguousarray(rows[1][k]).view(np.uint8)), k


# ---------------------------------------------------------------- 7. the read cap, waves and match play
def test_endgame_reads_caps_the_driver_rule_for_served_searches_only():
    from dotsboxesaz_amd.engine import Engine
    R, C, M = 4, 4, 18
    pool = DeepTables(R, C, max_free=M)
    acts, _ = ER.board(R, C)
    e = Engine(R, C, 16, mcts_num_read=40, temperature={0: 1.0}, reuse_tree=False, evaluator="uniform", endgame=pool, endgame_reads=3, seed=21)
    e.selfplay_start(16, 0)
    e.run()
    assert e.counters()["games_finished"] == 16
    got = e.fetch_samples()
    x = np.asarray(got["x"]).reshape(len(got["z"]), -1)
    left = (x[:, acts] == 0).sum(axis=1)
    reads = got["visits"].sum(axis=1)
    moved = got["played"] >= 0
    served = moved & (left <= M)
    assert served.sum() >= 16 * 8 and (reads[served] == 3).all()  # the rule gives min(4 * F!, 40) >= 4
    assert (reads[moved & (left > M)] == 40).all() and (moved & (left > M)).sum() > 16 * 10
    below, _ = starts_below(R, C, M)
    e2 = Engine(R, C, 64, mcts_num_read=40, evaluator="uniform", endgame=pool, endgame_reads=3)
    e2.set_positions(below)
    e2.search(11)  # explicit read counts are never touched
    assert (e2.roots()["visits"].sum(axis=1) == 11).all()
    e2.set_positions(below)
    e2.search()
    assert (e2.roots()["visits"].sum(axis=1) == 3).all()
    e.close()
    e2.close()
    pool.close()


@pytest.mark.parametrize("selfplay_pending", [False, True])
def test_pending_waves_find_the_optimal_move(selfplay_pending):
    from dotsboxesaz_amd.engine import Engine
    R, C, M, reads = 4, 4, 18, 50
    starts, _ = starts_below(R, C, M)
    x = rows_of(R, C, starts)
    pool = DeepTables(R, C, max_free=M, n_tables=64)
    sc = pool.solve(x).score(x, np.arange(64))
    value, q = sc["value"].astype(np.int64), sc["q"].astype(np.int64)
    assert sc["solved"].all()
    e = Engine(R, C, 64, mcts_num_read=reads, evaluator="formula", endgame=pool, max_pending_evals=8, selfplay_pending=selfplay_pending)
    e.set_positions(starts)
    e.search(reads)
    r = e.roots()
    assert e.counters()["error_slots"] == 0 and e.endgame_stats()[0] == 64
    e.close()
    pool.close()
    assert (r["visits"].sum(axis=1) == reads).all()
    top = r["visits"].argmax(axis=1)
    safe = value >= 0
    at = np.arange(64)
    seen = r["root_tv"] - 1.0  # one VIRTUAL_LOSS more than the backed-up values (test_hip_endgame_eval.py)
    assert (r["root_nv"] == reads + 1).all()
    assert safe.sum() >= 16 and (q[at, top] == q.max(axis=1))[safe].all()
    assert np.array_equal(np.sign(seen).astype(np.int64), value)


def test_match_model_with_deep_tables_holds_the_theoretical_result():
    from dotsboxesaz_amd.engine import Engine
    R, C, M = 4, 4, 18
    d, rs = O.dims(R, C), np.random.RandomState(4)
    book = [start_with_free(d, rs, 40, M - i % 6) for i in range(32)]
    pool = DeepTables(R, C, max_free=M, n_tables=64)
    e = Engine(R, C, 64, mcts_num_read=24, temperature={0: 1.0}, reuse_tree=False, match_play=True, evaluator="uniform", evaluator2="uniform",
               endgame=pool, endgame_models=(0,), endgame_seed=5, seed=9)
    e.selfplay_set_start(book, 2)
    e.selfplay_start(64, 0)
    e.run()
    c = e.counters()
    assert c["games_finished"] == 64 and c["error_slots"] == 0
    got = e.fetch_samples()
    model = got["player"].astype(np.int64) ^ (got["game_idx"].astype(np.int64) & 1)
    searched = np.unique(got["game_idx"][(model == 0) & (got["played"] >= 0)])
    assert e.endgame_stats()[0] == len(searched) and len(searched) >= 48
    e.close()
    first = np.nonzero(got["move_idx"] == 0)[0]
    assert np.array_equal(got["game_idx"][first], np.arange(64))
    x0 = np.asarray(got["x"])[first].reshape(64, -1)
    v = pool.solve(x0).score(x0, np.arange(64))["value"].astype(np.int64)
    pool.close()
    moves_first = (got["player"][first].astype(np.int64) ^ (got["game_idx"][first] & 1)) == 0
    z = got["z"][first].astype(np.int64)
    theory, result = np.where(moves_first, v, -v), np.where(moves_first, z, -z)
    assert moves_first.sum() == 32 and set(theory) >= {-1, 1}
    assert (result >= theory).all(), np.nonzero(result < theory)[0]


# ---------------------------------------------------------------- 8. errors
def test_attach_errors_and_borrowed_handle():
    from dotsboxesaz_amd.engine import Engine

    def code(fn):
        with pytest.raises(_lib.DbazError) as ei:
            fn()
        return ei.value.code

    pool = DeepTables(3, 3, max_free=18)
    e = Engine(3, 3, 2, mcts_num_read=5, evaluator="formula")
    assert code(lambda: e.slot_table(0)) == _lib.EINVAL  # nothing attached
    wrong_board = DeepTables(2, 3, max_free=10)
    assert code(lambda: e.attach_endgame(wrong_board)) == _lib.EINVAL
    wrong_board.close()
    assert code(lambda: e.attach_endgame(pool, 2)) == _lib.EINVAL
    assert code(lambda: e.attach_endgame(pool, 1)) == _lib.EINVAL  # no second model without match play
    assert code(lambda: e.attach_endgame(pool, 0, reads=-1)) == _lib.EINVAL
    assert code(lambda: Engine(3, 3, 2, evaluator="external", endgame=pool)) == _lib.EINVAL
    assert code(lambda: Engine(3, 3, 2, evaluator="solver", endgame=pool)) == _lib.EINVAL
    import torch
    if torch.cuda.device_count() > 1:
        other = DeepTables(3, 3, device=1, max_free=18)
        assert code(lambda: e.attach_endgame(other)) == _lib.EINVAL
        other.close()
    assert e.endgame_stats() == (0, 0) and code(lambda: e.slot_table(0)) == _lib.EINVAL  # none of the refused calls attached anything
    d, rs = O.dims(3, 3), np.random.RandomState(8)
    starts = [start_with_free(d, rs, 24, 18), start_with_free(d, rs, 24, 6)]
    e.set_positions(starts)
    e.search(5)
    assert e.endgame_stats() == (0, 0)
    e.attach_endgame(pool, 0, seed=2)
    e.set_positions(starts)
    e.search(5)
    assert e.endgame_stats()[0] == 2 and e.endgame_stats()[1] >= 2 and (e.roots()["visits"].sum(axis=1) == 5).all()
    assert code(lambda: e.slot_table(2)) == _lib.EINVAL and code(lambda: e.slot_table(-1)) == _lib.EINVAL
    assert e.slot_table(0)["n_free"] == 18 and e.slot_table(1)["n_free"] == 6
    # one kind and one max_free per handle: an Endgame after the DeepTables, or another max_free, is refused and changes nothing
    first = e.roots()
    g = Endgame(3, 3, max_free=16)
    assert code(lambda: e.attach_endgame(g, 0, seed=2)) == _lib.EINVAL
    for mf in (19, 17, 16):
        other = DeepTables(3, 3, max_free=mf)
        assert code(lambda: e.attach_endgame(other, 0, seed=2)) == _lib.EINVAL, mf
        other.close()
    e.set_positions(starts)
    e.search(5)
    same_roots(first, e.roots(), what="after the refused attaches")
    assert e.endgame_stats()[0] == 4
    again = DeepTables(3, 3, max_free=18)
    e.attach_endgame(again, 0, seed=2)
    e.search(5)  # the same positions, searched on: their tables were dropped and are solved again
    assert e.endgame_stats()[0] == 6 and e.counters()["error_slots"] == 0
    e.set_positions(starts)
    e.search(5)
    same_roots(first, e.roots(), what="after the re-attach")
    # the engine keeps nothing of a handle it no longer uses: replace `again` and destroy it before the next search
    third = DeepTables(3, 3, max_free=18)
    e.attach_endgame(third, 0, seed=2)
    again.close()
    e.set_positions(starts)
    e.search(5)
    same_roots(first, e.roots(), what="after the replaced handle was destroyed")
    assert e.endgame_stats()[0] == 10 and e.counters()["error_slots"] == 0
    want = pool.solve(rows_of(3, 3, starts))
    for slot in (0, 1):
        assert np.array_equal(e.slot_table(slot)["table"], want.table(slot)), slot
    again = third
    # slot tables that cannot be allocated: DBAZ_EDEVICE with the byte count, and the handle stays as it was
    big = DeepTables(3, 3, max_free=31)
    e3 = Engine(3, 3, 512, mcts_num_read=5, evaluator="formula")
    with pytest.raises(_lib.DbazError) as ei:
        e3.attach_endgame(big)
    assert ei.value.code == _lib.EDEVICE and str(512 << 31) in str(ei.value)
    assert e3.endgame_stats() == (0, 0) and code(lambda: e3.slot_table(0)) == _lib.EINVAL
    e3.attach_endgame(pool)  # still free to take either kind
    e3.set_positions([starts[i % 2] for i in range(512)])
    e3.search(5)
    assert e3.endgame_stats()[0] == 512 and e3.counters()["error_slots"] == 0
    e3.close()
    big.close()
    # the reverse order: a DeepTables after an Endgame
    e2 = Engine(3, 3, 2, mcts_num_read=5, evaluator="formula", endgame=g, endgame_seed=2)
    small = DeepTables(3, 3, max_free=16)
    assert code(lambda: e2.attach_endgame(small)) == _lib.EINVAL and code(lambda: e2.attach_endgame(pool)) == _lib.EINVAL
    small.close()
    e2.set_positions(starts)
    e2.search(5)
    assert e2.endgame_stats()[0] == 1 and not e2.slot_table(0)["valid"] and e2.slot_table(1)["n_free"] == 6  # the Endgame serves on
    assert code(lambda: e2.slot_table(2)) == _lib.EINVAL
    e2.close()
    # match play: the other model's handle must have the same max_free
    m = Engine(3, 3, 2, mcts_num_read=5, evaluator="formula", evaluator2="uniform", match_play=True, endgame=pool, endgame_models=(0,))
    wide = DeepTables(3, 3, max_free=20)
    assert code(lambda: m.attach_endgame(wide, 1)) == _lib.EINVAL
    m.attach_endgame(again, 1)
    m.close()
    wide.close()
    e.close()  # the handles are borrowed: they outlive the engine
    again.close()
    x = rows_of(3, 3, starts)
    assert np.array_equal(pool.solve(x).n_free, [18, 6])
    pool.close()
    g.close()
