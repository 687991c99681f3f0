"""Playout cap randomization in the self-play driver (dbaz_selfplay_set_playout_cap; start_move_search, begin_search and root_prep
in csrc/tree.hip), bit for bit against the CPU replay of tests/playout_cap_ref.py: every game the engine played is replayed on
one oracle tree with the reads and the `dirichlet=` that the rule gives each ply, and every row must equal the replay's in x,
player, visits, pi, q, TreeStats and z.
  (i)  noise off: the moves the engine sampled are teacher-forced into the replay
  (ii) noise on: games generated on the CPU are scripted into the engine, moves and per-ply noise vectors; the full plies use
       their vector, the fast plies ignore theirs."""
import numpy as np
import pytest

from oracle import oracle as O
import endgame_selfplay_ref as SR
import playout_cap_ref as PR

pytestmark = pytest.mark.gpu

SIMS, FAST, P, SEED = 40, 6, 0.25, 77
NOISE = (0.8, 0.25)


def make(R, C, n_slots, cap=(P, FAST), **kw):
    from dotsboxesaz_amd.engine import Engine
    kw.setdefault("mcts_num_read", SIMS)
    kw.setdefault("noise", (0.0, 0.0))
    kw.setdefault("seed", SEED)
    return Engine(R, C, n_slots, evaluator="formula", playout_cap=cap, **kw)


def game_rows(got, gi):
    r = np.nonzero(got["game_idx"] == gi)[0]
    assert list(got["move_idx"][r]) == list(range(len(r))), gi
    return {k: v[r] for k, v in got.items()}


def played(e, n_games, first=0):
    e.selfplay_start(n_games, first)
    e.run()
    c = e.counters()
    assert c["games_finished"] == n_games and c["error_slots"] == 0 and c["active_slots"] == 0 and c["pool_resets"] == 0
    pc = e.playout_cap()
    got = e.fetch_samples()
    assert sorted(set(got["game_idx"])) == list(range(first, first + n_games))
    return c, pc, got


def check_vs_replay(got, c, pc, games, d, what, *, cap=(P, FAST), starts=None, **kw):
    """replays every game; the counters of the run against the sums over the replays"""
    n_search = n_full = n_fast = 0
    refs = []
    for gi in games:
        rows = game_rows(got, gi)
        start = starts[gi % len(starts)] if starts else ()
        ref = PR.replay_game(d, rows["played"], seed=SEED, game_idx=gi, cap=cap, start=start, **kw)
        assert ref["n_rows"] == len(rows["played"]), (what, gi)
        for i in range(ref["n_rows"]):  # row by row: the message names the first move that differs and its kind
            assert np.array_equal(ref["visits"][i], rows["visits"][i]), (what, "game", gi, "ply", i, "full" if ref["full"][i] else "fast", int(ref["reads"][i]))
        assert PR.rows_differ(ref, rows) == -1, (what, gi)
        if "full" in rows:
            assert np.array_equal(rows["full"], ref["full"]), (what, gi)
        refs.append(ref)
        n_search += ref["n_search"]
        n_full += int(ref["full"].sum())
        n_fast += int((~ref["full"]).sum())
    assert (pc["full_searches"], pc["fast_searches"]) == (n_full, n_fast), what
    assert pc["full_searches"] + pc["fast_searches"] == c["moves_played"] == len(got["z"]), what
    assert c["expansions"] == n_search, what  # every read of every search and every root the tree did not hold
    if cap[0] not in (0.0, 1.0):
        assert n_full > 0 and n_fast > n_full, what
    return refs


# ---------------------------------------------------------------- (i) noise off, the engine's own moves
@pytest.mark.parametrize("reuse", [True, False])
@pytest.mark.parametrize("R,C,n_slots,n_games", [(3, 3, 8, 32), (2, 7, 16, 16), (6, 6, 16, 16)])
def test_sampled_games_vs_replay(R, C, n_slots, n_games, reuse):
    e = make(R, C, n_slots, reuse_tree=reuse)
    c, pc, got = played(e, n_games)
    assert pc["full_prob"] == P and pc["fast_reads"] == FAST
    e.close()
    check_vs_replay(got, c, pc, range(n_games), O.dims(R, C), "%dx%d reuse=%s" % (R, C, reuse), sims=SIMS, reuse=reuse)


def test_with_the_transposition_table():
    e = make(3, 3, 16, transposition_cache="force")
    c, pc, got = played(e, 32)
    e.close()
    assert c["cache_hits"] > 0
    check_vs_replay(got, c, pc, range(32), O.dims(3, 3), "tt", sims=SIMS, reuse=True)


def test_in_waves_of_8():
    e = make(3, 3, 16, max_pending_evals=8, selfplay_pending=True, transposition_cache=False)
    c, pc, got = played(e, 16)
    e.close()
    check_vs_replay(got, c, pc, range(16), O.dims(3, 3), "waves of 8", sims=SIMS, reuse=True, K=8)


def test_with_an_endgame_table_and_endgame_reads():
    """a served search runs min(rule, fast_reads if fast, endgame_reads) reads: both ceilings apply, and a fast search under a
    served root is still served"""
    from dotsboxesaz_amd.endgame import Endgame
    R, C, M, EG_SEED, EG_READS = 3, 3, 8, 3, 10
    h = Endgame(R, C, max_free=M)
    e = make(R, C, 16, transposition_cache="force", endgame=h, endgame_seed=EG_SEED, endgame_reads=EG_READS)
    c, pc, got = played(e, 32)
    stats = e.endgame_stats()
    e.close()
    h.close()
    refs = check_vs_replay(got, c, pc, range(32), O.dims(R, C), "endgame", sims=SIMS, reuse=True, table=SR.Table(R, C, M, EG_SEED),
                           endgame_reads=EG_READS)
    # either ceiling was the lower one somewhere: served fast searches of FAST reads, served full ones of EG_READS
    kinds = {(bool(f), int(r)) for ref in refs for f, r, s in zip(ref["full"], ref["reads"], ref["served"]) if s}
    assert (False, FAST) in kinds and (True, EG_READS) in kinds and stats[0] == 32


def test_from_an_opening_book_the_ply_counts_from_the_start():
    starts = [[0, 5, 9], [1], [2, 6, 12, 17, 8]]
    e = make(3, 3, 8)
    e.selfplay_set_start(starts, 1)
    c, pc, got = played(e, 24)
    e.close()
    check_vs_replay(got, c, pc, range(24), O.dims(3, 3), "book", sims=SIMS, reuse=True, starts=starts)


# ---------------------------------------------------------------- (ii) noise on, games scripted from the CPU
@pytest.mark.parametrize("R,C,n_games", [(3, 3, 16), (6, 6, 16)])
def test_scripted_noise_full_plies_use_it_fast_plies_ignore_it(R, C, n_games):
    d = O.dims(R, C)
    games = [PR.generate_game(d, np.random.RandomState(100 + gi), seed=SEED, game_idx=gi, sims=SIMS, reuse=True, noise=NOISE, cap=(P, FAST))
             for gi in range(n_games)]
    e = make(R, C, 8, noise=NOISE)
    for gi, g in enumerate(games):
        e.selfplay_script(gi, g["played"], g["vectors"])
    c, pc, got = played(e, n_games)
    e.close()
    for gi, g in enumerate(games):
        rows = game_rows(got, gi)
        assert np.array_equal(rows["played"], g["played"])
        assert PR.rows_differ(g, rows) == -1, gi
        assert np.array_equal(rows["full"], g["full"])
    assert pc["full_searches"] == sum(int(g["full"].sum()) for g in games) and pc["fast_searches"] == sum(int((~g["full"]).sum()) for g in games)
    assert c["expansions"] == sum(g["n_search"] for g in games)


# ---------------------------------------------------------------- rows, counters, settings
def packed_rows(e):
    import torch
    from dotsboxesaz_amd.self_play import _DevBuf
    ptr, n, rb = e.replay_rows_dev()
    return torch.as_tensor(_DevBuf(ptr, n * rb), device=torch.device("cuda", 0)).view(n, rb).cpu().numpy().copy()


def sorted_payload(e, packed):
    """the packed rows in (game, ply) order without the bytes that pad a row to 8 (the engine leaves those as it found them)"""
    from dotsboxesaz_amd.self_play import ROW_META
    meta = np.ascontiguousarray(packed[:, :28]).view(ROW_META).reshape(-1)
    return packed[np.lexsort((meta["move_idx"], meta["game_idx"]))][:, :28 + 2 * e.F + 4 * e.A]


def test_pad_bit_of_every_packed_row_and_the_full_column():
    from dotsboxesaz_amd import playout_cap as PC
    from dotsboxesaz_amd.self_play import unpack_rows
    e = make(3, 3, 8)
    e.selfplay_start(32, 5)
    e.run()
    rows = unpack_rows(packed_rows(e), e.F, e.A)
    got = e.fetch_samples()
    e.close()
    full = PC.is_full(SEED, rows["game_idx"], rows["move_idx"], P)
    assert np.array_equal(rows["pad"], (~full).astype(np.int16)) and full.any() and not full.all()
    assert np.array_equal(got["full"], full) and np.array_equal(got["game_idx"], rows["game_idx"]) and got["full"].dtype == bool
    assert np.array_equal(full, [PR.is_full(SEED, g, i, P) for g, i in zip(rows["game_idx"], rows["move_idx"])])


def test_off_and_cleared_are_the_engine_without_a_cap():
    never = make(3, 3, 8, cap=None, noise=NOISE)
    off = make(3, 3, 8, cap=(1.0, 0), noise=NOISE)
    cleared = make(3, 3, 8, cap=(P, FAST), noise=NOISE)
    cleared.selfplay_set_playout_cap(1.0, 0)
    want = None
    for e in (never, off, cleared):
        assert e.playout_cap()["full_prob"] == 1.0 and e.playout_cap()["fast_reads"] == 0
        e.selfplay_start(24, 0)
        e.run()
        pc, c = e.playout_cap(), e.counters()
        assert pc["fast_searches"] == 0 and pc["full_searches"] == c["moves_played"]
        rows = sorted_payload(e, packed_rows(e))
        assert "full" not in e.fetch_samples()
        assert not rows[:, 26:28].any()  # pad stays 0
        want = rows if want is None else want
        assert np.array_equal(rows, want)
        e.close()


def test_all_fast_is_an_engine_with_that_many_reads_and_no_noise():
    a = make(3, 3, 8, cap=(0.0, FAST), noise=NOISE)
    b = make(3, 3, 8, cap=None, mcts_num_read=FAST, noise=(0.0, 0.0), nodes_per_slot=a.nodes_per_slot)
    assert a.nodes_per_slot == b.nodes_per_slot
    ca, pa, ga = played(a, 32)
    cb, pb, gb = played(b, 32)
    a.close()
    b.close()
    assert ca["pool_resets"] == 0 and cb["pool_resets"] == 0
    assert pa["full_searches"] == 0 and pa["fast_searches"] == ca["moves_played"] and not ga["full"].any()
    for k in gb:
        assert np.array_equal(ga[k], gb[k]), k
    assert ca["expansions"] == cb["expansions"]


def test_8_and_32_slots_play_the_same_games():
    a, b = make(3, 3, 8, noise=NOISE), make(3, 3, 32, noise=NOISE)
    _, pa, ga = played(a, 32)
    _, pb, gb = played(b, 32)
    a.close()
    b.close()
    assert pa == pb and set(ga) == set(gb)
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k


def test_every_error_code():
    from dotsboxesaz_amd import _lib
    from dotsboxesaz_amd.engine import Engine
    e = make(3, 3, 4, cap=(0.5, 9))
    before = e.playout_cap()
    for p, n in ((float("nan"), 5), (-0.01, 5), (1.01, 5), (0.5, 0), (0.0, -3)):
        with pytest.raises(_lib.DbazError) as err:
            e.selfplay_set_playout_cap(p, n)
        assert err.value.code == _lib.EINVAL
    assert e.playout_cap() == before and before["full_prob"] == 0.5 and before["fast_reads"] == 9
    e.selfplay_set_playout_cap(1.0, 0)  # off: fast_reads is not looked at
    e.selfplay_set_playout_cap(0.5, 9)
    # games of an earlier start still being played
    e.selfplay_start(8, 0)
    e.step(3)
    with pytest.raises(_lib.DbazError) as err:
        e.selfplay_set_playout_cap(0.25, 4)
    assert err.value.code == _lib.ESTATE and e.playout_cap()["full_prob"] == 0.5 and e.playout_cap()["fast_reads"] == 9
    e.run()
    e.selfplay_set_playout_cap(0.25, 4)  # all games finished: it is a setting again, and holds for the next start
    assert e.playout_cap()["full_prob"] == 0.25
    e.fetch_samples()
    c, pc, got = played(e, 8)
    assert pc["fast_searches"] > 0 and np.array_equal(got["full"], [PR.is_full(SEED, g, i, 0.25) for g, i in zip(got["game_idx"], got["move_idx"])])
    e.close()
    m = Engine(3, 3, 4, mcts_num_read=SIMS, evaluator="formula", match_play=True)
    with pytest.raises(_lib.DbazError) as err:
        m.selfplay_set_playout_cap(0.25, 4)
    assert err.value.code == _lib.EINVAL and m.playout_cap()["full_prob"] == 1.0
    m.close()
    with pytest.raises(_lib.DbazError):
        Engine(3, 3, 4, mcts_num_read=SIMS, evaluator="formula", match_play=True, playout_cap=(0.25, 4))
