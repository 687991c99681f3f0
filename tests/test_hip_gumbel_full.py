"""The full mode of the Gumbel search in the self-play driver (dbaz_selfplay_set_gumbel_mode; gumbel_inner_scores and the mode-2
instantiations of descend, k_expand_backup and gumbel_finish in csrc/tree.hip, the rule in csrc/gumbel.h) against
tests/gumbel_full_ref.py, the Python search that test_gumbel_full_ref_cpu.py checks on its own: the engine plays the games of
gumbel_full_ref.CASES -- with the g of every ply scripted, or drawn from the rule's Philox stream -- and picks its own moves; every
row must equal the reference's bit for bit in played, q_value, the tree statistics, z and the flags (4 | 8, | 1 for a fast search),
and within +-1 count per entry in visits (device and host exp / log are not correctly rounded; the CPU test shows that no decision
of these games, interior ones included, is within 1e-9 of a tie).

Formula evaluators, 8 slots (the sixteen-game k_select), 1 to 8 games, 16 and 32 reads; one board per lanes-per-child class: 3x3,
6x6, 8x8, 10x10, and 2x7 with an m that is no power of two.  The network evaluator and the one-game k_select are
test_hip_gumbel_full_net.py's; tables, the leaf solver and start positions test_hip_gumbel_full_features.py's."""
import numpy as np
import pytest

import gumbel_full_ref as GF
import gumbel_ref as GR

pytestmark = pytest.mark.gpu

FULL = (4, GR.C_VISIT, GR.C_SCALE, True)


def make(R, C, n_slots, gumbel, *, sims=32, evaluator="formula", **kw):
    from dotsboxesaz_amd.engine import Engine
    kw.setdefault("noise", GR.NOISE)
    kw.setdefault("seed", GR.SEED)
    return Engine(R, C, n_slots, mcts_num_read=sims, evaluator=evaluator, gumbel=gumbel, **kw)


def game_rows(got, gi):
    r = np.nonzero(got["game_idx"] == gi)[0]
    assert list(got["move_idx"][r]) == list(range(len(r))), gi
    return {k: v[r] for k, v in got.items()}


def played(e, n_games, first=0):
    e.selfplay_start(n_games, first)
    e.run()
    c = e.counters()
    assert c["games_finished"] == n_games and c["error_slots"] == 0 and c["active_slots"] == 0 and c["pool_resets"] == 0
    gm = e.gumbel()
    got = e.fetch_samples()
    assert sorted(set(got["game_idx"])) == list(range(first, first + n_games))
    return c, gm, got


def packed_payload(e):
    import torch
    from dotsboxesaz_amd.self_play import _DevBuf, ROW_META
    ptr, n, rb = e.replay_rows_dev()
    packed = torch.as_tensor(_DevBuf(ptr, n * rb), device=torch.device("cuda", 0)).view(n, rb).cpu().numpy().copy()
    meta = np.ascontiguousarray(packed[:, :28]).view(ROW_META).reshape(-1)
    return packed[np.lexsort((meta["move_idx"], meta["game_idx"]))][:, :28 + 2 * e.F + 4 * e.A]


def flag_words(rows):
    return np.ascontiguousarray(rows[:, 26:28]).view("<i2").reshape(-1)


def compare(games, got, cap=None):
    """the rows of the engine against the reference's games, row by row; returns the largest difference in counts"""
    worst = 0
    for gi, g in enumerate(games):
        rows = game_rows(got, gi)
        n = min(len(rows["played"]), g["n_rows"])
        for i in range(n):  # row by row: the message names the first ply that differs
            where = ("game", gi, "ply", i, "full" if g["full"][i] else "fast", "reads", int(g["reads"][i]))
            assert rows["played"][i] == g["played"][i], where
            assert np.array_equal(rows["x"][i], g["x"][i]) and rows["player"][i] == g["player"][i], where
            assert np.float32(rows["q_value"][i]).tobytes() == np.float32(g["q_value"][i]).tobytes(), where
            for key in ("tree_size", "max_deepness", "terminal_count"):
                assert rows[key][i] == g[key][i], where + (key,)
            diff = int(np.abs(rows["visits"][i].astype(np.int64) - g["visits"][i]).max())
            worst = max(worst, diff)
            assert diff <= 1, where + (rows["visits"][i], g["visits"][i])
        assert len(rows["played"]) == g["n_rows"], gi
        assert np.array_equal(rows["z"], g["z"]), gi
        assert rows["gumbel"].all() and rows["gumbel_full"].all(), gi
        if cap is not None:
            assert np.array_equal(rows["full"], g["full"]), gi
    return worst


# ---------------------------------------------------------------- rows against the reference
@pytest.mark.parametrize("name", GF.CASE_IDS)
def test_rows_against_the_reference(name):
    """fails on a library without the feature: Engine(gumbel=(m, c_visit, c_scale, True)) finds no dbaz_selfplay_set_gumbel_mode"""
    _, R, C, sims, m, reuse, cap, g_mode, ev, n_games, c_visit, c_scale = GF.case(name)
    games = GF.case_games(name)
    e = make(R, C, 8, (m, c_visit, c_scale, True), sims=sims, evaluator=ev, reuse_tree=reuse, playout_cap=cap)
    if g_mode == "script":
        for gi, g in enumerate(games):
            e.selfplay_script(gi, np.full(g["n_rows"], -1, np.int16), g["vectors"])  # no move is forced: the rule picks
    c, gm, got = played(e, n_games)
    e.close()
    worst = compare(games, got, cap)
    print(name, "largest difference in counts", worst)
    n_rows = sum(g["n_rows"] for g in games)
    assert c["expansions"] == sum(g["n_search"] for g in games)  # the reads are the reference's, capped ones included
    assert gm == dict(m=m, c_visit=c_visit, c_scale=c_scale, searches=n_rows, rows=n_rows, full=True)


def test_flag_words_of_the_packed_rows():
    """bit 3 beside bit 2 on every row, bit 0 on the rows of the cap's fast searches"""
    from dotsboxesaz_amd import playout_cap as PC
    from dotsboxesaz_amd import self_play as sp
    assert sp.ROW_FLAG_GUMBEL_FULL == 8
    e = make(3, 3, 8, FULL, playout_cap=(0.5, 8))
    dev = sp.collect_rows_device(e, 8, 0)
    rows = sp.unpack_rows(dev.cpu().numpy(), e.F, e.A)
    e.close()
    full = PC.is_full(GR.SEED, rows["game_idx"], rows["move_idx"], 0.5)
    assert full.any() and not full.all()
    assert np.array_equal(rows["pad"], np.where(full, 12, 13))


# ---------------------------------------------------------------- the same games whatever the number of slots
def test_8_and_32_slots_play_the_same_games():
    want = None
    for n_slots in (8, 32):
        e = make(3, 3, n_slots, FULL)
        e.selfplay_start(32, 0)
        e.run()
        rows = packed_payload(e)
        e.close()
        want = rows if want is None else want
        assert np.array_equal(rows, want), n_slots


# ---------------------------------------------------------------- a twin's value is the same number
def test_transposition_hits_change_no_row():
    rows, hits = {}, {}
    for tc in ("force", False):
        e = make(3, 3, 8, FULL, transposition_cache=tc)
        e.selfplay_start(8, 0)
        e.run()
        hits[tc] = e.counters()["cache_hits"]
        rows[tc] = packed_payload(e)
        e.close()
    assert hits["force"] > 0 and hits[False] == 0
    assert np.array_equal(rows["force"], rows[False])


# ---------------------------------------------------------------- the mode alone is nothing; the modes differ
def test_mode_without_m_is_the_engine_that_was_never_told():
    want = None
    for how in ("never", "mode_only", "full_then_off"):
        e = make(3, 3, 8, None)
        if how == "mode_only":
            e._ck(e._L.dbaz_selfplay_set_gumbel_mode(e.h, 1))
        if how == "full_then_off":
            e.selfplay_set_gumbel(4, 50.0, 1.0, full=True)
            e.selfplay_set_gumbel(0)
            e._ck(e._L.dbaz_selfplay_set_gumbel_mode(e.h, 1))
        e.selfplay_start(16, 0)
        e.run()
        c = e.counters()
        rows = packed_payload(e)
        got = e.fetch_samples()
        e.close()
        assert not (flag_words(rows) & 12).any() and "gumbel" not in got and "gumbel_full" not in got
        this = (rows, {k: c[k] for k in ("expansions", "moves_played", "terminal_leaves", "steps")})
        want = this if want is None else want
        assert np.array_equal(this[0], want[0]) and this[1] == want[1], how


def test_root_only_and_full_play_different_rows():
    out = {}
    for full in (False, True):
        e = make(3, 3, 8, (4, GR.C_VISIT, GR.C_SCALE, full))
        c, gm, got = played(e, 8)
        e.close()
        assert ("full" in gm) == full and ("gumbel_full" in got) == full and got["gumbel"].all()
        out[full] = got
    a, b = out[False], out[True]
    assert len(a["played"]) != len(b["played"]) or not np.array_equal(a["played"], b["played"]) or not np.array_equal(a["visits"], b["visits"])


# ---------------------------------------------------------------- setter, getter, refusals
def test_setter_getter_and_every_refusal():
    from dotsboxesaz_amd import _lib
    from dotsboxesaz_amd.engine import Engine
    import ctypes as C
    e = Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", seed=GR.SEED)
    L = e._L

    def mode():
        m = C.c_int32(-7)
        assert L.dbaz_get_gumbel_mode(e.h, C.byref(m)) == 0
        return m.value

    assert mode() == 0 and "full" not in e.gumbel()
    e.selfplay_set_gumbel(4, 50.0, 1.0, full=True)
    assert mode() == 1 and e.gumbel() == dict(m=4, c_visit=50.0, c_scale=1.0, searches=0, rows=0, full=True)
    e.selfplay_set_gumbel(4, 50.0, 1.0)  # three arguments: the root-only mode, as always
    assert mode() == 0 and e.gumbel() == dict(m=4, c_visit=50.0, c_scale=1.0, searches=0, rows=0)
    assert L.dbaz_selfplay_set_gumbel_mode(e.h, 1) == 0 and mode() == 1
    for bad in (-1, 2, 3, 1 << 30):
        assert L.dbaz_selfplay_set_gumbel_mode(e.h, bad) == _lib.EINVAL and mode() == 1
    assert L.dbaz_get_gumbel_mode(e.h, None) == 0
    # the refusals of dbaz_selfplay_set_gumbel are what they were, and leave the mode alone
    before = e.gumbel()
    for m, cv, cs in ((-1, 50.0, 1.0), (257, 50.0, 1.0), (4, float("nan"), 1.0), (4, 50.0, 0.0)):
        with pytest.raises(_lib.DbazError) as err:
            e.selfplay_set_gumbel(m, cv, cs, full=True)
        assert err.value.code == _lib.EINVAL and e.gumbel() == before and mode() == 1
    with pytest.raises(_lib.DbazError) as err:
        e.selfplay_set_forced_playouts(2.0, True)
    assert err.value.code == _lib.EINVAL and e.gumbel() == before
    # games of an earlier start still being played
    e.selfplay_start(8, 0)
    e.step(3)
    for md in (0, 1):
        assert L.dbaz_selfplay_set_gumbel_mode(e.h, md) == _lib.ESTATE and mode() == 1
    with pytest.raises(_lib.DbazError) as err:
        e.selfplay_set_gumbel(4, 50.0, 1.0, full=False)
    assert err.value.code == _lib.ESTATE and e.gumbel()["m"] == 4 and mode() == 1
    e.run()
    gm = e.gumbel()
    got = e.fetch_samples()
    assert gm["rows"] == gm["searches"] == len(got["z"]) == int(got["gumbel_full"].sum())
    assert L.dbaz_selfplay_set_gumbel_mode(e.h, 0) == 0 and mode() == 0  # all games finished: a setting again
    e.close()
    for kw in (dict(match_play=True), dict(max_pending_evals=8, selfplay_pending=True, transposition_cache=False)):
        x = Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", **kw)
        with pytest.raises(_lib.DbazError) as err:
            x.selfplay_set_gumbel(16, 50.0, 1.0, full=True)
        assert err.value.code == _lib.EINVAL and x.gumbel() == dict(m=0, c_visit=0.0, c_scale=0.0, searches=0, rows=0)
        x.close()
        with pytest.raises(_lib.DbazError):
            Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", gumbel=FULL, **kw)


# ---------------------------------------------------------------- the Python layer
def test_params_reach_the_handle():
    from dotsboxesaz_amd import self_play as sp
    params = {"self_play": {"num_games": 8, "reuse_mcts_tree": True, "noise": GR.NOISE,
                            "mcts": {"mcts_num_read": 24, "mcts_cpuct": (1.25, 19652), "temperature": {0: 1.0}},
                            "gumbel": {"m": 8, "c_visit": 50, "c_scale": 1.0, "full": True}}}
    assert sp.engine_kwargs_from_params(params)["gumbel"] == (8, 50.0, 1.0, True)
    params["self_play"]["gumbel"]["full"] = False
    assert sp.engine_kwargs_from_params(params)["gumbel"] == (8, 50.0, 1.0)
    e = make(3, 3, 8, sp.engine_kwargs_from_params({"self_play": dict(params["self_play"], gumbel={"full": True})})["gumbel"])
    assert e.gumbel() == dict(m=16, c_visit=50.0, c_scale=1.0, searches=0, rows=0, full=True)
    e.close()
