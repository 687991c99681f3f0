"""The Gumbel root search in the self-play driver (dbaz_selfplay_set_gumbel; gumbel_prep, descend's root pre-pass and gumbel_finish
in csrc/tree.hip, the rule in csrc/gumbel.h) against tests/gumbel_ref.py, the Python search that test_gumbel_ref_cpu.py checks on
its own: the engine plays the games of gumbel_ref.CASES -- with the g of every ply scripted, or drawn from the rule's Philox stream
-- and picks its own moves; every row must equal the reference's bit for bit in played, q_value, the tree statistics, z and the
flags, and within +-1 count per entry in visits (device and host exp / log are not correctly rounded; the CPU test shows that
no decision of these games is within 1e-9 of a tie).

Formula evaluators, 8 slots, 2 to 16 games, 16 and 32 reads; one board per lanes-per-child class: 3x3 (A = 32), 6x6 (A = 98),
8x8 (A = 162), 10x10 (A = 242); 1x1 with m = 256, 2x7 with m = 3, and the constants (0, 0.1) and (1e6, 1) next to (50, 1).
The network evaluator is test_hip_gumbel_net.py's, tables, the leaf solver, start positions and more slots
test_hip_gumbel_features.py's."""
import numpy as np
import pytest

from oracle import oracle as O
import endgame_selfplay_ref as ESR
import gumbel_ref as GR

pytestmark = pytest.mark.gpu

GUM = (16, GR.C_VISIT, GR.C_SCALE)
CAP = (0.5, 8)


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


def packed_rows(e):
    import torch
    from dotsboxesaz_amd.self_play import _DevBuf
    ptr, n, rb = e.replay_rows_dev()
    return torch.as_tensor(_DevBuf(ptr, n * rb), device=torch.device("cuda", 0)).view(n, rb).cpu().numpy().copy()


def sorted_payload(e, packed):
    from dotsboxesaz_amd.self_play import ROW_META
    meta = np.ascontiguousarray(packed[:, :28]).view(ROW_META).reshape(-1)
    return packed[np.lexsort((meta["move_idx"], meta["game_idx"]))][:, :28 + 2 * e.F + 4 * e.A]


# ---------------------------------------------------------------- rows against the reference
@pytest.mark.parametrize("name", GR.CASE_IDS)
def test_rows_against_the_reference(name):
    """fails on a library without the feature: Engine(gumbel=) finds no dbaz_selfplay_set_gumbel"""
    _, R, C, sims, m, reuse, cap, g_mode, ev, n_games, c_visit, c_scale = GR.case(name)
    games = GR.case_games(name)
    e = make(R, C, 8, (m, c_visit, c_scale), sims=sims, evaluator=ev, reuse_tree=reuse, playout_cap=cap)
    if g_mode == "script":
        for gi, g in enumerate(games):
            e.selfplay_script(gi, np.full(g["n_rows"], -1, np.int16), g["vectors"])  # no move is forced: the rule picks
    c, gm, got = played(e, n_games)
    e.close()
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
        assert rows["gumbel"].all(), gi
        if cap is not None:
            assert np.array_equal(rows["full"], g["full"]), gi
        vs = rows["visits"].sum(axis=1, dtype=np.int64).astype(np.float64)
        assert np.array_equal(rows["pi"], rows["visits"] / vs[:, None])
    print(name, "largest difference in counts", worst)
    n_rows = sum(g["n_rows"] for g in games)
    assert c["expansions"] == sum(g["n_search"] for g in games)  # the reads are the reference's, capped ones included
    assert (gm["m"], gm["c_visit"], gm["c_scale"], gm["searches"], gm["rows"]) == (m, c_visit, c_scale, n_rows, n_rows)


# ---------------------------------------------------------------- the playout cap: flags and reads
def test_playout_cap_flags():
    from dotsboxesaz_amd import playout_cap as PC
    from dotsboxesaz_amd import self_play as sp
    e = make(3, 3, 8, GUM, playout_cap=CAP)
    dev = sp.collect_rows_device(e, 16, 0)
    rows = sp.unpack_rows(dev.cpu().numpy(), e.F, e.A)
    pc, gm = e.playout_cap(), e.gumbel()
    e.close()
    full = PC.is_full(GR.SEED, rows["game_idx"], rows["move_idx"], CAP[0])
    assert full.any() and not full.all()
    assert np.array_equal(rows["pad"], np.where(full, sp.ROW_FLAG_GUMBEL, sp.ROW_FLAG_GUMBEL | sp.ROW_FLAG_FAST))
    assert (pc["full_searches"], pc["fast_searches"]) == (int(full.sum()), int((~full).sum()))
    assert gm["rows"] == gm["searches"] == len(full)


# ---------------------------------------------------------------- a table-served root: one candidate
def test_table_served_root_is_one_hot():
    from dotsboxesaz_amd.endgame import Endgame
    h = Endgame(3, 3)
    e = make(3, 3, 8, GUM, reuse_tree=False, endgame=h, endgame_seed=3)
    c, gm, got = played(e, 16)
    assert e.endgame_stats()[0] > 0
    e.close()
    served = ESR.free_edges(3, 3, got["x"]) <= h.max_free
    h.close()
    assert served.any() and not served.all()
    v = got["visits"][served]
    assert ((v == 1 << 24).sum(axis=1) == 1).all() and (v.sum(axis=1) == 1 << 24).all()  # m' = 1: a one-hot target
    assert np.array_equal(got["played"][served], v.argmax(axis=1))
    assert ((got["visits"][~served] > 0).sum(axis=1) > 1).any() and got["gumbel"].all()


# ---------------------------------------------------------------- off is off
def test_off_is_the_engine_that_was_never_told():
    want = None
    for how in ("never", "zero", "on_then_off"):
        e = make(3, 3, 8, None if how == "never" else (0, 50.0, 1.0), playout_cap=CAP)
        if how == "on_then_off":
            e.selfplay_set_gumbel(16, 50.0, 1.0)
            e.selfplay_set_gumbel(0)
        e.selfplay_start(32, 0)
        e.run()
        c, gm, pc = e.counters(), e.gumbel(), e.playout_cap()
        rows = sorted_payload(e, packed_rows(e))
        assert not (np.ascontiguousarray(rows[:, 26:28]).view("<i2") & 4).any() and "gumbel" not in e.fetch_samples()
        assert gm == dict(m=0, c_visit=0.0, c_scale=0.0, searches=0, rows=0)
        this = (rows, {k: c[k] for k in ("expansions", "moves_played", "terminal_leaves", "steps")}, pc)
        want = this if want is None else want
        assert np.array_equal(this[0], want[0]) and this[1:] == want[1:], how
        e.close()


# ---------------------------------------------------------------- setter, getter, refusals
def test_setter_getter_and_every_refusal():
    from dotsboxesaz_amd import _lib
    from dotsboxesaz_amd.engine import Engine
    e = Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", seed=GR.SEED)
    off = dict(m=0, c_visit=0.0, c_scale=0.0, searches=0, rows=0)
    assert e.gumbel() == off
    e.selfplay_set_gumbel()
    assert e.gumbel() == dict(m=16, c_visit=50.0, c_scale=1.0, searches=0, rows=0)
    e.selfplay_set_gumbel(0, 7.0, 7.0)  # off: the constants are not kept
    assert e.gumbel() == off
    e.selfplay_set_gumbel(256, 0.0, 1e3)
    e.selfplay_set_gumbel(4, 1e6, 0.5)
    before = e.gumbel()
    nan, inf = float("nan"), float("inf")
    for m, cv, cs in ((-1, 50.0, 1.0), (257, 50.0, 1.0), (4, nan, 1.0), (4, -0.5, 1.0), (4, 1e6 + 1, 1.0), (4, inf, 1.0), (4, 50.0, nan), (4, 50.0, 0.0),
                      (4, 50.0, -1.0), (4, 50.0, 1e3 + 1), (4, 50.0, inf)):
        with pytest.raises(_lib.DbazError) as err:
            e.selfplay_set_gumbel(m, cv, cs)
        assert err.value.code == _lib.EINVAL, (m, cv, cs)
        assert e.gumbel() == before
    # forced playouts and the Gumbel rule both own the root's pick: each refuses a handle with the other on
    with pytest.raises(_lib.DbazError) as err:
        e.selfplay_set_forced_playouts(2.0, True)
    assert err.value.code == _lib.EINVAL and e.forced_playouts()["k"] == 0.0 and e.gumbel() == before
    e.selfplay_set_forced_playouts(0.0, True)  # switching forced playouts off is no clash
    e.selfplay_set_gumbel(0)
    e.selfplay_set_forced_playouts(2.0, True)
    with pytest.raises(_lib.DbazError) as err:
        e.selfplay_set_gumbel(4, 50.0, 1.0)
    assert err.value.code == _lib.EINVAL and e.gumbel() == off and e.forced_playouts()["k"] == 2.0
    e.selfplay_set_gumbel(0)  # and neither is switching the rule off
    e.selfplay_set_forced_playouts(0.0, True)
    e.selfplay_set_gumbel(4, 50.0, 1.0)
    # games of an earlier start still being played
    e.selfplay_start(8, 0)
    e.step(3)
    for args in ((16, 50.0, 1.0), (0, 0.0, 0.0)):
        with pytest.raises(_lib.DbazError) as err:
            e.selfplay_set_gumbel(*args)
        assert err.value.code == _lib.ESTATE and e.gumbel()["m"] == 4
    e.run()
    gm = e.gumbel()
    got = e.fetch_samples()
    assert gm["rows"] == gm["searches"] == len(got["z"]) == int(got["gumbel"].sum())
    e.selfplay_set_gumbel(2, 50.0, 1.0)  # all games finished: a setting again, not consumed by a start
    assert e.gumbel()["rows"] == gm["rows"]  # only a start zeroes the counters
    e.close()
    for kw in (dict(match_play=True), dict(max_pending_evals=8, selfplay_pending=True, transposition_cache=False)):
        x = Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", **kw)
        with pytest.raises(_lib.DbazError) as err:
            x.selfplay_set_gumbel(16, 50.0, 1.0)
        assert err.value.code == _lib.EINVAL and x.gumbel() == off
        x.close()
        with pytest.raises(_lib.DbazError):
            Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", gumbel=GUM, **kw)
    with pytest.raises(_lib.DbazError):
        Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", gumbel=GUM, forced_playouts=(2.0, True))


# ---------------------------------------------------------------- the data path
def test_flagged_rows_through_the_replay_store():
    """ReplayStore.dataset(pos_average=True) on Gumbel rows: pi is visits / visits.sum(), the positions' means as numpy takes them"""
    from dotsboxesaz_amd import self_play as sp
    from dotsboxesaz_amd import train_data as TD
    from oracle import train_ref as T
    e = make(3, 3, 8, GUM)
    dev = sp.collect_rows_device(e, 16, 0)
    host = dev.cpu().numpy()
    rows = sp.unpack_rows(host, e.F, e.A)
    assert (rows["pad"] == sp.ROW_FLAG_GUMBEL).all()
    meta = np.ascontiguousarray(host[:, :28]).view(sp.ROW_META).reshape(-1)
    x = np.ascontiguousarray(host[:, 28:28 + 2 * e.F]).view("<i2").reshape(len(host), e.F)
    vis = np.ascontiguousarray(host[:, 28 + 2 * e.F:28 + 2 * e.F + 4 * e.A]).view("<i4").reshape(len(host), e.A)
    store = TD.ReplayStore(e)
    np.random.seed(5)
    store.add_generation(0, dev, train_split=0.9)
    np.random.seed(6)
    ds = store.dataset(train=True, pos_average=True)
    got = e.dataset_fetch()
    np.random.seed(6)
    locs = store.chunks[0]["train_locs"]
    take = np.random.choice(len(locs), size=len(locs), replace=False)
    f, p, v = T.assemble_dataset(x[locs[take]], vis[locs[take]], meta["z"][locs[take]], True)
    e.close()
    assert len(ds) == len(f) < len(locs)
    assert np.array_equal(got[0], f) and np.array_equal(got[1], p) and np.array_equal(got[2], v)
    # and a position seen once keeps visits / visits.sum() itself
    keys, inv, cnt = np.unique(x[locs], axis=0, return_inverse=True, return_counts=True)
    once = locs[cnt[inv.ravel()] == 1]
    want = {x[i].tobytes(): (vis[i] / vis[i].sum(dtype=np.int64)).astype(np.float32) for i in once}
    seen = 0
    for xi, pi in zip(got[0], got[1]):
        w = want.get(np.ascontiguousarray(xi, dtype=np.int16).tobytes())
        if w is not None:
            assert np.array_equal(pi, w)
            seen += 1
    assert seen == len(want) > 20


# ---------------------------------------------------------------- the Python layer
def test_params_reach_the_handle(tmp_path, monkeypatch):
    import torch
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd import self_play as sp
    from dotsboxesaz_amd.engine import Engine
    params = dnn.resnet_params(3, 3, 32, 2, 4, 8)
    params["nn"]["model_class"] = dnn.ResNetZero
    params["nn"]["chkpts_filename"] = str(tmp_path / "model_gen{}.pt")
    params["self_play"] = {"num_games": 16, "reuse_mcts_tree": True, "noise": GR.NOISE,
                           "mcts": {"mcts_num_read": 24, "mcts_cpuct": (1.25, 19652), "temperature": {0: 1.0, 6: 0.02}}}
    assert "gumbel" not in sp.engine_kwargs_from_params(params)
    torch.manual_seed(0)
    plain = sp.generate_games(None, 0, dnn.ResNetZero, 16, params, rows=3, cols=3, n_slots=16)
    params["self_play"]["gumbel"] = {"m": 8, "c_visit": 50, "c_scale": 1.0}
    assert sp.engine_kwargs_from_params(params)["gumbel"] == (8, 50.0, 1.0)
    assert sp.engine_kwargs_from_params({"self_play": dict(params["self_play"], gumbel={})})["gumbel"] == (16, 50.0, 1.0)
    seen = []
    real = Engine.selfplay_set_gumbel

    def spy(self, m=16, c_visit=50.0, c_scale=1.0):
        real(self, m, c_visit, c_scale)
        seen.append(self.gumbel())

    monkeypatch.setattr(Engine, "selfplay_set_gumbel", spy)
    torch.manual_seed(0)
    gum = sp.generate_games(None, 0, dnn.ResNetZero, 16, params, rows=3, cols=3, n_slots=16)
    assert len(seen) >= 1 and all((s["m"], s["c_visit"], s["c_scale"]) == (8, 50.0, 1.0) for s in seen)
    assert list(gum.columns) == list(plain.columns) and not gum.equals(plain)
