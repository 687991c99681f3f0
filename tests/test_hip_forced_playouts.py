"""Forced playouts and policy target pruning in the self-play driver (dbaz_selfplay_set_forced_playouts; descend's root pre-pass
and advance_one in csrc/tree.hip, the rule in csrc/forced_playouts.h), against tests/forced_playouts_ref.py -- the Python search
that test_forced_playouts_ref_cpu.py pins to the oracle -- bit for bit: games generated on the CPU are scripted into the engine,
moves and per-ply Dirichlet vectors, and every row must equal the helper's in x, player, the (pruned) visits, pi, q, TreeStats, z,
`full` and `pruned`; the two counters must equal the helper's sums.

The bit-for-bit table runs the formula evaluators, which take the sixteen-game form of k_select.  The one-game form (full rounds,
eval_round > 0) exists with a network evaluator only, and the network is not restated here: that form is covered by playing the
same seeded games with and without the cut, which must give the same rows, with and without the cap and with prune on and off.

Every case: at most 32 games (40 on the network's 40 slots), at most 64 reads, boards up to 4x4 and 2x7 but for the one 6x6 run."""
import numpy as np
import pytest

from oracle import oracle as O
import forced_playouts_ref as FR

pytestmark = pytest.mark.gpu

SEED = 7
NOISE = (0.8, 0.25)
CAP = (0.5, 8)
K = 2.0


def make(R, C, n_slots, forced, *, sims=48, evaluator="formula", **kw):
    from dotsboxesaz_amd.engine import Engine
    kw.setdefault("noise", NOISE)
    kw.setdefault("seed", SEED)
    return Engine(R, C, n_slots, mcts_num_read=sims, evaluator=evaluator, forced_playouts=forced, **kw)


def game_rows(got, gi):
    r = np.nonzero(got["game_idx"] == gi)[0]
    assert list(got["move_idx"][r]) == list(range(len(r))), gi
    return {k: v[r] for k, v in got.items()}


def played(e, n_games, first=0):
    e.selfplay_start(n_games, first)
    e.run()
    c = e.counters()
    assert c["games_finished"] == n_games and c["error_slots"] == 0 and c["active_slots"] == 0 and c["pool_resets"] == 0
    fp = e.forced_playouts()
    got = e.fetch_samples()
    assert sorted(set(got["game_idx"])) == list(range(first, first + n_games))
    return c, fp, got


def same_rows(a, b):
    assert set(a) == set(b) and len(a["z"]) == len(b["z"])
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- setter and getter
def test_setter_getter_and_every_error_code():
    """fails on a library without the feature: the symbol is missing"""
    from dotsboxesaz_amd import _lib
    from dotsboxesaz_amd.engine import Engine
    assert hasattr(_lib.load(), "dbaz_selfplay_set_forced_playouts")
    e = Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", seed=SEED)
    assert e.forced_playouts() == dict(k=0.0, prune=False, rows_pruned=0, visits_pruned=0)
    e.selfplay_set_forced_playouts(2.0, True)
    assert e.forced_playouts() == dict(k=2.0, prune=True, rows_pruned=0, visits_pruned=0)
    e.selfplay_set_forced_playouts(0.5, False)
    assert (e.forced_playouts()["k"], e.forced_playouts()["prune"]) == (0.5, False)
    e.selfplay_set_forced_playouts(0.0, True)  # off: prune is not kept
    assert (e.forced_playouts()["k"], e.forced_playouts()["prune"]) == (0.0, False)
    e.selfplay_set_forced_playouts(16.0, True)
    e.selfplay_set_forced_playouts(2.0, True)
    before = e.forced_playouts()
    for k, p in ((float("nan"), 1), (-0.5, 1), (16.5, 1), (float("inf"), 0), (2.0, 2), (2.0, -1)):
        with pytest.raises(_lib.DbazError) as err:
            e._ck(e._L.dbaz_selfplay_set_forced_playouts(e.h, k, p))
        assert err.value.code == _lib.EINVAL
        assert e.forced_playouts() == before
    # games of an earlier start still being played
    e.selfplay_start(8, 0)
    e.step(3)
    with pytest.raises(_lib.DbazError) as err:
        e.selfplay_set_forced_playouts(1.0, False)
    assert err.value.code == _lib.ESTATE and (e.forced_playouts()["k"], e.forced_playouts()["prune"]) == (2.0, True)
    e.run()
    fp = e.forced_playouts()
    got = e.fetch_samples()
    assert fp["rows_pruned"] == len(got["z"]) == int(got["pruned"].sum()) and fp["visits_pruned"] > 0
    e.selfplay_set_forced_playouts(1.0, False)  # all games finished: a setting again, not consumed by a start
    assert e.forced_playouts()["rows_pruned"] == fp["rows_pruned"]  # only a start zeroes the counters
    c, fp, got = played(e, 8)
    assert (fp["k"], fp["prune"], fp["rows_pruned"], fp["visits_pruned"]) == (1.0, False, 0, 0) and "pruned" not in got
    c, fp2, got2 = played(e, 8)
    assert fp2 == fp
    same_rows(got, got2)
    e.close()
    for kw in (dict(match_play=True), dict(max_pending_evals=8, selfplay_pending=True, transposition_cache=False)):
        m = Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", **kw)
        with pytest.raises(_lib.DbazError) as err:
            m.selfplay_set_forced_playouts(2.0, True)
        assert err.value.code == _lib.EINVAL and m.forced_playouts()["k"] == 0.0
        m.close()
        with pytest.raises(_lib.DbazError):
            Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", forced_playouts=(2.0, True), **kw)
    # explicit searches with K pending evaluations are no self-play in waves: the handle takes the setting
    x = Engine(3, 3, 4, mcts_num_read=24, evaluator="formula", max_pending_evals=8, forced_playouts=(2.0, True))
    x.close()


# ---------------------------------------------------------------- bit for bit against the helper (the sixteen-game form of k_select)
KIND = {"formula": 0, "uniform": 1}
CASES = [
    # R, C, reads, k, prune, reuse, transposition table, evaluator, cap, noise
    (3, 3, 48, 2.0, True, True, False, "formula", None, NOISE),
    (3, 3, 16, 0.5, False, False, "force", "uniform", CAP, NOISE),
    (4, 4, 48, 2.0, True, True, "force", "formula", CAP, NOISE),
    (2, 7, 16, 2.0, True, False, False, "uniform", None, (0.0, 0.0)),
    (2, 7, 48, 0.5, False, True, False, "formula", CAP, NOISE),
    (4, 4, 16, 2.0, False, True, False, "formula", None, NOISE),
    (3, 3, 48, 0.5, True, False, False, "formula", CAP, NOISE),
]


@pytest.mark.parametrize("R,C,sims,k,prune,reuse,tt,ev,cap,noise", CASES)
def test_scripted_games_bit_for_bit(R, C, sims, k, prune, reuse, tt, ev, cap, noise):
    d = O.dims(R, C)
    n_games = 16
    games = [FR.generate_game(d, np.random.RandomState(100 + gi), seed=SEED, game_idx=gi, sims=sims, reuse=reuse, noise=noise, cap=cap,
                              base_ev=KIND[ev], forced_playouts=(k, prune)) for gi in range(n_games)]
    e = make(R, C, 8, (k, prune), sims=sims, evaluator=ev, reuse_tree=reuse, transposition_cache=tt, playout_cap=cap, noise=noise)
    for gi, g in enumerate(games):
        e.selfplay_script(gi, g["played"], g["vectors"])
    c, fp, got = played(e, n_games)
    e.close()
    for gi, g in enumerate(games):
        rows = game_rows(got, gi)
        assert np.array_equal(rows["played"], g["played"])
        for i in range(g["n_rows"]):  # row by row: the message names the first move that differs and its kind
            assert np.array_equal(g["visits"][i], rows["visits"][i]), ("game", gi, "ply", i, "full" if g["full"][i] else "fast", g["raw_visits"][i])
        assert FR.rows_differ(g, rows) == -1, gi
        if cap is not None:
            assert np.array_equal(rows["full"], g["full"]), gi
        if prune:
            assert np.array_equal(rows["pruned"], g["pruned"]), gi
        else:
            assert "pruned" not in rows
    assert c["expansions"] == sum(g["n_search"] for g in games)
    assert (fp["rows_pruned"], fp["visits_pruned"]) == (sum(g["rows_pruned"] for g in games), sum(g["visits_pruned"] for g in games))
    if prune:
        assert fp["visits_pruned"] > 0 and (cap is not None or fp["rows_pruned"] == len(got["z"]))
    if tt:
        assert c["cache_hits"] > 0


# ---------------------------------------------------------------- the one-game form of k_select (full rounds)
_net = {}


def net_run(cut, cap, forced, R=3, C=3, n_slots=40, n_games=40, sims=48):
    """one seeded run of a small random network; kept, shared and left unchanged"""
    key = (cut, cap, forced, R, C, n_slots, n_games, sims)
    if key not in _net:
        import torch
        from dotsboxesaz_amd import nn as dnn
        torch.manual_seed(4)
        model = dnn.ResNetZero(dnn.resnet_params(R, C, 32, 2, 4, 8))
        er, ed = (16, 15) if cut else (-1, 0)
        e = make(R, C, n_slots, forced, sims=sims, evaluator="resnet", reuse_tree=True, seed=11, playout_cap=cap, eval_round=er, eval_defer_max=ed)
        e.load_state_dict(model.state_dict(), "resnet", **model.shape)
        c, fp, got = played(e, n_games)
        e.close()
        _net[key] = (c, fp, got)
    return _net[key]


@pytest.mark.parametrize("cap", [None, CAP])
@pytest.mark.parametrize("prune", [True, False])
def test_full_rounds_play_the_same_forced_games(cap, prune):
    """the one-game k_select (the cut: put-off leaves, more steps) against the sixteen-game one: the same rows and counters"""
    cr, fr, ref = net_run(False, cap, (K, prune))
    cg, fg, got = net_run(True, cap, (K, prune))
    assert cg["steps"] > cr["steps"] and fg == fr and cg["expansions"] == cr["expansions"]
    same_rows(ref, got)
    assert ("pruned" in got) == prune and (not prune or (fg["visits_pruned"] > 0 and got["pruned"].sum() == fg["rows_pruned"]))
    # and the forcing is in these games: without it the visits are others
    _, _, off = net_run(True, cap, None)
    assert len(off["z"]) != len(got["z"]) or not np.array_equal(off["visits"], got["visits"])


# ---------------------------------------------------------------- k = 0 is today
def packed_rows(e):
    import torch
    from dotsboxesaz_amd.self_play import _DevBuf
    ptr, n, rb = e.replay_rows_dev()
    return torch.as_tensor(_DevBuf(ptr, n * rb), device=torch.device("cuda", 0)).view(n, rb).cpu().numpy().copy()


def sorted_payload(e, packed):
    from dotsboxesaz_amd.self_play import ROW_META
    meta = np.ascontiguousarray(packed[:, :28]).view(ROW_META).reshape(-1)
    return packed[np.lexsort((meta["move_idx"], meta["game_idx"]))][:, :28 + 2 * e.F + 4 * e.A]


def test_k0_is_the_engine_that_was_never_told():
    never = make(3, 3, 8, None, playout_cap=CAP)
    zero = make(3, 3, 8, (0.0, True), playout_cap=CAP)
    want = None
    for e in (never, zero):
        e.selfplay_start(32, 0)
        e.run()
        c, fp, pc = e.counters(), e.forced_playouts(), e.playout_cap()
        rows = sorted_payload(e, packed_rows(e))
        assert not (np.ascontiguousarray(rows[:, 26:28]).view("<i2") & 2).any() and "pruned" not in e.fetch_samples()
        assert (fp["k"], fp["prune"], fp["rows_pruned"], fp["visits_pruned"]) == (0.0, False, 0, 0)
        this = (rows, {k: c[k] for k in ("expansions", "moves_played", "terminal_leaves", "steps")}, pc)
        want = this if want is None else want
        assert np.array_equal(this[0], want[0]) and this[1:] == want[1:]
        e.close()


# ---------------------------------------------------------------- schedule independence
def test_8_and_32_slots_play_the_same_games():
    a, b = make(3, 3, 8, (K, True), playout_cap=CAP), make(3, 3, 32, (K, True), playout_cap=CAP)
    _, fa, ga = played(a, 32)
    _, fb, gb = played(b, 32)
    a.close()
    b.close()
    assert fa == fb and fa["visits_pruned"] > 0
    same_rows(ga, gb)


# ---------------------------------------------------------------- pruning does not steer the game
def check_pruning_only_touches_the_row(raw, cut, fp_cut):
    """raw: rows with prune = 0, cut: with prune = 1, the same seed, the production move sampling"""
    assert "pruned" not in raw and cut["pruned"].all()
    for k in raw:
        if k not in ("visits", "pi"):
            assert np.array_equal(raw[k], cut[k]), k  # the same moves, q, TreeStats, z: the same games
    v0, v1 = raw["visits"], cut["visits"]
    assert (v1 <= v0).all() and (v1 >= 0).all() and (v1.sum(axis=1) > 0).all()
    best = v0.argmax(axis=1)  # the first maximum
    rows = np.arange(len(best))
    assert np.array_equal(v1.argmax(axis=1), best) and np.array_equal(v1[rows, best], v0[rows, best])
    assert not (v1[v1 < v0] == 1).any()
    assert fp_cut["visits_pruned"] == int(v0.sum() - v1.sum()) > 0 and fp_cut["rows_pruned"] == len(best)
    assert np.array_equal(cut["pi"], v1 / v1.sum(axis=1, keepdims=True))


def test_pruning_does_not_steer_the_game():
    a, b = make(3, 3, 16, (K, False)), make(3, 3, 16, (K, True))
    _, _, raw = played(a, 32)
    _, fp, cut = played(b, 32)
    a.close()
    b.close()
    check_pruning_only_touches_the_row(raw, cut, fp)


def test_pruning_does_not_steer_the_game_6x6_network():
    """the only network case with properties of its own: 16 games, 32 reads, a random ResNetZero"""
    _, _, raw = net_run(False, None, (K, False), R=6, C=6, n_slots=16, n_games=16, sims=32)
    _, fp, cut = net_run(False, None, (K, True), R=6, C=6, n_slots=16, n_games=16, sims=32)
    check_pruning_only_touches_the_row(raw, cut, fp)


# ---------------------------------------------------------------- with an endgame table attached
def test_with_an_endgame_table():
    """the properties above with table-served searches; k = 0 equals the table-served engine that was never told.  (A bit-for-bit
    replay of this combination is not asked for: DESIGN.md section 3, "not pinned".)"""
    from dotsboxesaz_amd.endgame import Endgame
    h = Endgame(3, 3, max_free=8)
    kw = dict(transposition_cache="force", endgame=h, endgame_seed=3)
    runs = {}
    for name, forced in (("never", None), ("zero", (0.0, True)), ("raw", (K, False)), ("cut", (K, True))):
        e = make(3, 3, 16, forced, **kw)
        c, fp, got = played(e, 32)
        assert e.endgame_stats()[0] > 16  # tables solved: most games' late searches are table-served
        e.close()
        runs[name] = (c, fp, got)
    h.close()
    same_rows(runs["never"][2], runs["zero"][2])
    assert runs["never"][0]["expansions"] == runs["zero"][0]["expansions"]
    check_pruning_only_touches_the_row(runs["raw"][2], runs["cut"][2], runs["cut"][1])
    assert not np.array_equal(runs["raw"][2]["visits"], runs["never"][2]["visits"]) or len(runs["raw"][2]["z"]) != len(runs["never"][2]["z"])


# ---------------------------------------------------------------- the Python layer
def test_rows_datasets_and_params(tmp_path, monkeypatch):
    import torch
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd import self_play as sp
    from dotsboxesaz_amd.engine import Engine
    # the packed rows carry the bit through collect_rows_device / unpack_rows, and the dataset's pi is visits / sum of the pruned visits
    e = make(3, 3, 16, (K, True), playout_cap=CAP)
    dev = sp.collect_rows_device(e, 32, 0)
    rows = sp.unpack_rows(dev.cpu().numpy(), e.F, e.A)
    full = (rows["pad"] & sp.ROW_FLAG_FAST) == 0
    assert np.array_equal((rows["pad"] & sp.ROW_FLAG_PRUNED) != 0, full) and full.any() and not full.all() and not (rows["pad"] & ~3).any()
    assert e.forced_playouts()["rows_pruned"] == int(full.sum())
    e.dataset_select(3)
    e.dataset_begin()
    e.dataset_add_rows(dev, np.arange(len(dev), dtype=np.int32))
    assert e.dataset_finish(False) == len(dev)
    x, pi, z = e.dataset_fetch()
    meta = np.ascontiguousarray(dev.cpu().numpy()[:, :28]).view(sp.ROW_META).reshape(-1)
    order = np.lexsort((meta["move_idx"], meta["game_idx"]))
    vis = rows["visits"].astype(np.float64)
    assert np.array_equal(pi[order], (vis / vis.sum(axis=1, keepdims=True)).astype(np.float32))
    # fetch_samples()["pruned"] is the flag bit of the same games
    _, fp, got = played(e, 32)
    e.close()
    assert got["pruned"].dtype == bool and np.array_equal(got["pruned"], full) and np.array_equal(got["full"], full)
    assert np.array_equal(got["visits"], rows["visits"])
    # params.self_play.forced_playouts reaches the handle through generate_games
    params = dnn.resnet_params(3, 3, 32, 2, 4, 8)
    params["nn"]["model_class"] = dnn.ResNetZero
    params["nn"]["chkpts_filename"] = str(tmp_path / "model_gen{}.pt")
    params["self_play"] = {"num_games": 16, "reuse_mcts_tree": True, "noise": NOISE,
                           "mcts": {"mcts_num_read": 24, "mcts_cpuct": (1.25, 19652), "temperature": {0: 1.0, 6: 0.02}}}
    assert "forced_playouts" not in sp.engine_kwargs_from_params(params)
    torch.manual_seed(0)
    plain = sp.generate_games(None, 0, dnn.ResNetZero, 16, params, rows=3, cols=3, n_slots=16)
    params["self_play"]["forced_playouts"] = {"k": K, "prune": True}
    assert sp.engine_kwargs_from_params(params)["forced_playouts"] == (K, True)
    seen = []
    real = Engine.selfplay_set_forced_playouts

    def spy(self, k, prune=True):
        real(self, k, prune)
        seen.append(self.forced_playouts())

    monkeypatch.setattr(Engine, "selfplay_set_forced_playouts", spy)
    torch.manual_seed(0)
    forced = sp.generate_games(None, 0, dnn.ResNetZero, 16, params, rows=3, cols=3, n_slots=16)
    assert len(seen) == 1 and (seen[0]["k"], seen[0]["prune"]) == (K, True)
    assert list(forced.columns) == list(plain.columns) and not forced.equals(plain)
    with pytest.raises(Exception):
        params["self_play"]["mcts"]["max_async_searches"] = 8
        sp.generate_games(None, 0, dnn.ResNetZero, 16, params, rows=3, cols=3, n_slots=16, async_searches=True)
