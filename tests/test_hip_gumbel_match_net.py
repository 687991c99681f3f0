"""The search of each model of a match with network evaluators, against tests/gumbel_match_ref.py, and through compute_elo(search=)
and solver_match(search=).

Two small seeded ResNetZero(32 channels, 2 blocks) with different seeds are the two models; model 0 searches with the full Gumbel
rule at 16 reads, model 1 with PUCT at 24.  3x3 at 40 slots and 6x6 at 24 slots (one and two lanes per child; more than one
sixteen-game workgroup of k_select, no multiple of 16).  A subset of the games, fixed below, is replayed by the helper with the
engine's own network outputs -- each model's, asked one position at a time -- as its evaluators.  Every compared field, the visits of
either kind of row included, is compared bit for bit; the gap condition is asserted on the replayed games themselves."""
import numpy as np
import pytest

from oracle import oracle as O
import gumbel_match_ref as GM
import gumbel_ref as GR
from gumbel_match_ref import compare_game, game_rows, played

pytestmark = pytest.mark.gpu

SPECS = (dict(reads=16, gumbel=(4, GR.C_VISIT, GR.C_SCALE, True)), dict(reads=24))
NET = {(3, 3): dict(slots=40, replay=(0, 11, 22, 39)), (6, 6): dict(slots=24, replay=(3, 20))}
NET_SEEDS = (1, 2)  # torch.manual_seed of model 0's and model 1's network


def network(R, C, seed):
    import torch
    from dotsboxesaz_amd import nn as dnn
    torch.manual_seed(seed)
    return dnn.ResNetZero(dnn.resnet_params(R, C, 32, 2, 4, 8))


def asks(e, R, C, model):
    """the helper's evaluator of one model: the same engine, one position at a time, memoised"""
    memo = {}

    def hip_net(dd, st):
        x = O.features(dd, st)
        key = x.tobytes()
        if key not in memo:
            e._ck(e._L.dbaz_nn_select_model(e.h, model))
            try:
                pv = e.predict(x.astype(np.float32).reshape(1, 3, R + 1, C + 1))
            finally:
                e._L.dbaz_nn_select_model(e.h, 0)
            memo[key] = (pv[0][0].copy(), pv[1][0].copy())
        return memo[key]
    return hip_net


@pytest.mark.parametrize("R,C", list(NET))
def test_full_gumbel_against_puct_with_two_networks(R, C):
    from dotsboxesaz_amd.engine import Engine
    n = NET[(R, C)]
    assert n["slots"] > 16 and n["slots"] % 16
    e = Engine(R, C, n["slots"], mcts_num_read=32, noise=(0.0, 0.0), reuse_tree=True, evaluator="resnet", evaluator2="resnet", match_play=True,
               seed=GM.SEED, match_search=SPECS)
    try:
        for k in (0, 1):
            m = network(R, C, NET_SEEDS[k])
            e.load_state_dict(m.state_dict(), "resnet", model=k, **m.shape)
        c, gm, got = played(e, n["slots"])
        assert c["f32_fallback_evals"] == 0
        d = O.dims(R, C)
        evs = (asks(e, R, C, 0), asks(e, R, C, 1))
        probe = O.new_state(d)
        assert not np.array_equal(evs[0](d, probe)[0], evs[1](d, probe)[0])  # two networks
        refs = {gi: GM.replay(d, game_rows(got, gi), seed=GM.SEED, sims=32, reuse=True, specs=SPECS, evs=evs) for gi in n["replay"]}
    finally:
        e.close()
    for gi in n["replay"]:
        compare_game(refs[gi], game_rows(got, gi), ("%dx%d" % (R, C), "game", gi))
    gap = min(r["min_gap"] for r in refs.values())
    print("%dx%d: %d games replayed, minimum gap %g, interior picks %d"
          % (R, C, len(refs), gap, sum(r["interior_picks"] for r in refs.values())))
    assert gap >= 1e-9  # no decision of the replayed games is near a tie that a last bit of log or exp could turn
    assert sum(r["interior_picks"] for r in refs.values()) > 0
    model = (got["player"] ^ (got["game_idx"] & 1)) & 1
    assert np.array_equal(got["gumbel"], model == 0) and np.array_equal(got["gumbel_full"], model == 0)
    assert gm["rows"] == gm["searches"] == int((model == 0).sum())


def _params(channels, blocks, reads=24):
    from dotsboxesaz_amd import nn as dnn
    p = dnn.resnet_params(3, 3, channels, blocks)
    p["self_play"] = {"reuse_mcts_tree": True, "noise": [0.8, 0.25], "gumbel": {"m": 16},  # (a match drops the params' own gumbel key)
                      "mcts": {"mcts_num_read": reads, "mcts_cpuct": [1.25, 19652], "temperature": {0: 1.0, 12: 0.02}}}
    return p


def _spy(monkeypatch):
    """every Engine that closes leaves its two models' settings and its rows' flag columns behind"""
    from dotsboxesaz_amd.engine import Engine
    seen = []
    close, fetch = Engine.close, Engine.fetch_samples

    def fetch_samples(self):
        got = fetch(self)
        self._spy_rows = got
        return got

    def closing(self):
        if getattr(self, "h", None):
            seen.append(([self.match_search(k) for k in (0, 1)], getattr(self, "_spy_rows", None)))
        close(self)
    monkeypatch.setattr(Engine, "fetch_samples", fetch_samples)
    monkeypatch.setattr(Engine, "close", closing)
    return seen


def test_compute_elo_with_a_search_per_model(monkeypatch):
    import torch
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd.self_play import compute_elo
    seen = _spy(monkeypatch)
    pa, pb = _params(32, 2), _params(32, 2)
    elo_params = {"n_games": 16, "self_play_override": {"reuse_mcts_tree": False, "noise": [0.0, 0.0], "mcts": {"mcts_num_read": 24}}}

    def run(**kw):
        torch.manual_seed(0)
        return compute_elo(elo_params, [pa, pb], [0, 0], (1000.0, 1000.0), nn_classes=[dnn.ResNetZero, dnn.ResNetZero], rows=3, cols=3, n_slots=8, **kw)

    search = ({"reads": 16, "gumbel": {"m": 4, "c_visit": 50, "c_scale": 1.0, "full": True, "g_scale": 0.5}}, {"reads": 24})
    e0, e1, wins1 = run(search=search)
    assert abs((e0 - 1000.0) + (e1 - 1000.0)) < 1e-9 and (np.isnan(wins1) or 0.0 <= wins1 <= 1.0)
    setting, got = seen[-1]
    assert setting == [dict(reads=16, m=4, c_visit=50.0, c_scale=1.0, full=True, g_scale=0.5), dict(reads=24, m=0, c_visit=0.0, c_scale=0.0, full=False, g_scale=0.0)]
    model = (got["player"] ^ (got["game_idx"] & 1)) & 1
    assert np.array_equal(got["gumbel"], model == 0) and np.array_equal(got["gumbel_full"], model == 0)  # only the Gumbel seat's rows carry the bits
    assert len(set(got["game_idx"])) == 16
    # without search= the match is the one of the signature without it, on the same seed; a spec of nothing is nothing
    zero = [dict(reads=0, m=0, c_visit=0.0, c_scale=0.0, full=False, g_scale=0.0)] * 2
    want = run()
    assert seen[-1][0] == zero and "gumbel" not in seen[-1][1]
    rows = seen[-1][1]
    for kw in (dict(search=None), dict(search=(None, None))):
        same = run(**kw)
        assert np.array_equal(np.array(same), np.array(want), equal_nan=True), kw
        assert seen[-1][0] == zero and set(seen[-1][1]) == set(rows), kw
        for k in rows:
            assert np.array_equal(rows[k], seen[-1][1][k]), (kw, k)


def test_solver_match_with_a_search_for_the_network(monkeypatch):
    import torch
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd.self_play import solver_match
    from dotsboxesaz_amd.solver import Solver
    seen = _spy(monkeypatch)
    sv = Solver(3, 3, 0).solve()
    try:
        d = O.dims(3, 3)
        book = GR.openings(d, 4, (2, 3, 4, 5))
        params = _params(32, 2, reads=32)

        def run(**kw):
            torch.manual_seed(0)
            return solver_match(params, 0, 16, 3, 3, openings=book, solver=sv, solver_seed=1, nn_class=dnn.ResNetZero, n_slots=8, **kw)

        out = run(search={"reads": 16, "gumbel": {"m": 4, "g_scale": 0.0}})
        assert seen[-1][0] == [dict(reads=16, m=4, c_visit=50.0, c_scale=1.0, full=False, g_scale=0.0),
                               dict(reads=0, m=0, c_visit=0.0, c_scale=0.0, full=False, g_scale=0.0)]
        assert out["games"] == 16 == out["wins"] + out["draws"] + out["losses"] == sum(out["theory"].values())
        assert 0.0 <= out["held_rate"] <= 1.0 and out["held"] == round(out["held_rate"] * 16)
        got = out["samples"]
        model = (got["player"] ^ (got["game_idx"] & 1)) & 1
        assert np.array_equal(got["gumbel"], model == 0) and "gumbel_full" not in got
        want, same = run(), run(search=None)
        assert "gumbel" not in want["samples"]
        for k in ("games", "wins", "draws", "losses", "theory", "held"):
            assert want[k] == same[k], k
        for k in want["samples"]:
            assert np.array_equal(want["samples"][k], same["samples"][k]), k
    finally:
        sv.close()
