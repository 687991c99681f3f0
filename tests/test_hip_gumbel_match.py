"""The search of each model of a match (dbaz_match_set_search: per-model reads, rule, constants, mode and noise scale; the per-model
loads and the per-search full bit in csrc/tree.hip) against tests/gumbel_match_ref.py, the Python restatement that
test_gumbel_match_ref_cpu.py checks on its own.  The engine plays the games of gumbel_match_ref.CASES at 16 slots and picks its own
moves; every game is replayed by the helper -- a PUCT ply's move is the engine's, a Gumbel ply's the helper's own -- and every row must
equal the replay's in the move, the visits -- a PUCT row's counts and a Gumbel row's target in units of 2^-24 alike --, q_value's
bits, the tree statistics, the flag bits and z.  counters.expansions is the replay's searches.

Formula evaluators; the network evaluator is test_hip_gumbel_match_net.py's."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
import gumbel_match_ref as GM
import gumbel_ref as GR
from gumbel_match_ref import compare_game, game_rows, played

pytestmark = pytest.mark.gpu

GUM16 = dict(reads=16, gumbel=(4, GR.C_VISIT, GR.C_SCALE))
FULL16 = dict(reads=16, gumbel=(4, GR.C_VISIT, GR.C_SCALE, True))
PUCT24 = dict(reads=24)


def make(R, C, n_slots, specs, *, sims=32, evs=("formula", "formula"), **kw):
    from dotsboxesaz_amd.engine import Engine
    kw.setdefault("seed", GM.SEED)
    return Engine(R, C, n_slots, mcts_num_read=sims, evaluator=evs[0], evaluator2=evs[1], match_play=True, match_search=specs, **kw)


def case_engine(name, n_slots=16):
    c = GM.CASES[name]
    kw = {}
    if "table" in c:
        from dotsboxesaz_amd.endgame import Endgame
        kw.update(endgame=Endgame(c["R"], c["C"], max_free=c["table"]), endgame_seed=GM.TABLE_SEED, endgame_reads=c["endgame_reads"],
                  endgame_models=(0,))
    e = make(c["R"], c["C"], n_slots, c["specs"], sims=c["sims"], evs=c["evs"], reuse_tree=c["reuse"], **kw)
    book = GM.case_book(name)
    if book:
        e.selfplay_set_start(book, 2)
    if c.get("script"):
        for gi in range(c["games"]):
            V = GM.script_vectors(name, gi)
            e.selfplay_script(gi, np.full(len(V), -1, np.int16), V)  # no move is forced
    return e, kw.get("endgame")


@pytest.mark.parametrize("name", GM.CASE_IDS)
def test_rows_against_the_replay(name):
    """fails on a library without the feature: Engine(match_search=) finds no dbaz_match_set_search"""
    c = GM.CASES[name]
    d = O.dims(c["R"], c["C"])
    e, table = case_engine(name)
    assert [e.match_search(k) for k in (0, 1)] == [dict(zip(("reads", "m", "c_visit", "c_scale", "full", "g_scale"), GM.norm_spec(s)))
                                                    for s in c["specs"]]
    cn, gm, got = played(e, c["games"])
    e.close()
    if table is not None:
        table.close()
    n_search, n_gumbel, n_rows = 0, 0, 0
    for gi in range(c["games"]):
        rows = game_rows(got, gi)
        ref = GM.replay(d, rows, **{k: v for k, v in GM.case_kw(name, gi).items() if k != "game_idx"})
        compare_game(ref, rows, (name, "game", gi))
        n_search += ref["n_search"]
        n_gumbel += ref["n_gumbel"]
        n_rows += ref["n_rows"]
        # only the Gumbel models' rows carry bit 2, and bit 3 only a full model's
        S = [GM.norm_spec(s) for s in c["specs"]]
        model = (rows["player"] ^ (gi & 1)) & 1
        assert np.array_equal(rows["flags"], np.array([4 * (S[k][1] > 0) + 8 * (S[k][1] > 0 and S[k][4]) for k in model])), gi
    assert cn["expansions"] == n_search  # the reads are the replay's: per model, capped ones included
    assert n_gumbel > 0 and n_gumbel < n_rows or all(GM.norm_spec(s)[1] > 0 for s in c["specs"])
    assert (gm["m"], gm["c_visit"], gm["c_scale"], gm["searches"], gm["rows"]) == (0, 0.0, 0.0, n_gumbel, n_gumbel)
    if name == "d":
        # deterministic models from a book of 4 openings, 2 games each: games 2k and 2k + 8 have the same opening and seating
        for k in range(4):
            a, b = game_rows(got, 2 * k), game_rows(got, 2 * k + 8)
            for key in ("x", "played", "visits", "q_value", "z", "flags"):
                assert np.array_equal(a[key], b[key]), (k, key)


# ---------------------------------------------------------------- the same games whatever the number of slots
def packed_payload(e):
    import torch
    from dotsboxesaz_amd.self_play import _DevBuf, ROW_META
    ptr, n, rb = e.replay_rows_dev()
    packed = torch.as_tensor(_DevBuf(ptr, n * rb), device=torch.device("cuda", 0)).view(n, rb).cpu().numpy().copy()
    meta = np.ascontiguousarray(packed[:, :28]).view(ROW_META).reshape(-1)
    return packed[np.lexsort((meta["move_idx"], meta["game_idx"]))][:, :28 + 2 * e.F + 4 * e.A]


def test_8_and_32_slots_play_the_same_games():
    want = None
    for n_slots in (8, 32):
        e = make(3, 3, n_slots, (FULL16, PUCT24))
        e.selfplay_start(32, 0)
        e.run()
        rows = packed_payload(e)
        e.close()
        want = rows if want is None else want
        assert np.array_equal(rows, want), n_slots


# ---------------------------------------------------------------- a setting of nothing is the handle that was never told
def test_zero_setting_is_the_handle_never_told():
    want = None
    for how in ("never", "zeros", "on_then_off"):
        e = make(3, 3, 16, None, noise=GR.NOISE)
        if how == "zeros":
            e.match_set_search(0, 0, None)
            e.match_set_search(1, 0, (0, 5.0, 5.0, True, 3.0))
        if how == "on_then_off":
            e.match_set_search(0, 16, (4, GR.C_VISIT, GR.C_SCALE, True))
            e.match_set_search(1, 8, (2, GR.C_VISIT, GR.C_SCALE))
            e.match_set_search(0, 0, None)
            e.match_set_search(1, 0, None)
        assert [e.match_search(k) for k in (0, 1)] == [dict(reads=0, m=0, c_visit=0.0, c_scale=0.0, full=False, g_scale=0.0)] * 2
        e.selfplay_start(16, 0)
        e.run()
        got = e.fetch_samples()
        assert "gumbel" not in got and "gumbel_full" not in got
        rows = packed_payload(e)
        e.close()
        want = rows if want is None else want
        assert np.array_equal(rows, want), how


# ---------------------------------------------------------------- setter, getter, refusals
def test_setter_getter_and_refusals():
    from dotsboxesaz_amd import _lib
    from dotsboxesaz_amd.engine import Engine
    e = make(3, 3, 8, None)
    e.match_set_search(0, 16, (4, 50.0, 1.0, True, 0.5))
    e.match_set_search(1, 24)
    want = [dict(reads=16, m=4, c_visit=50.0, c_scale=1.0, full=True, g_scale=0.5), dict(reads=24, m=0, c_visit=0.0, c_scale=0.0, full=False, g_scale=0.0)]
    assert [e.match_search(k) for k in (0, 1)] == want
    bad = [(2, 0, None), (-1, 0, None), (0, -1, None), (0, 33, None), (0, 0, (-1, 50.0, 1.0)), (0, 0, (257, 50.0, 1.0)),
           (0, 0, (4, -1.0, 1.0)), (0, 0, (4, 2e6, 1.0)), (0, 0, (4, float("nan"), 1.0)), (0, 0, (4, 50.0, 0.0)), (0, 0, (4, 50.0, 2e3)),
           (1, 0, (4, 50.0, 1.0, False, -0.5)), (1, 0, (4, 50.0, 1.0, False, 2e3)), (1, 0, (4, 50.0, 1.0, False, float("nan")))]
    for model, reads, g in bad:
        with pytest.raises(_lib.DbazError) as err:
            e.match_set_search(model, reads, g)
        assert err.value.code == _lib.EINVAL, (model, reads, g)
        assert [e.match_search(k) for k in (0, 1)] == want, (model, reads, g)
    rc = e._L.dbaz_match_set_search(e.h, 0, 0, 4, C.c_double(50.0), C.c_double(1.0), 2, C.c_double(1.0))  # a mode that is neither
    assert rc == _lib.EINVAL and [e.match_search(k) for k in (0, 1)] == want
    with pytest.raises(_lib.DbazError) as err:
        e.match_search(2)
    assert err.value.code == _lib.EINVAL
    # the self-play setters go on refusing a match handle, and their getters read 0 on it
    for call in (lambda: e.selfplay_set_gumbel(4, 50.0, 1.0), lambda: e.selfplay_set_playout_cap(0.5, 8), lambda: e.selfplay_set_forced_playouts(2.0, True)):
        with pytest.raises(_lib.DbazError) as err:
            call()
        assert err.value.code == _lib.EINVAL
    assert e.gumbel() == dict(m=0, c_visit=0.0, c_scale=0.0, searches=0, rows=0)
    assert [e.match_search(k) for k in (0, 1)] == want
    # ESTATE while the games of a selfplay_start are being played; the getter's answer stays
    e.selfplay_start(8, 0)
    e.step(2)
    with pytest.raises(_lib.DbazError) as err:
        e.match_set_search(1, 8)
    assert err.value.code == _lib.ESTATE and [e.match_search(k) for k in (0, 1)] == want
    e.run()
    e.match_set_search(1, 8)
    assert e.match_search(1)["reads"] == 8
    e.close()
    # a handle without match_play
    s = Engine(3, 3, 8, mcts_num_read=32, evaluator="formula")
    for call in (lambda: s.match_set_search(0, 16), lambda: s.match_search(0)):
        with pytest.raises(_lib.DbazError) as err:
            call()
        assert err.value.code == _lib.EINVAL
    s.close()
    # (selfplay_pending: dbaz_create refuses max_pending_evals > 1 on a match handle, so that refusal of the setter cannot be reached)


# ---------------------------------------------------------------- the command line
def test_match_command_line(capsys):
    """python -m dotsboxesaz_amd.gumbel --match on 3x3 with the formula evaluator: the line's counts add up, a seat against itself
    from a book (each opening once per seating, two deterministic seats) ends level, and --vs-solver adds held_rate"""
    import json
    from dotsboxesaz_amd import gumbel as G
    common = ["--rows", "3", "--cols", "3", "--match", "32", "--slots", "16", "--evaluator", "formula", "--m", "4", "--openings", "4",
              "--opening-plies", "3"]
    G.main(common + ["--seat0", "gumbel:16:g0", "--seat1", "gumbel:16:g0"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["games"] == 32 == out["wins"] + out["draws"] + out["losses"] and out["games_per_s"] > 0 and out["evals_per_game"] > 0
    assert out["wins"] == out["losses"] and out["elo_diff"] == 0.0  # the same deterministic search on both seats: every win is mirrored
    assert out["gumbel_rows"] > 0 and "held_rate" not in out
    G.main(common + ["--seat0", "gumbel:16:full", "--seat1", "puct:32"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["games"] == 32 == out["wins"] + out["draws"] + out["losses"] and out["seat1"] == "puct:32"
    G.main(common + ["--seat0", "puct:32", "--vs-solver"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["games"] == 32 == out["wins"] + out["draws"] + out["losses"] and out["seat1"] == "solver" and 0.0 <= out["held_rate"] <= 1.0
    with pytest.raises(ValueError):
        G.main(common + ["--seat0", "gumbel:16:fast"])
