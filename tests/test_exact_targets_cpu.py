"""Exact training targets (include/dbaz.h dbaz_exact_targets / dbaz_dataset_exact_targets): the numpy restatement
(targets_ref.py) against the rules of the game, its modes, and the binding and keywords of every layer (runs without a GPU)."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO
from oracle import oracle as O
from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.endgame import random_rows
import endgame_ref as ER
import targets_ref as TR
from test_endgame_cpu import negamax

_late = {}


def late(R, C, seed):
    """(rows, states, facts) of the late positions of random oracle play, built once and left unchanged"""
    if (R, C) not in _late:
        x, states = TR.late_positions(R, C, seed)
        _late[(R, C)] = (x, states, TR.solve_rows(R, C, x))
    return _late[(R, C)]


# ---------------------------------------------------------------- the definition against the rules
@pytest.mark.parametrize("R,C,seed", [(4, 4, 99), (6, 6, 264)])
def test_targets_equal_negamax_over_the_rules(R, C, seed):
    """z is the true result; the moves of O are exactly those whose successor keeps it, every other free move does worse"""
    x, states, facts = late(R, C, seed)
    d = O.dims(R, C)
    acts, _ = ER.board(R, C)
    memo, values, proper = {}, [], 0
    assert len(x) >= 60 and all(f["touched"] and f["n_free"] <= 9 for f in facts)
    for row, s, f in zip(x, states, facts):
        v = negamax(d, s, memo)
        assert f["v"] == v
        values.append(v)
        free = [a for a in acts if row[a] == 0]
        assert free == [int(a) for a in np.nonzero(O.valid_moves(d, s))[0]]
        for a in free:
            t = s.copy()
            O.play_(d, t, a)
            w = negamax(d, t, memo)
            w = w if t.to_play == s.to_play else -w
            assert (w == v) if a in f["O"] else (w < v), (a, w, v)
        proper += len(f["O"]) < len(free)
    assert set(values) == {-1, 0, 1} and proper >= 10


# ---------------------------------------------------------------- the modes
def rows_4x4():
    x = random_rows(4, 4, 40, np.arange(40) % 17, seed=3)
    acts, _ = ER.board(4, 4)
    pi = np.random.RandomState(7).rand(40, 50).astype(np.float32) * (x[:, :50] == 0)
    pi /= pi.sum(axis=1, keepdims=True).clip(1e-30)
    z = (np.arange(40) % 3 - 1).astype(np.float32)
    return x, pi.astype(np.float32), z, acts


def test_modes_of_the_reference():
    x, pi, z, acts = rows_4x4()
    facts = TR.solve_rows(4, 4, x)
    touched = np.array([f["touched"] for f in facts])
    assert touched.sum() >= 30 and (~touched).sum() >= 1
    uni, res, keep = (TR.apply_targets(facts, pi, z, m, True) for m in ("uniform", "restrict", "keep"))
    for i, f in enumerate(facts):
        if not f["touched"]:
            continue
        on = np.zeros(50, bool)
        on[f["O"]] = True
        assert abs(float(uni["pi"][i].sum(dtype=np.float64)) - 1.0) <= 1e-6 and np.array_equal(uni["pi"][i] != 0, on)
        assert (uni["pi"][i][on] == uni["pi"][i][on][0]).all()
        # restrict: zero outside O, inside the ratios of pi (each entry is one correctly rounded division by the same S)
        assert (res["pi"][i][~on] == 0).all() and res["mass"][i] > 0
        assert np.array_equal(res["pi"][i][on], pi[i][on] / res["mass"][i])
        ratio = res["pi"][i][on].astype(np.float64) * float(res["mass"][i])
        assert np.allclose(ratio, pi[i][on], rtol=2e-7, atol=0)
        assert uni["z"][i] == f["v"] and res["z"][i] == f["v"]
    assert np.array_equal(keep["pi"], pi) and np.array_equal(keep["z"], uni["z"])
    assert np.array_equal(TR.apply_targets(facts, pi, z, "uniform", False)["z"], z)
    assert np.array_equal(res["mass"], uni["mass"]) and np.array_equal(res["relabelled"], touched.astype(np.uint8))


def test_restrict_without_mass_on_the_set_falls_back_to_uniform():
    x, pi, z, acts = rows_4x4()
    facts = TR.solve_rows(4, 4, x)
    rows = [i for i, f in enumerate(facts) if f["touched"] and len(f["O"]) < f["n_free"]]
    assert len(rows) >= 10
    hot = np.zeros_like(pi)
    for i in rows:
        outside = [a for a in acts if x[i, a] == 0 and a not in facts[i]["O"]]
        hot[i, outside[0]] = 1.0
    sub = [facts[i] for i in rows]
    res = TR.apply_targets(sub, hot[rows], z[rows], "restrict", True)
    uni = TR.apply_targets(sub, hot[rows], z[rows], "uniform", True)
    assert (res["mass"] == 0).all() and np.array_equal(res["pi"], uni["pi"]) and (res["pi"].sum(axis=1) > 0.999).all()


def test_finished_and_deep_rows_come_back_unchanged():
    x = random_rows(6, 6, 54, np.arange(54) % 18, seed=5)
    acts, _ = ER.board(6, 6)
    pi = np.random.RandomState(2).rand(54, 98).astype(np.float32)
    z = (np.arange(54) % 3 - 1).astype(np.float32)
    facts = TR.solve_rows(6, 6, x)
    out = TR.apply_targets(facts, pi, z, "uniform", True)
    deep = np.array([f["n_free"] == 17 for f in facts])
    fin = np.array([f["finished"] for f in facts])
    assert deep.sum() == 3 and fin.sum() >= 1 and not (deep & fin).any()
    same = deep | fin
    assert np.array_equal(same, out["relabelled"] == 0)
    assert np.array_equal(out["pi"][same].view(np.uint32), pi[same].view(np.uint32)) and np.array_equal(out["z"][same], z[same])
    assert (out["mass"][same] == 0).all() and np.array_equal(out["n_free"], np.arange(54) % 18)
    # a smaller max_free leaves the rows above it alone as well
    small = TR.targets_ref(6, 6, x, pi, z, "uniform", True, max_free=10)
    above = (np.arange(54) % 18) > 10
    assert (small["relabelled"][above] == 0).all() and np.array_equal(small["pi"][above], pi[above])
    assert np.array_equal(small["pi"][~above], out["pi"][~above])


# ---------------------------------------------------------------- binding and keywords
def test_new_symbols_are_declared_and_bound():
    src = open(os.path.join(REPO, "include", "dbaz.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.load()
    for name, n_args in (("dbaz_exact_targets", 11), ("dbaz_dataset_exact_targets", 5)):
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert name in _lib.SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, name
        assert not name.startswith(("dbaz_endgame_", "dbaz_solver_"))


def test_every_layer_takes_the_new_keywords():
    from dotsboxesaz_amd.coach import Coach
    from dotsboxesaz_amd.endgame import Endgame
    from dotsboxesaz_amd.engine import Engine
    from dotsboxesaz_amd.train_data import ReplayDataset, ReplayStore
    p = inspect.signature(Coach.__init__).parameters
    assert p["exact_targets"].default is None and p["exact_pi"].default == "restrict" and p["exact_z"].default is True
    for fn in (ReplayStore.dataset, ReplayDataset.__init__):
        p = inspect.signature(fn).parameters
        assert p["exact"].default is None and p["exact_pi"].default == "restrict" and p["exact_z"].default is True, fn
    p = inspect.signature(Endgame.targets).parameters
    assert list(p)[1:] == ["x", "pi", "z", "pi_mode", "z_mode"] and p["pi_mode"].default == "restrict" and p["z_mode"].default is True
    assert list(inspect.signature(Engine.dataset_exact_targets).parameters)[1:] == ["endgame", "pi_mode", "z_mode"]
    from dotsboxesaz_amd.endgame import target_modes
    assert [target_modes(m, True) for m in ("keep", "uniform", "restrict")] == [(0, 1), (1, 1), (2, 1)] and target_modes("keep", False) == (0, 0)
    with pytest.raises(ValueError):
        target_modes("sharpen", True)
