"""The full mode of the Gumbel search on the host (no device): the new symbols, and dbaz_gumbel_improved_policy,
dbaz_gumbel_nonroot_pick and dbaz_gumbel_target_full -- csrc/gumbel.h, the code the kernels run -- against the rule as
tests/gumbel_full_ref.py writes it from the header's comment, on a few thousand random node rows."""
import ctypes as C

import numpy as np
import pytest

import gumbel_full_ref as GF
from dotsboxesaz_amd import _lib
from dotsboxesaz_amd import gumbel as G

NEW = ("dbaz_selfplay_set_gumbel_mode", "dbaz_get_gumbel_mode", "dbaz_gumbel_improved_policy", "dbaz_gumbel_nonroot_pick",
       "dbaz_gumbel_target_full")
KINDS = ("mixed", "zero_priors", "no_positive_prior", "S0", "all_visited", "root_f64_priors")
CONSTANTS = ((50.0, 1.0), (0.0, 0.1), (1e6, 1.0))


def test_new_symbols_are_bound_and_exported():
    """fails on a library without the feature"""
    L = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.dbaz_version() == _lib.ABI_VERSION == 3


def node(rs, A, kind):
    """one random node row: (v, P float64, W float32, n, same, valid)"""
    valid = rs.rand(A) < 0.7
    valid[rs.randint(A)] = True
    p = rs.dirichlet(np.full(A, 0.3)).astype(np.float32) * valid
    s = p.sum(dtype=np.float32)
    P = (p / s if s > 0 else p).astype(np.float64)
    if kind == "root_f64_priors":
        P = rs.dirichlet(np.full(A, 0.3)) * valid
    if kind == "zero_priors":
        P[rs.rand(A) < 0.5] = 0.0
    if kind == "no_positive_prior":
        P[:] = 0.0
    n = np.where(rs.rand(A) < 0.5, rs.randint(0, 40, A), 0) * valid
    if kind == "S0":
        n[:] = 0
    if kind == "all_visited":
        n = np.where(valid, rs.randint(1, 40, A), 0)
    same = rs.rand(A) < 0.3
    q = rs.uniform(-1, 1, A)
    W = (np.where(same, q, -q) * (1 + n)).astype(np.float32) * (n > 0)
    v = float(np.float32(rs.uniform(-1, 1)))
    return v, P, W, n.astype(np.int64), same, valid


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)).clip(min=1e-300))


@pytest.mark.parametrize("A", [1, 24, 98, 242])
def test_host_rule_against_the_python_rule(A):
    rs = np.random.RandomState(100 + A)
    rows = 0
    for kind in KINDS:
        for i in range(120 if A < 200 else 60):
            cv, cs = CONSTANTS[i % 3]
            v, P, W, n, same, valid = node(rs, A, kind)
            sgn = np.where(same, 1, -1)
            what = (A, kind, i)
            C_, x, pi = GF.improved_policy(cv, cs, v, P, W, n, sgn, valid)
            got = G.improved_policy(cv, cs, v, P, W, n, same, valid)
            assert (got[~np.isin(np.arange(A), C_)] == 0).all() and abs(got.sum() - 1.0) < 1e-12, what
            assert ulps(got[C_], np.array(pi)[C_]).max() <= 4, what
            assert G.nonroot_pick(cv, cs, v, P, W, n, same, valid) == GF.nonroot_pick(cv, cs, v, P, W, n, sgn, valid), what
            t = G.target(cv, cs, P, W, n, same, valid, v=v)
            assert np.abs(t.astype(np.int64) - GF.target_full(cv, cs, v, P, W, n, sgn, valid)).max() <= 1, what
            if kind == "all_visited":  # no unvisited candidate: v_mix is not read, whatever it is anchored on
                assert np.array_equal(G.target(cv, cs, P, W, n, same, valid, v=0.0), G.target(cv, cs, P, W, n, same, valid)), what
                assert np.array_equal(t, G.target(cv, cs, P, W, n, same, valid)), what
            rows += 1
    assert rows >= 360


def test_full_v_mix_differs_from_the_root_only_one():
    """an unvisited candidate is completed around v: pi' moves with v (in float64; at (50, 1) one child holds nearly all of the
    2^24 counts of a row, so the constants here are small), and does not where every candidate is visited"""
    rs = np.random.RandomState(5)
    moved = 0
    for i in range(50):
        v, P, W, n, same, valid = node(rs, 24, "mixed")
        unvisited = bool(((n == 0) & valid & (P > 0)).any())
        a, b = G.improved_policy(0.0, 0.1, 0.9, P, W, n, same, valid), G.improved_policy(0.0, 0.1, -0.9, P, W, n, same, valid)
        assert np.array_equal(a, b) == (not unvisited), i
        moved += unvisited
    assert moved >= 40


def test_argument_checks_and_refusals_without_a_device():
    L = _lib.load()
    mode = C.c_int32(5)
    for m in (0, 1, 2):
        assert L.dbaz_selfplay_set_gumbel_mode(None, m) == _lib.EINVAL
    assert L.dbaz_get_gumbel_mode(None, C.byref(mode)) == _lib.EINVAL and mode.value == 5
    rs = np.random.RandomState(1)
    v, P, W, n, same, valid = node(rs, 24, "mixed")
    G.improved_policy(50.0, 1.0, v, P, W, n, same, valid)
    for bad in (dict(c_visit=-1.0), dict(c_visit=1e6 + 1), dict(c_scale=0.0), dict(c_scale=1e3 + 1), dict(c_visit=float("nan")),
                dict(v=float("nan")), dict(v=float("inf"))):
        kw = dict(c_visit=50.0, c_scale=1.0, v=v)
        kw.update(bad)
        for fn in (G.improved_policy, G.nonroot_pick):
            with pytest.raises(ValueError):
                fn(kw["c_visit"], kw["c_scale"], kw["v"], P, W, n, same, valid)
        with pytest.raises(ValueError):
            G.target(kw["c_visit"], kw["c_scale"], P, W, n, same, valid, v=kw["v"])
    with pytest.raises(ValueError):
        G.improved_policy(50.0, 1.0, v, P[:-1], W, n, same, valid)
    out = np.zeros(300, np.float64)
    for A in (0, 257):
        assert L.dbaz_gumbel_improved_policy(A, 50.0, 1.0, 0.0, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data) == _lib.EINVAL
    assert L.dbaz_gumbel_nonroot_pick(24, 50.0, 1.0, 0.0, None, None, None, None, None) == _lib.EINVAL
    # no valid child: nothing to pick
    assert G.nonroot_pick(50.0, 1.0, 0.0, P, W, n, same, np.zeros(24, bool)) == -1
