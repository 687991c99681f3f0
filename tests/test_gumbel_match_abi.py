"""The search of each model of a match on the host (no device): the two new symbols in the header, in _lib.SYMBOLS, bound and
exported; what the calls answer without a handle; the CLI's seat grammar and the specs of compute_elo / solver_match."""
import ctypes as C
import os
import re

import pytest

from dotsboxesaz_amd import _lib
from dotsboxesaz_amd import gumbel as G
from dotsboxesaz_amd import self_play as sp

NEW = ("dbaz_match_set_search", "dbaz_match_get_search")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dbaz.h")


def test_new_symbols_are_declared_bound_and_exported():
    """fails on a library without the feature"""
    L = _lib.load()
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\bint %s\(dbaz_engine \*e, int32_t model," % name, text), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.dbaz_version() == _lib.ABI_VERSION == 3  # no struct changed


def test_calls_without_a_handle_are_refused():
    L = _lib.load()
    r = C.c_int32(7)
    assert L.dbaz_match_set_search(None, 0, 16, 4, C.c_double(50.0), C.c_double(1.0), 0, C.c_double(1.0)) == _lib.EINVAL
    assert L.dbaz_match_get_search(None, 0, C.byref(r), None, None, None, None, None) == _lib.EINVAL and r.value == 7


def test_seat_grammar():
    assert G.parse_seat("puct:800") == dict(reads=800)
    assert G.parse_seat("gumbel:32") == dict(reads=32, gumbel=(16, 50.0, 1.0, False, 1.0))
    assert G.parse_seat("gumbel:32:full") == dict(reads=32, gumbel=(16, 50.0, 1.0, True, 1.0))
    assert G.parse_seat("gumbel:32:g0", 4, 0.0, 0.1) == dict(reads=32, gumbel=(4, 0.0, 0.1, False, 0.0))
    assert G.parse_seat("gumbel:64:full:g0") == dict(reads=64, gumbel=(16, 50.0, 1.0, True, 0.0))
    for bad in ("puct", "puct:0", "puct:800:full", "gumbel:x", "gumbel:32:fast", "uct:32", ""):
        with pytest.raises(ValueError):
            G.parse_seat(bad)


def test_elo_difference_of_a_score():
    assert G.elo_difference(5, 0, 5) == 0.0 and G.elo_difference(0, 10, 0) == 0.0
    assert abs(G.elo_difference(3, 0, 1) - 400 * 0.47712125471966244) < 1e-9  # a score of 3/4: 400 log10(3)
    assert G.elo_difference(4, 0, 0) == float("inf") and G.elo_difference(0, 0, 4) == float("-inf")


def test_specs_of_compute_elo_and_solver_match():
    assert sp.match_search_spec(None) is None
    assert sp.match_search_spec({"reads": 800}) == {"reads": 800}
    assert sp.match_search_spec({"gumbel": {"m": 4}}) == {"reads": 0, "gumbel": (4, 50.0, 1.0, False, 1.0)}
    assert sp.match_search_spec({"reads": 32, "gumbel": {"m": 8, "c_visit": 0, "c_scale": 0.1, "full": True, "g_scale": 0}}) == \
        {"reads": 32, "gumbel": (8, 0.0, 0.1, True, 0.0)}
