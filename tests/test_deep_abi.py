"""Deep endgames (include/dbaz.h dbaz_deep_*, dotsboxesaz_amd/endgame.py DeepEndgame): the binding and the argument checks that
never reach the device (runs without a GPU)."""
import os
import re

import pytest

from conftest import REPO
from dotsboxesaz_amd import _lib, build
from dotsboxesaz_amd.endgame import DeepEndgame

ARGS = dict(dbaz_deep_last_error=1, dbaz_deep_create=5, dbaz_deep_destroy=1, dbaz_deep_solve=3, dbaz_deep_info=5, dbaz_deep_table=4,
            dbaz_deep_score=11, dbaz_deep_policy=8)


def test_deep_symbols_are_bound_with_the_documented_arguments():
    names = sorted(s for s in _lib.SYMBOLS if s.startswith("dbaz_deep_"))
    assert names == sorted(ARGS) and len(names) == 8
    L = _lib.load()
    src = open(os.path.join(REPO, "include", "dbaz.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in names:
        assert len(getattr(L, n).argtypes) == ARGS[n], n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, src, flags=re.S).group(1)
        assert len(decl.split(",")) == ARGS[n], (n, decl)  # the header declares as many
    assert L.dbaz_deep_last_error.restype is not None and L.dbaz_deep_destroy.restype is None
    assert _lib.ABI_VERSION == 3  # symbols were added, nothing else changed


def test_bad_arguments_rejected_before_touching_the_device():
    for kw, word in ((dict(rows=12, cols=12), "338"), (dict(rows=6, cols=6, max_free=32), "32"), (dict(rows=6, cols=6, max_free=-1), "-1"),
                     (dict(rows=0, cols=3), "0x3")):
        with pytest.raises(_lib.DbazError) as ei:
            DeepEndgame(**kw)
        assert ei.value.code == _lib.EINVAL and word in str(ei.value), kw


def test_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        d = DeepEndgame(6, 6)
        assert (d.max_free, d.n_edges, d.A, d.table_bytes, d.n_free) == (24, 84, 98, 1 << 24, -1)
        assert DeepEndgame(6, 6, max_free=0).max_free == 24 and DeepEndgame(6, 6, max_free=31).table_bytes == 1 << 31  # no table yet
        d.close()
        return
    with pytest.raises(_lib.DbazError) as ei:
        DeepEndgame(6, 6)
    assert ei.value.code == _lib.EDEVICE and "no CPU fallback" in str(ei.value)


def test_deep_code_stays_out_of_the_network_sources():
    """the nn= build hash covers NN_SOURCES: the deep solver lives in solver.hip and position_geo.h"""
    csrc = os.path.join(REPO, "dotsboxesaz_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "position_geo.h")) and "position_geo.h" not in build.NN_SOURCES
    for f in build.NN_SOURCES:
        assert "dbaz_deep" not in open(os.path.join(csrc, f)).read(), f
