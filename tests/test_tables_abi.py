"""Deep endgames in batches (include/dbaz.h dbaz_tables_*, dotsboxesaz_amd/endgame.py DeepTables): the binding and the argument
checks that never reach the device (runs without a GPU)."""
import inspect
import os
import re

import pytest

from conftest import REPO
from dotsboxesaz_amd import _lib, build
from dotsboxesaz_amd import endgame as E
from dotsboxesaz_amd.endgame import DeepTables

ARGS = dict(dbaz_tables_last_error=1, dbaz_tables_create=6, dbaz_tables_destroy=1, dbaz_tables_solve=4, dbaz_tables_info=5, dbaz_tables_roots=3,
            dbaz_tables_table=5, dbaz_tables_score=12, dbaz_tables_targets=12)


def test_tables_symbols_are_bound_with_the_documented_arguments():
    names = sorted(s for s in _lib.SYMBOLS if s.startswith("dbaz_tables_"))
    assert names == sorted(ARGS) and len(names) == 9
    L = _lib.load()
    src = open(os.path.join(REPO, "include", "dbaz.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in names:
        assert len(getattr(L, n).argtypes) == ARGS[n], n
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, src, flags=re.S).group(1)
        assert len(decl.split(",")) == ARGS[n], (n, decl)  # the header declares as many
    assert L.dbaz_tables_last_error.restype is not None and L.dbaz_tables_destroy.restype is None
    assert len([s for s in _lib.SYMBOLS if s.startswith("dbaz_deep_")]) == 8  # the single-table family is as it was
    assert _lib.ABI_VERSION == 3  # symbols were added, nothing else changed


def test_bad_arguments_rejected_before_touching_the_device():
    for kw, word in ((dict(rows=12, cols=12), "338"), (dict(rows=6, cols=6, max_free=32), "32"), (dict(rows=6, cols=6, max_free=-1), "-1"),
                     (dict(rows=6, cols=6, n_tables=-1), "n_tables -1"), (dict(rows=0, cols=3), "0x3")):
        with pytest.raises(_lib.DbazError) as ei:
            DeepTables(**kw)
        assert ei.value.code == _lib.EINVAL and word in str(ei.value), kw


def test_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        t = DeepTables(6, 6, max_free=12, n_tables=3)
        assert (t.max_free, t.n_tables, t.n_edges, t.A, t.table_bytes, t.pool_bytes, t.n_solved) == (12, 3, 84, 98, 1 << 12, 3 << 12, 0)
        d = DeepTables(6, 6, max_free=0, n_tables=0)  # the defaults; no pool yet
        assert (d.max_free, d.n_tables, d.pool_bytes) == (24, 64, 1 << 30)
        assert DeepTables(6, 6, max_free=31, n_tables=64).pool_bytes == 1 << 37  # 64 bits
        t.close()
        d.close()
        return
    with pytest.raises(_lib.DbazError) as ei:
        DeepTables(6, 6)
    assert ei.value.code == _lib.EDEVICE and "no CPU fallback" in str(ei.value)


def test_python_interface_is_the_documented_one():
    assert list(inspect.signature(DeepTables.__init__).parameters)[1:] == ["rows", "cols", "device", "max_free", "n_tables"]
    assert list(inspect.signature(DeepTables.score).parameters)[1:] == ["x", "table_of", "pi"]
    assert list(inspect.signature(DeepTables.targets).parameters)[1:] == ["x", "table_of", "pi", "z", "pi_mode", "z_mode"]
    assert inspect.signature(E.score_game_tails).parameters["tables"].default is None
    p = inspect.signature(E.game_tail_targets).parameters
    assert list(p)[:7] == ["samples", "rows", "cols", "max_free", "tables", "pi_mode", "z_mode"]
    assert (p["max_free"].default, p["tables"].default, p["pi_mode"].default, p["z_mode"].default) == (24, 64, "restrict", True)


def test_tables_code_stays_out_of_the_network_sources():
    """the nn= build hash covers NN_SOURCES: the batch plan lives in deep_batch.h, the kernels in solver.hip; src= covers both"""
    csrc = os.path.join(REPO, "dotsboxesaz_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "deep_batch.h")) and "deep_batch.h" not in build.NN_SOURCES
    assert os.path.join(csrc, "deep_batch.h") in build.source_files()
    for f in build.NN_SOURCES:
        assert "dbaz_tables" not in open(os.path.join(csrc, f)).read(), f
