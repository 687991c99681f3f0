"""Exact solver (include/dbaz.h dbaz_solver_*, dotsboxesaz_amd/solver.py): argument checks that never reach the device,
and the parts of the binding that need no table (runs without a GPU)."""
import os

import numpy as np
import pytest

from conftest import REPO
from dotsboxesaz_amd import _lib, build
from dotsboxesaz_amd.solver import Solver, edge_actions


def test_board_with_more_than_31_edges_rejected_before_touching_the_device():
    with pytest.raises(_lib.DbazError) as ei:
        Solver(4, 4)  # E = 40
    assert ei.value.code == _lib.EINVAL and "40" in str(ei.value)
    with pytest.raises(_lib.DbazError) as ei:
        Solver(2, 6)  # E = 32: one edge too many
    assert ei.value.code == _lib.EINVAL


def test_degenerate_board_rejected():
    for r, c in ((0, 3), (3, 0), (-1, 2)):
        with pytest.raises(_lib.DbazError) as ei:
            Solver(r, c)
        assert ei.value.code == _lib.EINVAL


def test_solver_symbols_are_bound():
    names = [s for s in _lib.SYMBOLS if s.startswith("dbaz_solver_")]
    assert sorted(names) == ["dbaz_solver_create", "dbaz_solver_destroy", "dbaz_solver_info", "dbaz_solver_last_error",
                             "dbaz_solver_score", "dbaz_solver_solve", "dbaz_solver_table"]
    L = _lib.load()
    for n in names:
        assert getattr(L, n).argtypes is not None, n


def test_solver_stays_out_of_the_network_sources():
    """the nn= build hash (bench.py's roofline.traffic key) covers these files: the solver must not touch them"""
    csrc = os.path.join(REPO, "dotsboxesaz_amd", "csrc")
    for f in build.NN_SOURCES:
        assert "solver" not in open(os.path.join(csrc, f)).read().lower(), f
    assert "solver.hip" in [u for u, _ in build.UNITS]


@pytest.mark.parametrize("rows,cols,n_edges", [(1, 1, 4), (2, 3, 17), (3, 2, 17), (3, 3, 24), (3, 4, 31), (1, 10, 31)])
def test_compact_edge_order(rows, cols, n_edges):
    """compact edge i = rank of the action index p*H*W + l*W + c among the real edges; sentinels board[0,:,W-1], board[1,H-1,:]"""
    H, W = rows + 1, cols + 1
    board = np.zeros((2, H, W), bool)
    board[0, :, W - 1] = True
    board[1, H - 1, :] = True
    want = np.nonzero(~board.ravel())[0]
    got = edge_actions(rows, cols)
    assert len(got) == n_edges and np.array_equal(got, want)


def test_handle_without_a_table():
    """no GPU: creation fails loudly (no CPU fallback); with one: a fresh handle reports its size and refuses to hand out a table"""
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_lib.DbazError) as ei:
            Solver(3, 3)
        assert ei.value.code == _lib.EDEVICE
        return
    s = Solver(3, 3)
    i = s.info()
    assert s.n_edges == 24 and i == dict(n_edges=24, table_bytes=1 << 24, solve_ms=-1.0, d0=-128)
    with pytest.raises(_lib.DbazError) as ei:
        s.table(0, 16)
    assert ei.value.code == _lib.ESTATE
    assert s.mask_of([0, 1, 16]) == (1 << 0 | 1 << 1 | 1 << 12) and s.mask_of([]) == 0  # action 16 = first edge of plane 1
    with pytest.raises(ValueError):
        s.mask_of([3])  # sentinel slot of plane 0
    s.close()
