"""Exact targets on packed replay rows (include/dbaz.h dbaz_replay_exact_targets, DeepTables.replay_targets, Coach(exact_targets=
DeepTables(...))): the binding, the Python interface, the numpy restatement of the rule (replay_targets_ref.py) against
targets_ref.apply_targets on synthetic games, and the host-only chunk plan (csrc/replay_chunks.h) compiled with g++ under
AddressSanitizer and UBSan.  Runs without a GPU."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.coach import Coach
from dotsboxesaz_amd.endgame import DeepTables
from dotsboxesaz_amd.self_play import unpack_rows
import endgame_ref as ER
import replay_targets_ref as RR
import targets_ref as TR

NAME, N_ARGS = "dbaz_replay_exact_targets", 9
PINNED = {"dbaz_tables_": 9, "dbaz_deep_": 8, "dbaz_endgame_": 4, "dbaz_solver_": 7}


# ---------------------------------------------------------------- the binding and the Python interface
def test_symbol_is_bound_with_the_documented_arguments():
    assert NAME in _lib.SYMBOLS and _lib.ABI_VERSION == 3
    L = _lib.load()
    assert len(getattr(L, NAME).argtypes) == N_ARGS
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dbaz.h")).read(), flags=re.S)
    decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % NAME, src, flags=re.S).group(1)
    assert len(decl.split(",")) == N_ARGS, decl
    for family, count in PINNED.items():  # no pinned family gained a member
        assert not NAME.startswith(family)
        assert len([s for s in _lib.SYMBOLS if s.startswith(family)]) == count, family


def test_python_interface_is_the_documented_one():
    p = inspect.signature(DeepTables.replay_targets).parameters
    assert list(p)[1:] == ["rows", "pi_mode", "z_mode", "return_roots"]
    assert (p["pi_mode"].default, p["z_mode"].default, p["return_roots"].default) == ("restrict", True, False)
    assert "clone" in DeepTables.replay_targets.__doc__ and "IN PLACE" in DeepTables.replay_targets.__doc__
    c = inspect.signature(Coach.__init__).parameters
    assert {"exact_targets", "exact_pi", "exact_z"} <= set(c)
    assert (c["exact_targets"].default, c["exact_pi"].default, c["exact_z"].default) == (None, "restrict", True)


def test_row_layout_has_one_definition():
    csrc = os.path.join(REPO, "dotsboxesaz_amd", "csrc")
    for f in ("replay.hip", "solver.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "replay_row.h"' in text and not re.search(r"#define\s+ROW_(X|Z)_OFF", text), f
    assert len(re.findall(r"#define\s+ROW_X_OFF\s+28\b", open(os.path.join(csrc, "replay_row.h")).read())) == 1


# ---------------------------------------------------------------- the rule restated, on synthetic games
def synthetic_games(R, C, seed):
    """late_positions' rows cut into games (a new game where the free edges go up again), packed with visits and z of their own:
    (packed rows, x, game, move)"""
    x, _ = TR.late_positions(R, C, seed)
    acts = ER.board(R, C)[0]
    left = (x[:, acts] == 0).sum(axis=1)
    game = np.concatenate([[0], np.cumsum(left[1:] > left[:-1])])
    move = np.concatenate([np.arange(c) for c in np.bincount(game)]) + 30
    rs = np.random.RandomState(seed)
    A = 2 * (R + 1) * (C + 1)
    visits = rs.randint(0, 40, (len(x), A)).astype(np.int32)
    visits[:, [a for a in range(A) if a not in acts]] = rs.randint(0, 3, (len(x), A - len(acts)))  # sentinel slots too
    visits[::5] = np.where(x[::5, :A] == 0, 0, visits[::5])  # every fifth row: no visit on any free edge
    z = rs.randint(-1, 2, len(x)).astype(np.int8)
    return RR.pack(R, C, game, move, x, visits, z, seed), x, game, move


@pytest.mark.parametrize("R,C,seed", [(4, 4, 99), (6, 6, 264)])
@pytest.mark.parametrize("max_free", [5, 9])
def test_restatement_equals_apply_targets(R, C, seed, max_free):
    packed, x, game, move = synthetic_games(R, C, seed)
    F, A = 3 * (R + 1) * (C + 1), 2 * (R + 1) * (C + 1)
    n = len(x)
    assert len(set(game.tolist())) >= 3
    perm = np.random.RandomState(1).permutation(n)  # the rule does not look at the rows' order
    packed, x = packed[perm], x[perm]
    facts = TR.solve_rows(R, C, x, max_free)  # touched: unfinished and F <= max_free -- in a real game, the rows from the root on
    p = RR.plan(R, C, packed, max_free, lambda root, rows: TR.solve_rows(R, C, rows, 31))
    assert (p["root_of"] >= 0).sum() == sum(f["n_free"] <= max_free for f in facts)
    if max_free == 5:
        assert (p["root_of"] < 0).any()  # rows before their game's root
    assert "unserved" not in p["status"] and "finished" not in p["status"]  # late_positions stops where a game is over
    before = unpack_rows(packed, F, A)
    meta = RR.fields(R, C, packed)[0]
    order = np.lexsort((meta["move_idx"], meta["game_idx"]))  # unpack_rows sorts: row k of `before` is packed[order[k]]
    assert np.array_equal(before["x"], x[order])
    pi0, z0 = before["pi"].astype(np.float32), before["z"].astype(np.float32)
    for pi_mode in ("restrict", "uniform", "keep"):
        for z_mode in (True, False):
            out, st = RR.apply(R, C, packed, p, pi_mode, z_mode, n_tables=3, max_free=max_free)
            want = TR.apply_targets([facts[i] for i in order], pi0, z0, pi_mode, z_mode)
            after = unpack_rows(out, F, A)
            relabelled = np.array([s == "relabel" for s in p["status"]])[order]
            assert np.array_equal(relabelled, want["relabelled"] != 0) and st["relabelled"] == relabelled.sum() >= 10
            assert np.array_equal(after["z"].astype(np.float32), want["z"]) and st["z_changed"] == want["z_changed"]
            assert np.array_equal(after["visits"] != 0, want["pi"] != 0) or pi_mode == "keep"
            if pi_mode == "keep":
                assert np.array_equal(after["visits"], before["visits"])
            if pi_mode == "uniform":
                got = after["pi"][relabelled].astype(np.float32)
                assert np.array_equal(got.view(np.uint32), want["pi"][relabelled].view(np.uint32))
            assert st["by_free"].sum() == st["relabelled"] and st["finished"] == p["status"].count("finished")
            assert (st["rows"], st["roots"], st["chunks"]) == (n, len(p["roots"]), -(-len(p["roots"]) // 3))
            # nothing but z and the visits of relabelled rows changes
            diff = np.nonzero((out != packed).any(axis=1))[0]
            assert set(diff.tolist()) <= set(np.nonzero([s == "relabel" for s in p["status"]])[0].tolist())
            keep = np.ones(out.shape[1], bool)
            keep[25] = False
            keep[28 + 2 * F:28 + 2 * F + 4 * A] = False
            assert np.array_equal(out[:, keep], packed[:, keep])
            # idempotent: the relabelled rows relabel to themselves
            again, st2 = RR.apply(R, C, out, RR.plan(R, C, out, max_free, lambda root, rows: TR.solve_rows(R, C, rows, 31)), pi_mode, z_mode, 3, max_free)
            assert np.array_equal(again, out) and st2["relabelled"] == st["relabelled"] and (st2["z_changed"] == 0 or not z_mode)


def test_restatement_refuses_a_duplicated_row_and_skips_foreign_rows():
    R, C = 4, 4
    packed, x, game, move = synthetic_games(R, C, 99)
    solve = lambda root, rows: TR.solve_rows(R, C, rows, 31)  # noqa: E731
    twice = np.concatenate([packed, packed[3:4]])
    with pytest.raises(ValueError):
        RR.plan(R, C, twice, 9, solve)
    # a late row of game 0 gets another game's position: no subset of its root's free edges
    g0, g1 = np.nonzero(game == 0)[0], np.nonzero(game == 1)[0]
    bad = packed.copy()
    F = 3 * (R + 1) * (C + 1)
    bad[g0[2], 28:28 + 2 * F] = packed[g1[0], 28:28 + 2 * F]
    p = RR.plan(R, C, bad, 9, solve)
    assert p["status"][g0[2]] == "unserved"
    out, st = RR.apply(R, C, bad, p, "uniform", True)
    assert st["unserved"] == 1 and np.array_equal(out[g0[2]], bad[g0[2]])
    assert RR.apply(R, C, packed, RR.plan(R, C, packed, 0, solve))[1]["relabelled"] == 0  # nothing is late enough: nothing to do


# ---------------------------------------------------------------- the chunk plan, compiled with g++
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "g++ builds the library's build-identity unit too: it is part of the toolchain"
    exe = tmp_path_factory.mktemp("replay_chunks") / "replay_chunks"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "dotsboxesaz_amd", "csrc"), os.path.join(REPO, "tests", "replay_chunks_main.cpp"), "-o", str(exe)],
                   check=True)
    return str(exe)


def run_plan(program, cases):
    text = "%d\n" % len(cases) + "".join("%d %d %d %d\n%s\n" % (len(g), n, mf, nt, " ".join("%d %d %d %d" % r for r in g)) for g, n, mf, nt in cases)
    r = subprocess.run([program], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # a sanitizer report ends the program with a message
    out = []
    for line in r.stdout.strip().split("\n"):
        v = [int(t) for t in line.split()]
        got, at = dict(rc=v[0]), 1
        for k in ("order", "n_free", "first", "cum", "chunk_first"):
            got[k] = v[at + 1:at + 1 + v[at]]
            at += 1 + v[at]
        assert at == len(v)
        out.append(got)
    return out


def test_chunk_plan_orders_the_roots_and_numbers_the_candidates(program):
    rs = np.random.RandomState(3)
    cases = []
    for n_games, n_tables, max_free in ((1, 1, 20), (8, 3, 20), (8, 8, 16), (40, 7, 24), (5, 64, 31), (9, 2, 0)):
        games, at = [], 0
        for g in range(n_games):
            rows = int(rs.randint(1, 30))
            rooted = rs.rand() < 0.8
            lo = int(rs.randint(0, rows))
            games.append((3 * g - 7, int(rs.randint(0, max_free + 1)) if rooted else -1, at + lo if rooted else at + rows, at + rows))
            at += rows
        cases.append((games, at, max_free, n_tables))
    got = run_plan(program, cases)
    for (games, n, max_free, n_tables), r in zip(cases, got):
        want = sorted((g for g in range(len(games)) if games[g][1] >= 0), key=lambda g: (-games[g][1], games[g][0]))
        assert r["rc"] == 0 and r["order"] == want
        assert r["n_free"] == [games[g][1] for g in want] and r["first"] == [games[g][2] for g in want]
        assert r["cum"] == np.concatenate([[0], np.cumsum([games[g][3] - games[g][2] for g in want])]).astype(int).tolist()
        assert r["chunk_first"] == list(range(0, len(want), n_tables)) + [len(want)]
        for lo, hi in zip(r["chunk_first"][:-1], r["chunk_first"][1:]):  # a chunk is in the solve plan's own order: deepest first
            assert 0 < hi - lo <= n_tables and r["n_free"][lo:hi] == sorted(r["n_free"][lo:hi], reverse=True)


def test_chunk_plan_refuses_records_that_do_not_tile_the_rows(program):
    ok = [(0, 5, 2, 6), (1, -1, 9, 9), (4, 3, 9, 12)]
    bad = [
        ([(0, 5, 2, 6), (1, -1, 9, 9), (4, 3, 9, 11)], 12, 20, 4),  # the last game ends early
        ([(0, 5, 2, 6), (1, 4, 5, 9), (4, 3, 9, 12)], 12, 20, 4),   # a root inside the previous game
        ([(0, 21, 2, 6), (1, -1, 9, 9), (4, 3, 9, 12)], 12, 20, 4),  # F past max_free
        ([(0, 5, 2, 6), (0, -1, 9, 9), (4, 3, 9, 12)], 12, 20, 4),  # game_idx does not ascend
        ([(0, 5, 6, 6), (1, -1, 9, 9), (4, 3, 9, 12)], 12, 20, 4),  # a root past its game
        (ok, 12, 20, 0), (ok, 12, 32, 4), (ok, 13, 20, 4),
    ]
    got = run_plan(program, [(ok, 12, 20, 4), ([], 0, 20, 4)] + bad)
    assert got[0]["rc"] == 0 and got[0]["order"] == [0, 2] and got[0]["cum"] == [0, 4, 7] and got[0]["chunk_first"] == [0, 2]
    assert got[1]["rc"] == 0 and got[1]["order"] == [] and got[1]["cum"] == [0] and got[1]["chunk_first"] == [0]
    for r in got[2:]:
        assert r["rc"] == -1 and not any(r[k] for k in ("order", "n_free", "first", "cum", "chunk_first"))
