"""The subgame geometry of one position (csrc/position_geo.h, the host side of the deep endgame solver): compiled
with g++ into a stand-alone program under AddressSanitizer and UBSan, and compared with the box masks endgame_ref.py derives
(runs without a GPU)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from dotsboxesaz_amd.endgame import random_rows
import endgame_ref as ER

NO_BOX = 0x80000000
MAX_FREE = 31


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "g++ builds the library's build-identity unit too: it is part of the toolchain"
    exe = tmp_path_factory.mktemp("position_geo") / "position_geo"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "dotsboxesaz_amd", "csrc"), os.path.join(REPO, "tests", "position_geo_main.cpp"), "-o", str(exe)],
                   check=True)
    return str(exe)


def run(program, cases):
    """cases: [(rows, cols, row)] -> [(rc, F, free set as a python int, act, other)]"""
    text = "%d\n" % len(cases) + "".join("%d %d\n%s\n" % (R, C, " ".join(str(int(v)) for v in np.asarray(x).ravel())) for R, C, x in cases)
    r = subprocess.run([program], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # a sanitizer report ends the program with a message
    out = []
    for line in r.stdout.splitlines():
        v = [int(t) for t in line.split()]
        rest = np.array(v[6:], np.int64).reshape(-1, 3)
        out.append((v[0], v[1], v[2] | v[3] << 64 | v[4] << 128 | v[5] << 192, rest[:, 0].tolist(), rest[:, 1:].tolist()))
    assert len(out) == len(cases)
    return out


def reference(R, C, x):
    """(F, free set, act, per compact edge the sorted pair of other-masks) from endgame_ref's box masks"""
    acts, boxes = ER.board(R, C)
    free = [a for a in acts if x[a] == 0]
    idx = {a: j for j, a in enumerate(free)}
    other = [[] for _ in free]
    for b in boxes:
        bm = sum(1 << idx[a] for a in b if a in idx)
        for a in b:
            if a in idx:
                other[idx[a]].append(bm & ~(1 << idx[a]))
    return len(free), sum(1 << a for a in free), free, [sorted(o + [NO_BOX] * (2 - len(o))) for o in other]


def check(got, R, C, x):
    rc, F, free_set, act, other = got
    want_F, want_set, want_act, want_other = reference(R, C, x)
    assert (F, free_set) == (want_F, want_set)
    if want_F > MAX_FREE:
        assert rc == 1 and act == [] and other == []  # reported, not truncated: F and the edge set are complete
        return
    assert rc == 0 and act == want_act and act == sorted(act)
    assert [sorted(o) for o in other] == want_other


@pytest.mark.parametrize("R,C", [(1, 1), (2, 7), (6, 6), (10, 10), (15, 7)])
def test_random_rows_equal_the_reference(program, R, C):
    E = 2 * R * C + R + C
    free = np.minimum(np.arange(40) % 33, E)  # 0 .. 32 free edges: both sides of the limit
    xs = random_rows(R, C, 40, free, seed=100 * R + C)
    got = run(program, [(R, C, x) for x in xs])
    for g, x, f in zip(got, xs, free):
        assert g[1] == f
        check(g, R, C, x)
    if E > MAX_FREE:
        assert sum(g[0] == 1 for g in got) == int((free > MAX_FREE).sum()) >= 1
    # edges that border one box have one NO_BOX entry, inner edges none (wherever the row leaves them free)
    assert any(NO_BOX in o for g in got for o in g[4])
    if R > 1 or C > 1:
        assert any(NO_BOX not in o for g in got for o in g[4])


def test_sentinel_slots_are_never_edges(program):
    """a row that holds 0 in its sentinel slots (get_features writes 1 there) has the same geometry"""
    R, C = 6, 6
    x = random_rows(R, C, 1, 12, seed=3)[0]
    acts, _ = ER.board(R, C)
    y = x.copy()
    y[np.setdiff1d(np.arange(2 * 49), acts)] = 0
    a, b = run(program, [(R, C, x), (R, C, y)])
    assert a == b and a[1] == 12
    check(b, R, C, y)


def test_empty_and_full_boards(program):
    cases = []
    for R, C in ((6, 6), (3, 3), (3, 4), (1, 1)):
        HW = (R + 1) * (C + 1)
        acts, _ = ER.board(R, C)
        empty = np.ones(3 * HW, np.int16)
        empty[acts] = 0
        empty[2 * HW:] = R * C
        full = np.ones(3 * HW, np.int16)
        full[2 * HW:] = 0
        cases += [(R, C, empty), (R, C, full)]
    got = run(program, cases)
    for g, (R, C, x) in zip(got, cases):
        check(g, R, C, x)
    assert [(g[0], g[1]) for g in got] == [(1, 84), (0, 0), (0, 24), (0, 0), (0, 31), (0, 0), (0, 4), (0, 0)]
    assert got[1][2] == 0 and got[1][3] == []  # the full board: no free edge, no compact edge
    # 3x3 from the empty board: the compact edges are the solver's, every box mask has three bits
    assert got[2][3] == ER.board(3, 3)[0] and all(bin(m).count("1") == 3 for o in got[2][4] for m in o if m != NO_BOX)


def test_an_edge_whose_box_is_otherwise_drawn_has_other_zero(program):
    """box (0, 0) of a 4x4 board with three edges drawn: its last edge completes it whatever else happens"""
    R, C = 4, 4
    HW = 25
    acts, boxes = ER.board(R, C)
    x = np.ones(3 * HW, np.int16)
    x[acts] = 0
    top, bottom, left, right = boxes[0]
    x[[top, left, right]] = 1
    x[2 * HW:] = R * C
    (g,) = run(program, [(R, C, x)])
    assert g[0] == 1 and g[1] == 37  # 40 - 3 free edges: too many, drawn further below
    drawn = [a for a in acts if x[a] == 0 and a != bottom][:10]
    x[drawn] = 1
    (g,) = run(program, [(R, C, x)])
    check(g, R, C, x)
    j = g[3].index(bottom)
    assert g[0] == 0 and g[1] == 27 and 0 in g[4][j]
    # the edge below borders a second box with free edges: its other mask is neither 0 nor NO_BOX
    assert sorted(g[4][j])[0] == 0 and sorted(g[4][j])[1] not in (0, NO_BOX)


def test_unsupported_boards(program):
    x = np.ones(3 * 13 * 13, np.int16)
    assert run(program, [(12, 12, x)])[0][0] == -1  # A = 338 > 256
    assert run(program, [(0, 3, np.ones(12, np.int16))])[0][0] == -1
