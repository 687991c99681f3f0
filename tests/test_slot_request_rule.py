"""slot_request_rule (csrc/endgame.h), the keep / drop / solve rule that k_endgame_table and k_slot_requests both call, run on the
host: tests/slot_request_rule_main.cpp compiled with hipcc for the host only under AddressSanitizer and UBSan (no device code, no
GPU, no preload).  The decisions are compared with what tests/slot_tables_ref.py says about the same positions: a request is KEPT
when the header's table is of the same game and serves the row (SlotTablesRef.one: served), it is SOLVED when it is not kept and
a SlotTablesRef with that max_free gives the row a table, and it is DROPPED otherwise."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
import endgame_policy_ref as PR
import endgame_ref as ER
from slot_tables_ref import SlotTablesRef

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
R, C = 4, 4  # 50 action slots, one 64-bit word; test_four_words uses all four


def words(R, C, x):
    acts, _ = ER.board(R, C)
    w = [0, 0, 0, 0]
    for a in acts:
        if x[a] == 0:
            w[a >> 6] |= 1 << (a & 63)
    return w


def want(R, C, hdr_x, hdr_game, x, game, max_free):
    """(F, keep, solve) from the numpy reference; hdr_x None: no valid table"""
    acts, _ = ER.board(R, C)
    F = int(sum(1 for a in acts if x[a] == 0))
    keep = hdr_x is not None and hdr_game == game and SlotTablesRef(R, C, [hdr_x], max_free=31).one(x)[2]
    solve = not keep and len(SlotTablesRef(R, C, [x], max_free=max_free).roots) == 1
    return F, int(keep), int(solve)


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    assert os.path.exists(HIPCC), "hipcc builds the library too: it is part of the toolchain"
    exe = tmp_path_factory.mktemp("slot_request_rule") / "slot_request_rule"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "dotsboxesaz_amd", "csrc"),
                    os.path.join(REPO, "tests", "slot_request_rule_main.cpp"), "-o", str(exe)], check=True)

    def run(cases):
        """cases: (valid, hdr_game, hdr_words, game, words, max_free) -> [(F, keep, solve)]"""
        text = "".join("%d %d %s %d %s %d\n" % (v, hg, " ".join("%x" % w for w in hw), g, " ".join("%x" % w for w in fw), mf)
                       for v, hg, hw, g, fw, mf in cases)
        r = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr  # a sanitizer report ends the program with a message
        out = [tuple(int(t) for t in line.split()) for line in r.stdout.strip().split("\n")]
        assert len(out) == len(cases)
        return out
    return run


def test_keep_drop_solve_and_the_boundaries(rule):
    x, left = PR.random_games(R, C, 2, seed=3)
    per_game = len(x) // 2
    a, b = x[:per_game], x[per_game:]  # two games; row i has per_game - 1 - i free edges
    la = left[:per_game]
    row = lambda f: a[np.nonzero(la == f)[0][0]]
    M = 12
    zero = [0, 0, 0, 0]
    cases, wants, names = [], [], []

    def add(name, hdr_x, hdr_game, x_row, game, max_free):
        cases.append((0 if hdr_x is None else 1, hdr_game, zero if hdr_x is None else words(R, C, hdr_x), game, words(R, C, x_row), max_free))
        wants.append(want(R, C, hdr_x, hdr_game, x_row, game, max_free))
        names.append(name)

    add("keep: a later row of the table's game", row(12), 5, row(9), 5, M)
    add("keep: the table's own root", row(12), 5, row(12), 5, M)
    add("keep comes first: a table that serves the row is kept whatever F is", row(14), 5, row(13), 5, M)
    add("solve: no valid table", None, 0, row(10), 5, M)
    add("solve: same edges, another game", row(12), 5, row(9), 6, M)
    add("solve: same game, not a subset", row(8), 5, row(10), 5, M)
    add("solve: same game, a non-subset of equal size (the other game's row)", row(10), 5, b[np.nonzero(left[per_game:] == 10)[0][0]], 5, M)
    add("solve: the boundary F = max_free", None, 0, row(M), 7, M)
    add("drop: the boundary F = max_free + 1", None, 0, row(M + 1), 7, M)
    add("drop: F = max_free + 1 over a table of another game", row(10), 5, row(M + 1), 6, M)
    add("drop: the opening", row(12), 5, a[0], 6, M)
    add("solve: a finished board, F = 0", None, 0, a[-1], 5, 0)
    got = rule(cases)
    for name, g, w in zip(names, got, wants):
        assert g == w, (name, g, w)
    kinds = {(k, s) for _, k, s in got}
    assert kinds == {(1, 0), (0, 1), (0, 0)}  # keep, solve and drop all occur; keep and solve never together
    assert [w[0] for w in wants][7:9] == [M, M + 1] and wants[7][1:] == (0, 1) and wants[8][1:] == (0, 0)


def test_four_words(rule):
    """sets that use all four 64-bit words, against Python integers"""
    rs = np.random.RandomState(1)
    cases, wants = [], []
    for i in range(64):
        hdr = [int(rs.randint(0, 1 << 16)) << (16 * (i % 4)) | int(rs.randint(0, 4)) for _ in range(4)]
        fe = [h & (int(rs.randint(0, 1 << 16)) << (16 * (i % 4)) | 3) for h in hdr]
        if i % 3 == 0:  # one edge outside the header's set, in word i % 4
            fe[i % 4] |= (~hdr[i % 4]) & (1 << 63 | 1 << 17)
        same = i % 5 != 0
        F = sum(bin(w).count("1") for w in fe)
        subset = all(f & ~h == 0 for f, h in zip(fe, hdr))
        keep = same and subset
        mf = F if i % 2 else F - 1
        cases.append((1, 9, hdr, 9 if same else 10, fe, mf))
        wants.append((F, int(keep), int(not keep and F <= mf)))
    assert rule(cases) == wants
    assert {w[1:] for w in wants} == {(1, 0), (0, 1), (0, 0)}
