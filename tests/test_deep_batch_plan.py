"""The launch plan of a batch of deep endgame solves (csrc/deep_batch.h, the host side of dbaz_tables_solve):
compiled with g++ into a stand-alone program under AddressSanitizer and UBSan, and compared with the grouping, the slots and the
launch list restated here (runs without a GPU)."""
import os
import shutil
import subprocess
from math import comb

import pytest

from conftest import REPO

MIN_LOW, MAX_LOW, MAX_HIGH = 4, 16, 20
DEPTHS = [0, 1, 3, 4, 5, 12, 16, 17, 20, 31]


def default_low_bits(E):
    """the values dbaz_solver_solve and dbaz_deep_solve have used since they were written"""
    return min(14, max(E // 2, min(E, 8)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "g++ builds the library's build-identity unit too: it is part of the toolchain"
    exe = tmp_path_factory.mktemp("deep_batch") / "deep_batch"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "dotsboxesaz_amd", "csrc"), os.path.join(REPO, "tests", "deep_batch_main.cpp"), "-o", str(exe)],
                   check=True)
    return str(exe)


def run(program, cases):
    """cases: [(F list, max_free, n_tables, low_bits)] -> (default_low_bits of 0 .. 31, [dict per case])"""
    text = "%d\n" % len(cases) + "".join("%d %d %d %d\n%s\n" % (len(F), mf, nt, lb, " ".join(map(str, F))) for F, mf, nt, lb in cases)
    r = subprocess.run([program], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # a sanitizer report ends the program with a message
    lines = r.stdout.split("\n")
    defaults = [int(v) for v in lines[0].split()]
    out = []
    for i in range(len(cases)):
        v = [int(t) for t in lines[1 + 2 * i].split()]
        rc, bad, ng, nl = v[:4]
        n = (len(v) - 4 - 5 * ng - 4 * nl) // 2
        order, slots = v[4:4 + n], v[4 + n:4 + 2 * n]
        at = 4 + 2 * n
        groups = [dict(zip(("F", "L", "plain", "first", "count"), v[at + 5 * g:at + 5 * g + 5])) for g in range(ng)]
        at += 5 * ng
        launches = [tuple(v[at + 4 * k:at + 4 * k + 4]) for k in range(nl)]
        out.append(dict(rc=rc, bad_root=bad, order=order, slots=slots, groups=groups, launches=launches, error=lines[2 + 2 * i]))
    assert len(defaults) == 32
    return defaults, out


def expected(F, max_free, low_bits):
    """(order, groups, launches) from the issue's words: equal F together, deepest group first, root index within a group"""
    order = sorted(range(len(F)), key=lambda i: (-F[i], i))
    groups, launches = [], []
    for f in sorted(set(F), reverse=True):
        members = [i for i in order if F[i] == f]
        plain = f < MIN_LOW or low_bits == -1
        L = 0 if plain else (default_low_bits(f) if low_bits == 0 else low_bits)
        g = len(groups)
        groups.append(dict(F=f, L=L, plain=int(plain), first=order.index(members[0]), count=len(members)))
        if plain:
            launches += [(g, k, ((1 << f) + 255) // 256, len(members)) for k in range(f, -1, -1)]
        else:
            launches += [(g, k, comb(f - L, k), len(members)) for k in range(f - L, -1, -1)]
    return order, groups, launches


def check(got, F, max_free, low_bits):
    order, groups, launches = expected(F, max_free, low_bits)
    assert got["rc"] == 0 and got["bad_root"] == -1 and got["error"] == ""
    assert got["order"] == order and got["groups"] == groups and got["launches"] == launches
    assert got["slots"] == [i << max_free for i in range(len(F))]  # root i owns slot i, whatever group it is in
    for g in got["groups"]:
        if not g["plain"]:  # what one solve launches covers every high pattern once
            assert sum(l[2] for l in got["launches"] if got["groups"][l[0]] is g) == 1 << (g["F"] - g["L"])


def test_default_low_bits_keeps_its_values(program):
    defaults, _ = run(program, [])
    assert defaults == [default_low_bits(E) for E in range(32)]
    assert defaults == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 14, 14]


def test_groups_slots_and_launches(program):
    lists = [DEPTHS,                                     # every depth once
             [20, 20, 17, 16, 12, 5, 4, 3, 1, 0],        # the GPU test's batch
             [5, 20, 3, 20, 12, 5, 0, 31, 20, 12, 3],    # repeats, out of order
             [12],                                       # a single root
             [20] * 7, [3] * 5, [0, 0],                  # all F equal: one group
             [31, 31, 4]]
    cases = [(F, 31, 64, 0) for F in lists]
    cases += [(F, 31, len(F), -1) for F in lists]                      # the plain kernel everywhere; a pool that is exactly full
    cases += [([12, 12, 3, 1, 0, 12], 12, 8, lb) for lb in range(4, 13)]  # every explicit split of F = 12; F < 4 stays plain
    cases += [([31, 20], 31, 2, 16), ([24, 20, 16], 24, 64, 16), ([21, 5, 2], 24, 64, 5)]
    _, got = run(program, cases)
    for g, (F, mf, nt, lb) in zip(got, cases):
        check(g, F, mf, lb)
    first = got[0]
    assert [g["F"] for g in first["groups"]] == sorted(DEPTHS, reverse=True) and first["order"] == list(range(9, -1, -1))
    assert [(g["plain"], g["L"]) for g in first["groups"]] == [(0, 14), (0, 10), (0, 8), (0, 8), (0, 8), (0, 5), (0, 4), (1, 0), (1, 0), (1, 0)]
    # F = 20, L = 10: the launches of one group are C(10, k) wide and as many high as the group has roots
    batch = got[1]
    assert [l[2:] for l in batch["launches"] if l[0] == 0] == [(comb(10, k), 2) for k in range(10, -1, -1)]
    assert batch["order"] == list(range(10)) and len(batch["launches"]) == 11 + 10 + 9 + 5 + 1 + 1 + 4 + 2 + 1
    # a plain group: F + 1 launches over all 2^F masks
    assert [l for l in got[5]["launches"]] == [(0, k, 1, 5) for k in (3, 2, 1, 0)]
    assert [l[2] for l in got[8 + 3]["launches"]] == [16] * 13  # [12] with the plain kernel: 2^12 / 256 workgroups per layer


def test_refusals(program):
    cases = [([12, 21, 5], 20, 8, 0),        # 0: root 1 is too deep for the pool's tables
             ([5, 12, 32], 31, 8, 0),        # 1: past 31 (position_geometry counts on)
             ([12] * 5, 20, 4, 0),           # 2: more roots than tables
             ([12, 5, 12], 20, 8, 8),        # 3: low_bits 8 > F = 5
             ([12, 20], 20, 8, 3),           # 4: below SOLVER_MIN_LOW
             ([12, 17], 20, 8, 17),          # 5: above SOLVER_MAX_LOW
             ([12, 31], 31, 8, 10),          # 6: 31 - 10 high bits: more than SOLVER_MAX_HIGH
             ([3, 12], 20, 8, -2),           # 7: no such form; the F = 3 root is plain whatever low_bits says
             ([], 20, 8, 0),                 # 8: no root
             ([12], 20, 0, 0), ([12], 32, 4, 0), ([-1, 4], 20, 8, 0)]
    _, got = run(program, cases)
    assert all(g["rc"] == -1 and g["error"] and not g["order"] and not g["groups"] and not g["launches"] for g in got)
    assert [g["bad_root"] for g in got] == [1, 2, -1, 1, 0, 0, 1, 1, -1, -1, -1, 0]
    for i, words in ((0, ("root 1", "21")), (1, ("root 2", "32")), (2, ("5 roots", "4 tables")), (3, ("root 1", "low_bits 8")),
                     (6, ("root 1", "low_bits 10", "31")), (7, ("root 1", "low_bits -2"))):
        assert all(w in got[i]["error"] for w in words), got[i]["error"]
    # the same lists are fine where the reason is gone
    _, ok = run(program, [([12, 21, 5], 21, 8, 0), ([12] * 5, 20, 5, 0), ([12, 3, 12], 20, 8, 8), ([12, 30], 31, 8, 10), ([3, 2], 20, 8, -2)])
    assert all(g["rc"] == 0 for g in ok)
