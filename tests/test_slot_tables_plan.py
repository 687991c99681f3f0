"""The launch plan of the deep slot tables inside the search (csrc/slot_tables_plan.h, the host side of dbaz_attach_tables,
DESIGN.md 4.7): compiled with g++ next to csrc/deep_batch.h into a stand-alone program under AddressSanitizer and UBSan.  For every
max_free M = 0 .. 31 and every F <= M the (L, plain, layer sequence) the slot plan gives F equals the launches deep_batch_plan
gives ONE root of that F with low_bits = 0; S is the maximum over F, the LDS size is 2^max L (runs without a GPU)."""
import os
import shutil
import subprocess
from math import comb

import pytest

from conftest import REPO


def default_low_bits(E):
    return min(14, max(E // 2, min(E, 8)))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    assert shutil.which("g++"), "g++ builds the library's build-identity unit too: it is part of the toolchain"
    exe = tmp_path_factory.mktemp("slot_tables_plan") / "slot_tables_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "dotsboxesaz_amd", "csrc"), os.path.join(REPO, "tests", "slot_tables_plan_main.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr  # a sanitizer report ends the program with a message
    out, lines = {}, iter(r.stdout.strip().split("\n"))
    for line in lines:
        v = [int(t) for t in line.split()]
        M, rc, S, max_low, lds = v[:5]
        plan = dict(rc=rc, S=S, max_low=max_low, lds=lds, widest=v[5:], slot={}, deep={})
        assert len(plan["widest"]) == S
        if rc == 0:
            for F in range(M + 1):
                t = next(lines).split()
                assert t[0] == "slot" and int(t[1]) == F
                w = [int(x) for x in t[2:]]
                plan["slot"][F] = dict(L=w[0], plain=w[1], top=w[2], layers=list(zip(w[3::2], w[4::2])))
                t = next(lines).split()
                assert t[0] == "deep" and int(t[1]) == F
                w = [int(x) for x in t[2:]]
                plan["deep"][F] = dict(L=w[0], plain=w[1], launches=list(zip(w[3::3], w[4::3], w[5::3])))
                assert len(plan["deep"][F]["launches"]) == w[2]
        out[M] = plan
    return out


def test_every_depth_walks_the_launches_of_a_single_root(plans):
    for M in range(32):
        p = plans[M]
        assert p["rc"] == 0 and sorted(p["slot"]) == list(range(M + 1))
        for F in range(M + 1):
            s, d = p["slot"][F], p["deep"][F]
            assert (s["L"], s["plain"]) == (d["L"], d["plain"]), (M, F)
            live = [(k, w) for k, w in s["layers"] if k >= 0]
            assert live == [(k, gx) for k, gx, gy in d["launches"]] and all(gy == 1 for _, _, gy in d["launches"]), (M, F)
            # a finished root has nothing left in any later launch, and the live launches come first
            assert s["layers"][len(live):] == [(s["top"] - i, 0) for i in range(len(live), p["S"])] and len(s["layers"]) == p["S"]
            assert s["top"] == live[0][0] and [k for k, _ in live] == list(range(s["top"], -1, -1))
            # the restatement of deep_batch.h's rules
            plain = F < 4
            L = 0 if plain else default_low_bits(F)
            assert (s["L"], s["plain"], s["top"]) == (L, int(plain), F - L)
            assert [w for _, w in live] == ([1] * (F + 1) if plain else [comb(F - L, k) for k in range(F - L, -1, -1)])


def test_launch_count_lds_and_widest_layers(plans):
    for M in range(32):
        p = plans[M]
        tops = [p["slot"][F]["top"] for F in range(M + 1)]
        assert p["S"] == max(tops) + 1
        assert p["max_low"] == max(p["slot"][F]["L"] for F in range(M + 1)) and p["lds"] == 1 << p["max_low"]
        assert p["widest"] == [max(p["slot"][F]["layers"][s][1] for F in range(M + 1)) for s in range(p["S"])]
        assert all(w >= 1 for w in p["widest"])
    assert (plans[20]["S"], plans[24]["S"], plans[16]["S"], plans[3]["S"], plans[0]["S"]) == (11, 13, 9, 4, 1)
    assert (plans[20]["lds"], plans[24]["lds"], plans[31]["lds"], plans[3]["lds"]) == (1 << 10, 1 << 12, 1 << 14, 1)
    assert plans[20]["widest"][5] == comb(10, 5) and plans[31]["S"] == 18
    # a shallow plain root needs more launches than a root of 4 .. 10 free edges: S is a maximum, not the deepest root's count
    assert plans[8]["S"] == 4 and plans[8]["slot"][8]["top"] == 0


def test_refusals(plans):
    for M in (-1, 32):
        assert plans[M]["rc"] == -1 and plans[M]["S"] == 0 and plans[M]["widest"] == []
