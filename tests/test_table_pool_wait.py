"""The pool of tables in wait mode (csrc/table_pool.h, dbaz_attach_tables_pool_wait): the header's settle and grant steps with
standing requests, run on the host.  tests/table_pool_wait_main.cpp and the header are compiled with g++ under AddressSanitizer
and UBSan into a stand-alone program (no device code, no GPU, nothing loaded into Python) and compared with a short model of the
rule in include/dbaz.h: releases first, then the waiting slots and the new askers together take the free regions in ascending
slot order; whoever gets nothing keeps asking and is counted in `waited`, never in `denied`."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

GXX = os.environ.get("CXX") or shutil.which("g++")
PASSES = 200


class WaitRef:
    """the rule restated with plain Python containers: a LIFO of free regions (region 0 on top at the start), a set of requests"""

    def __init__(self, n_tables, n_slots):
        self.n_tables, self.n_slots = n_tables, n_slots
        self.free = list(range(n_tables - 1, -1, -1))  # the top is the end
        self.held = {}  # slot -> region
        self.asking = set()
        self.high_water = self.waited = self.waiting = 0

    def release(self, slots):
        for s in slots:
            if s in self.held:
                self.free.append(self.held.pop(s))

    def ask(self, slots):
        self.asking |= set(int(s) for s in slots)

    def grant(self):
        """-> (the askers of this pass, the granted of them), both ascending"""
        askers = sorted(s for s in self.asking if s not in self.held)
        granted = askers[:len(self.free)]
        for s in granted:
            self.held[s] = self.free.pop()
        self.asking = set(askers[len(granted):])
        self.waiting = len(askers) - len(granted)
        self.waited += self.waiting
        self.high_water = max(self.high_water, len(self.held))
        return askers, granted

    def table(self):
        t = np.full(self.n_slots, -1, np.int64)
        for s, r in self.held.items():
            t[s] = r
        return t


@pytest.fixture(scope="module")
def pool(tmp_path_factory):
    assert GXX, "g++ builds csrc/buildinfo.cpp too: it is part of the toolchain"
    exe = tmp_path_factory.mktemp("table_pool_wait") / "table_pool_wait"
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "dotsboxesaz_amd", "csrc"), os.path.join(REPO, "tests", "table_pool_wait_main.cpp"), "-o", str(exe)],
                   check=True)

    def run(commands):
        """("I", n_tables, n_slots) | ("R", slots) | ("A", slots, n_slots) | ("G",) -> per G: (top, high, denied, waited, waiting, table, stack)"""
        text = []
        for c in commands:
            if c[0] == "I":
                text.append("I %d %d" % (c[1], c[2]))
            elif c[0] == "R":
                text.append("R %d %s" % (len(c[1]), " ".join(str(int(s)) for s in c[1])))
            elif c[0] == "A":
                flags = np.zeros(c[2], bool)
                flags[np.asarray(c[1], np.int64)] = True
                text.append("A " + "".join("1" if f else "0" for f in flags))
            else:
                text.append("G")
        r = subprocess.run([str(exe)], input="\n".join(text) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)  # a sanitizer report ends the program with a message
        lines = r.stdout.split("\n")
        out = []
        for i in range(sum(1 for c in commands if c[0] == "G")):
            figures = tuple(int(t) for t in lines[3 * i].split())
            assert len(figures) == 5
            out.append(figures + (np.array(lines[3 * i + 1].split(), np.int64), np.array(lines[3 * i + 2].split(), np.int64)))
        return out
    return run


@pytest.mark.parametrize("n_tables", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n_slots", [7, 17, 40])
def test_waiting_slots_and_new_askers_are_served_in_slot_order_and_nothing_is_denied(pool, n_tables, n_slots):
    rs = np.random.RandomState(100 * n_tables + n_slots)
    ref = WaitRef(n_tables, n_slots)
    commands, expect = [("I", n_tables, n_slots)], []
    unserved_sum = 0
    for p in range(PASSES):
        holders = sorted(ref.held)
        # holders give back (none at all in a dry spell, so that the queue grows), and so do two slots that may hold nothing
        n_give = 0 if 60 <= p < 70 else rs.randint(0, len(holders) + 1)
        give = np.concatenate([rs.permutation(holders)[:n_give], rs.randint(0, n_slots, 2)]).astype(np.int64)
        # new askers: slots that neither hold nor wait (a waiting slot searches nothing, so it starts no new search either)
        idle = [s for s in range(n_slots) if s not in ref.held and s not in ref.asking]
        new = [s for s in idle if rs.rand() < (0.6 if p % 50 < 5 else 0.08)]
        ref.release(give)
        free_before = len(ref.free)
        ref.ask(new)
        askers, granted = ref.grant()
        # the properties of the rule, on the model itself
        assert len(granted) == min(free_before, len(askers))  # work-conserving: no region stays free while a slot asks
        assert granted == askers[:len(granted)]  # the lowest asking, waiting and new alike
        unserved_sum += len(askers) - len(granted)
        commands += [("R", give), ("A", new, n_slots), ("G",)]
        expect.append((len(ref.free), ref.high_water, 0, ref.waited, ref.waiting, ref.table(), np.array(ref.free, np.int64)))
    assert ref.waited == unserved_sum and ref.waited > 0 and ref.high_water == n_tables  # the pool ran dry, and slots waited
    got = pool(commands)
    assert len(got) == PASSES
    for g, x in zip(got, expect):
        assert g[:5] == x[:5], (g[:5], x[:5])  # top, high_water, denied == 0, waited, waiting
        assert np.array_equal(g[5], x[5]) and np.array_equal(g[6], x[6])
        held = g[5][g[5] >= 0]
        assert sorted(g[6].tolist() + held.tolist()) == list(range(n_tables))  # a region is held or on the stack, never both
        assert g[0] == len(g[6]) == n_tables - len(held)


def test_a_slot_waits_until_a_region_comes_back_and_a_lower_slot_that_asks_later_goes_first(pool):
    got = pool([("I", 1, 6), ("A", [2, 4], 6), ("G",), ("G",), ("A", [1], 6), ("G",), ("R", [2]), ("G",), ("R", [1]), ("G",), ("R", [4]), ("G",)])
    figures = [g[:5] for g in got]
    tables = [g[5].tolist() for g in got]
    # top, high_water, denied, waited, waiting
    assert figures == [(0, 1, 0, 1, 1), (0, 1, 0, 2, 1), (0, 1, 0, 4, 2), (0, 1, 0, 5, 1), (0, 1, 0, 5, 0), (1, 1, 0, 5, 0)]
    assert tables == [[-1, -1, 0, -1, -1, -1], [-1, -1, 0, -1, -1, -1], [-1, -1, 0, -1, -1, -1], [-1, 0, -1, -1, -1, -1],
                      [-1, -1, -1, -1, 0, -1], [-1, -1, -1, -1, -1, -1]]


def test_the_entry_points_are_bound_and_the_python_interface_takes_the_wait_mode():
    import inspect
    import re
    from dotsboxesaz_amd import _lib, self_play
    from dotsboxesaz_amd import endgame as E
    from dotsboxesaz_amd.engine import Engine
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dbaz.h")).read(), flags=re.S)
    L = _lib.load()
    for name, count in dict(dbaz_attach_tables_pool_wait=6, dbaz_get_table_pool_waits=4).items():
        assert name in _lib.SYMBOLS and len(getattr(L, name).argtypes) == count
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == count, (name, decl)
    assert _lib.ABI_VERSION == 3  # symbols were added, nothing else changed
    assert "endgame_wait" in inspect.signature(Engine.__init__).parameters
    assert list(inspect.signature(Engine.attach_endgame_pool_wait).parameters)[1:] == ["endgame", "tables", "model", "seed", "reads"]
    assert hasattr(Engine, "table_pool_waits")
    for fn in (self_play.generate_games, self_play.compute_elo):
        assert "endgame_wait" in inspect.signature(fn).parameters
    assert "--wait" in inspect.getsource(E.main) and "peak_waiting" in inspect.getsource(E._selfplay_bench)
