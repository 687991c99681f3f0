"""The pool of tables that the slots of an engine share (csrc/table_pool.h, dbaz_attach_tables_pool): the grant rule and the free
stack, run on the host.  tests/table_pool_main.cpp and the header are compiled with g++ under AddressSanitizer and UBSan into a
stand-alone program (no device code, no GPU, nothing loaded into Python) and compared with a numpy restatement of the rule in
include/dbaz.h: every region given back in a pass is free before the grants, the asking slots are granted in ascending slot order
as long as free regions last, the others are denied and counted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

GXX = os.environ.get("CXX") or shutil.which("g++")


class PoolRef:
    """the rule restated: a LIFO of free regions, region 0 on top at the start"""

    def __init__(self, n_tables, n_slots):
        self.n_tables = n_tables
        self.stack = np.arange(n_tables - 1, -1, -1, dtype=np.int64)
        self.table = np.full(n_slots, -1, np.int64)
        self.high_water = 0
        self.denied = 0

    def release(self, slots):
        for s in slots:
            if self.table[s] >= 0:
                self.stack = np.append(self.stack, self.table[s])
                self.table[s] = -1

    def grant(self, flags):
        asking = np.nonzero(flags & (self.table < 0))[0]  # ascending slot order
        n = min(len(asking), len(self.stack))
        self.table[asking[:n]] = self.stack[::-1][:n]
        self.stack = self.stack[:len(self.stack) - n]
        self.denied += len(asking) - n
        self.high_water = max(self.high_water, self.n_tables - len(self.stack))
        return asking[:n], asking[n:]


@pytest.fixture(scope="module")
def pool(tmp_path_factory):
    assert GXX, "g++ builds csrc/buildinfo.cpp too: it is part of the toolchain"
    exe = tmp_path_factory.mktemp("table_pool") / "table_pool"
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "dotsboxesaz_amd", "csrc"), os.path.join(REPO, "tests", "table_pool_main.cpp"), "-o", str(exe)],
                   check=True)

    def run(commands):
        """commands: ("I", n_tables, n_slots) | ("R", slots) | ("G", flags) -> per G: (top, high_water, denied, table, stack)"""
        text = []
        for c in commands:
            if c[0] == "I":
                text.append("I %d %d" % (c[1], c[2]))
            elif c[0] == "R":
                text.append("R %d %s" % (len(c[1]), " ".join(str(int(s)) for s in c[1])))
            else:
                text.append("G " + "".join("1" if f else "0" for f in c[1]))
        r = subprocess.run([str(exe)], input="\n".join(text) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)  # a sanitizer report ends the program with a message
        lines = r.stdout.split("\n")
        out = []
        for i in range(sum(1 for c in commands if c[0] == "G")):
            top, high, denied = (int(t) for t in lines[3 * i].split())
            out.append((top, high, denied, np.array(lines[3 * i + 1].split(), np.int64), np.array(lines[3 * i + 2].split(), np.int64)))
        return out
    return run


def same(got, ref):
    top, high, denied, table, stack = got
    assert (top, high, denied) == (len(ref.stack), ref.high_water, ref.denied)
    assert np.array_equal(table, ref.table) and np.array_equal(stack, ref.stack)


# the group boundaries of k_pool_grant's ranking (TABLE_POOL_GROUP = 1024 slots per round), 8 192 slots and one count above
@pytest.mark.parametrize("n_slots", [1, 63, 1023, 1024, 1025, 2049, 8191, 8192, 8193, 9001])
def test_grants_in_slot_order_for_every_supply(pool, n_slots):
    rs = np.random.RandomState(n_slots)
    commands, refs = [], []
    for density in (0.0, 0.03, 0.5, 1.0):
        flags = rs.rand(n_slots) < density
        asked = int(flags.sum())
        for n_free in sorted({0, 1, asked // 2, max(asked - 1, 0), asked, asked + 1, n_slots}):  # none, fewer, equal, more
            if n_free > n_slots:
                continue
            ref = PoolRef(n_free, n_slots)
            granted, denied = ref.grant(flags)
            assert len(granted) == min(asked, n_free) and len(denied) == asked - len(granted)
            assert len(granted) == 0 or len(denied) == 0 or granted.max() < denied.min()  # the lowest slots are served
            commands += [("I", n_free, n_slots), ("G", flags)]
            refs.append(ref)
    got = pool(commands)
    assert len(got) == len(refs)
    for g, ref in zip(got, refs):
        same(g, ref)
        held = g[3][g[3] >= 0]
        assert len(set(held.tolist())) == len(held) and g[1] == len(held)  # distinct regions; the high-water mark of one pass


@pytest.mark.parametrize("n_slots,n_tables", [(64, 16), (1500, 400), (8200, 3000)])
def test_release_and_grant_passes_keep_the_stack_a_permutation_of_the_unheld_regions(pool, n_slots, n_tables):
    rs = np.random.RandomState(n_tables)
    ref = PoolRef(n_tables, n_slots)
    commands, states = [("I", n_tables, n_slots)], []
    for p in range(40):
        holders = np.nonzero(ref.table >= 0)[0]
        # some holders give their region back, and so do a few slots that hold none (nothing may happen); a dry spell in the middle
        give = rs.permutation(holders)[:rs.randint(0, len(holders) + 1) if p % 7 else 0]
        give = np.concatenate([give, rs.randint(0, n_slots, 3)])
        flags = rs.rand(n_slots) < (0.9 if 10 <= p < 14 else 0.15)
        ref.release(give)
        ref.grant(flags)
        commands += [("R", give), ("G", flags)]
        states.append((ref.stack.copy(), ref.table.copy(), ref.high_water, ref.denied))
    got = pool(commands)
    assert len(got) == len(states)
    for (top, high, denied, table, stack), (rstack, rtable, rhigh, rdenied) in zip(got, states):
        held = table[table >= 0]
        assert sorted(stack.tolist() + held.tolist()) == list(range(n_tables))  # every region is free or held, never both
        assert top == len(stack) == n_tables - len(held)
        assert np.array_equal(table, rtable) and np.array_equal(stack, rstack) and (high, denied) == (rhigh, rdenied)
    assert states[-1][3] > 0 and states[-1][2] == n_tables  # the pool ran dry on the way


def test_the_entry_points_are_bound_and_the_python_interface_takes_a_pool():
    import inspect
    import re
    from dotsboxesaz_amd import _lib, build, self_play
    from dotsboxesaz_amd import endgame as E
    from dotsboxesaz_amd.engine import Engine
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dbaz.h")).read(), flags=re.S)
    L = _lib.load()
    for name, count in dict(dbaz_attach_tables_pool=6, dbaz_get_table_pool=5, dbaz_get_slot_table_index=3).items():
        assert name in _lib.SYMBOLS and len(getattr(L, name).argtypes) == count
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == count, (name, decl)
    assert _lib.ABI_VERSION == 3  # symbols were added, nothing else changed
    assert "endgame_tables" in inspect.signature(Engine.__init__).parameters
    assert list(inspect.signature(Engine.attach_endgame_pool).parameters)[1:] == ["endgame", "tables", "model", "seed", "reads"]
    assert hasattr(Engine, "table_pool") and "table_index" in Engine.slot_table.__doc__
    for fn in (self_play.generate_games, self_play.compute_elo):
        assert "endgame_tables" in inspect.signature(fn).parameters
    assert "--pool" in inspect.getsource(E.main) and "high_water" in inspect.getsource(E._selfplay_bench)
    path = os.path.join(REPO, "dotsboxesaz_amd", "csrc", "table_pool.h")
    assert path in build.source_files() and "table_pool.h" not in build.NN_SOURCES
