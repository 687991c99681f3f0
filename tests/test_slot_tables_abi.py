"""Deep tables inside the search (include/dbaz.h dbaz_attach_tables / dbaz_get_slot_table, Engine.attach_endgame / slot_table): the
binding, the header's declarations and the Python interface (runs without a GPU)."""
import inspect
import os
import re

from conftest import REPO
from dotsboxesaz_amd import _lib, build
from dotsboxesaz_amd import endgame as E
from dotsboxesaz_amd import self_play
from dotsboxesaz_amd.engine import Engine

ARGS = dict(dbaz_attach_tables=5, dbaz_get_slot_table=9)


def header():
    src = open(os.path.join(REPO, "include", "dbaz.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_the_two_symbols_are_bound_with_the_documented_arguments():
    L, src = _lib.load(), header()
    for n, count in ARGS.items():
        assert n in _lib.SYMBOLS and hasattr(L, n)
        assert len(getattr(L, n).argtypes) == count, n
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, src, flags=re.S).group(1)
        assert len(decl.split(",")) == count, (n, decl)
        assert getattr(L, n).restype is not None
    assert re.search(r"\bint\s+dbaz_attach_tables\s*\(\s*dbaz_engine\s*\*\s*e\s*,\s*int32_t\s+model\s*,\s*dbaz_tables\s*\*", src)
    assert re.search(r"uint64_t\s+free_edges\s*\[\s*4\s*\]", src)
    # dbaz_attach_endgame's argument types, so that Engine.attach_endgame can call either
    assert [t for t in L.dbaz_attach_tables.argtypes] == [t for t in L.dbaz_attach_endgame.argtypes]
    assert _lib.ABI_VERSION == 3  # symbols were added, nothing else changed


def test_the_pinned_families_keep_their_members():
    count = lambda prefix: len([s for s in _lib.SYMBOLS if s.startswith(prefix)])  # noqa: E731
    assert (count("dbaz_endgame_"), count("dbaz_deep_"), count("dbaz_tables_"), count("dbaz_solver_")) == (4, 8, 9, 7)


def test_python_interface_is_the_documented_one():
    assert list(inspect.signature(Engine.attach_endgame).parameters)[1:] == ["endgame", "model", "seed", "reads"]
    assert list(inspect.signature(Engine.slot_table).parameters)[1:] == ["slot"]
    assert "DeepTables" in Engine.attach_endgame.__doc__ and "dbaz_attach_tables" in Engine.attach_endgame.__doc__
    # the entry is named by the handle's class, so a handle made by `python -m dotsboxesaz_amd.endgame` (whose classes live in
    # __main__, not in the imported module) is still routed to its own entry
    assert (E.Endgame.ATTACH, E.DeepTables.ATTACH) == ("dbaz_attach_endgame", "dbaz_attach_tables")
    assert "ATTACH" in inspect.getsource(Engine.attach_endgame) and "isinstance" not in inspect.getsource(Engine.attach_endgame)
    for fn in (self_play.generate_games, self_play.compute_elo):
        assert "endgame" in inspect.signature(fn).parameters and "DeepTables" in fn.__doc__
    assert "DeepTables" in inspect.getsource(E._selfplay_bench)
    for key in ("endgame16", "deep", "table_bytes"):
        assert key in inspect.getsource(E._selfplay_bench), key


def test_the_plan_header_is_part_of_the_build_identity_and_host_only():
    csrc = os.path.join(REPO, "dotsboxesaz_amd", "csrc")
    path = os.path.join(csrc, "slot_tables_plan.h")
    assert path in build.source_files() and "slot_tables_plan.h" not in build.NN_SOURCES
    text = open(path).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()  # no HIP types: g++ compiles it
    for f in build.NN_SOURCES:
        assert "dbaz_attach_tables" not in open(os.path.join(csrc, f)).read(), f
