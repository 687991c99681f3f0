"""Deep endgames in the search from a pool of tables that the slots share (dbaz_attach_tables_pool, Engine(endgame_tables=N):
k_pool_decide / k_pool_grant in front of k_slot_requests in csrc/solver.hip, the rule in csrc/table_pool.h, the release request at
game end in csrc/tree.hip).  A pool as large as the engine against the per-slot attach, byte for byte; a dry pool against the
deterministic rule of include/dbaz.h -- the lowest asking slots are served, the others search with their model's evaluator --, its
invariants during self-play, reproducibility, the refusals and match play.  Formula and uniform evaluators on small boards."""
import warnings

import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.endgame import DeepTables, Endgame

pytestmark = pytest.mark.gpu


# ---- the helpers of test_hip_slot_tables.py
def start_with_free(d, rs, n_edges, free):
    """a random legal move sequence that leaves `free` >= 1 free edges and the game unfinished"""
    while True:
        s, moves = O.new_state(d), []
        for _ in range(n_edges - free):
            valid = np.nonzero(O.valid_moves(d, s))[0]
            m = int(valid[rs.randint(len(valid))])
            O.play_(d, s, m)
            moves.append(m)
            if O.get_result(s) is not None:
                break
        if len(moves) == n_edges - free and O.get_result(s) is None:
            return moves


def n_edges(R, C):
    return 2 * R * C + R + C


def same_roots(ra, rb, slots=slice(None), what=""):
    for k in ra:
        assert np.array_equal(np.ascontiguousarray(ra[k][slots]).view(np.uint8), np.ascontiguousarray(rb[k][slots]).view(np.uint8)), (what, k)


def same_rows(ra, rb, what=""):
    assert set(ra) == set(rb)
    for k in ra:
        assert np.array_equal(np.ascontiguousarray(ra[k]).view(np.uint8), np.ascontiguousarray(rb[k]).view(np.uint8)), (what, k)


R4, M = 4, 18
_cache = {}


def starts_4x4():
    """64 starts with 3 <= F <= M and 64 with F > M on 4x4, built once"""
    if "starts" not in _cache:
        d, rs = O.dims(R4, R4), np.random.RandomState(41)
        below = [start_with_free(d, rs, n_edges(R4, R4), f) for f in [M] * 4 + [M - 1 - i % (M - 3) for i in range(60)]]
        above = [start_with_free(d, rs, n_edges(R4, R4), M + 1 + i % 6) for i in range(64)]
        _cache["starts"] = (below, above)
    return _cache["starts"]


def searched(starts, reads, **kw):
    """the roots after one search of `starts` on a fresh 64-slot formula engine; computed once per configuration"""
    from dotsboxesaz_amd.engine import Engine
    e = Engine(R4, R4, 64, mcts_num_read=50, evaluator="formula", **kw)
    e.set_positions(starts)
    e.search(reads)
    r = e.roots()
    assert e.counters()["error_slots"] == 0
    e.close()
    return r


# ---------------------------------------------------------------- 2. a pool of n_slots tables is the per-slot attach
@pytest.mark.parametrize("mode", ["lockstep", "stagger", "waves"])
def test_pool_of_n_slots_equals_the_per_slot_attach(mode):
    from dotsboxesaz_amd.engine import Engine
    tables = DeepTables(R4, R4, max_free=M)
    out = []
    for n_tables in (64, None):
        kw = dict(max_pending_evals=8, selfplay_pending=True) if mode == "waves" else {}
        e = Engine(R4, R4, 64, mcts_num_read=20, noise=(0.8, 0.25), temperature={0: 1.0}, evaluator="formula", endgame=tables, endgame_seed=2,
                   seed=5, endgame_tables=n_tables, **kw)
        if mode == "stagger":
            e.selfplay_stagger(1 + np.arange(64) % 20)
        e.selfplay_start(128, 0)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*dry.*")  # nothing is denied: run() has nothing to say about the pool
            e.run()
        c = e.counters()
        assert c["games_finished"] == 128 and c["error_slots"] == 0
        out.append((e.fetch_samples(), e.endgame_stats(), e.table_pool(), [e.slot_table(s)["table_index"] for s in range(64)]))
        e.close()
    tables.close()
    (ra, sa, pa, ia), (rb, sb, pb, ib) = out
    same_rows(ra, rb, mode)
    assert sa == sb and sa[0] >= 128
    print("pool of 64, %s: %s" % (mode, pa))
    assert pa["n_tables"] == 64 and pa["denied"] == 0
    assert pa["in_use"] == 0  # every game gave its region back when it ended
    assert 1 <= pa["high_water"] <= 64
    assert ia == [-1] * 64  # ... and no header names one any more
    assert pb == dict(n_tables=0, in_use=0, high_water=0, denied=0) and ib == list(range(64))  # per slot: region == slot


# ---------------------------------------------------------------- 3. a dry pool under manual search: the rule, exactly
def check_dry(e, starts, per_slot, plain, served, denied_before, what):
    """e: the engine with a pool of 16 after a search of `starts`; served: the 16 slots the rule gives a table"""
    others = np.setdiff1d(np.arange(64), served)
    r = e.roots()
    same_roots(r, per_slot, served, what + ": served slots against the per-slot attach")
    same_roots(r, plain, others, what + ": the other slots against a plain engine")
    p = e.table_pool()
    print("%s: %s" % (what, p))
    assert p["in_use"] == 16 and p["high_water"] == 16
    valid = [s for s in range(64) if e.slot_table(s)["valid"]]
    assert valid == list(served)
    held = [e.slot_table(int(s))["table_index"] for s in served]
    assert sorted(held) == list(range(16)) and all(e.slot_table(int(s))["table_index"] == -1 for s in others)
    return p["denied"] - denied_before


def test_dry_pool_serves_the_lowest_asking_slots():
    from dotsboxesaz_amd.engine import Engine
    below, above = starts_4x4()
    reads = 30
    tables = DeepTables(R4, R4, max_free=M)
    e = Engine(R4, R4, 64, mcts_num_read=50, evaluator="formula", endgame=tables, endgame_seed=1, endgame_tables=16)
    assert e.table_pool() == dict(n_tables=16, in_use=0, high_water=0, denied=0)
    e.set_positions(below)
    e.search(reads)
    per_slot, plain = searched(below, reads, endgame=tables, endgame_seed=1), searched(below, reads)
    assert check_dry(e, below, per_slot, plain, np.arange(16), 0, "64 asking slots") == 48
    assert e.endgame_stats()[0] == 16
    # a second search of the same positions: the 16 keep their tables, the 48 ask again and are denied again
    e.search(reads)
    assert e.table_pool()["denied"] == 96 and e.table_pool()["in_use"] == 16 and e.endgame_stats()[0] == 16
    # clear-all: every region is free again, and the reversed starts give the same relation
    rev = below[::-1]
    e.set_positions(rev)
    assert e.table_pool()["in_use"] == 0 and all(e.slot_table(s)["table_index"] == -1 for s in range(64))
    e.search(reads)
    per_slot, plain = searched(rev, reads, endgame=tables, endgame_seed=1), searched(rev, reads)
    assert check_dry(e, rev, per_slot, plain, np.arange(16), 96, "reversed") == 48
    # mixed: odd slots are above max_free and never ask; the pool serves even slots 0, 2, .., 30
    mixed = [below[i] if i % 2 == 0 else above[i] for i in range(64)]
    e.set_positions(mixed)
    e.search(reads)
    per_slot, plain = searched(mixed, reads, endgame=tables, endgame_seed=1), searched(mixed, reads)
    assert check_dry(e, mixed, per_slot, plain, np.arange(0, 32, 2), 144, "mixed") == 16
    with pytest.warns(UserWarning, match="dry"):
        e._warn_tables_denied()
    e.close()
    tables.close()


# ---------------------------------------------------------------- 4. a dry pool in self-play: invariants, reuse, reproducibility
def play_dry(tables, check):
    from dotsboxesaz_amd.engine import Engine
    R, C = 5, 5
    e = Engine(R, C, 64, mcts_num_read=24, noise=(0.0, 0.0), temperature={0: 1.0}, reuse_tree=False, evaluator="uniform", endgame=tables,
               endgame_seed=3, seed=11, endgame_tables=16)
    e.selfplay_start(128, 0)
    want = DeepTables(R, C, max_free=M, n_tables=1) if check else None
    pieces = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # run() says that searches were denied
        while e.counters()["active_slots"] > 0:
            e.run(max_steps=150)
            pieces += 1
            assert pieces < 400
            if not check:
                continue
            hdr = [e.slot_table(s) for s in range(64)]
            p = e.table_pool()
            held = [h["table_index"] for h in hdr if h["valid"]]
            assert len(set(held)) == len(held) and all(0 <= t < 16 for t in held)  # pairwise distinct regions of the pool
            assert len(held) == p["in_use"] <= 16
            assert all(h["table_index"] == -1 for h in hdr if not h["valid"])
            for h in [h for h in hdr if h["valid"]][:2]:  # the region holds the table of the header's root
                x = np.ones(3 * (R + 1) * (C + 1), np.int16)
                free = [a for a in range(2 * (R + 1) * (C + 1)) if int(h["free_edges"][a >> 6]) >> (a & 63) & 1]
                x[free] = 0
                assert len(free) == h["n_free"] <= M
                assert np.array_equal(h["table"], want.solve(x[None]).table(0)), h["game"]
                _cache["tables_checked"] = _cache.get("tables_checked", 0) + 1
    c = e.counters()
    out = (e.fetch_samples(), e.endgame_stats(), e.table_pool(), {k: c[k] for k in ("games_finished", "error_slots", "expansions", "moves_played")})
    e.close()
    if want is not None:
        want.close()
    return out


def test_dry_pool_in_selfplay_keeps_its_invariants_and_is_reproducible():
    tables = DeepTables(5, 5, max_free=M)
    rows, stats, p, c = play_dry(tables, True)
    print("dry pool in self-play: %s, tables solved %d, tables compared %d" % (p, stats[0], _cache.get("tables_checked", 0)))
    assert c["games_finished"] == 128 and c["error_slots"] == 0
    assert p["denied"] > 0 and p["high_water"] == 16 and p["in_use"] == 0
    assert stats[0] > 16  # more tables than regions: later games took the regions earlier games gave back
    assert _cache.get("tables_checked", 0) >= 4
    rows2, stats2, p2, c2 = play_dry(tables, False)
    tables.close()
    same_rows(rows, rows2, "second run")
    assert (stats, p, c) == (stats2, p2, c2)


# ---------------------------------------------------------------- 5. refusals
def test_refusals_change_nothing():
    from dotsboxesaz_amd.engine import Engine

    def code(fn):
        with pytest.raises(_lib.DbazError) as ei:
            fn()
        return ei.value.code

    below, _ = starts_4x4()
    starts = below[:8]
    tables = DeepTables(R4, R4, max_free=M)

    def roots(e):
        e.set_positions(starts)
        e.search(20)
        return e.roots()

    # nothing attached yet: every refused pooled attach leaves the handle without tables
    e = Engine(R4, R4, 8, mcts_num_read=50, evaluator="formula")
    before = roots(e)
    g = Endgame(R4, R4, max_free=16)
    for bad in (lambda: e.attach_endgame_pool(tables, 0), lambda: e.attach_endgame_pool(tables, -3), lambda: e.attach_endgame_pool(tables, 9),
                lambda: e.attach_endgame_pool(tables, 4, reads=3), lambda: e.attach_endgame_pool(g, 4),
                lambda: e.attach_endgame_pool(tables, 4, model=1)):
        assert code(bad) == _lib.EINVAL
    assert code(lambda: e.slot_table(0)) == _lib.EINVAL and e.table_pool()["n_tables"] == 0
    same_roots(before, roots(e), what="after refused attaches on a bare handle")
    assert code(lambda: Engine(R4, R4, 8, evaluator="formula", endgame=tables, endgame_tables=4, endgame_reads=2)) == _lib.EINVAL
    # a pooled handle: per-slot, another n_tables, another max_free, an Endgame and a read cap are refused and change nothing
    e.attach_endgame_pool(tables, 4, seed=2)
    pooled = roots(e)
    assert e.table_pool() == dict(n_tables=4, in_use=4, high_water=4, denied=4)
    other = DeepTables(R4, R4, max_free=M - 1)
    for bad in (lambda: e.attach_endgame(tables, 0, seed=2), lambda: e.attach_endgame_pool(tables, 5, seed=2), lambda: e.attach_endgame(g, 0),
                lambda: e.attach_endgame_pool(tables, 8), lambda: e.attach_endgame_pool(other, 4), lambda: e.attach_endgame_pool(tables, 4, reads=1)):
        assert code(bad) == _lib.EINVAL
    other.close()
    assert e.table_pool() == dict(n_tables=4, in_use=4, high_water=4, denied=4)  # not even the headers were dropped
    same_roots(pooled, roots(e), what="after refused attaches on a pooled handle")
    # a re-attach with the same figures frees every region; the handle it replaced may be destroyed
    again = DeepTables(R4, R4, max_free=M)
    e.attach_endgame_pool(again, 4, seed=2)
    assert e.table_pool()["in_use"] == 0
    third = DeepTables(R4, R4, max_free=M)
    e.attach_endgame_pool(third, 4, seed=2)
    again.close()
    same_roots(pooled, roots(e), what="after the replaced handle was destroyed")
    assert e.counters()["error_slots"] == 0
    e.close()
    third.close()
    # a per-slot handle refuses the pooled attach
    e2 = Engine(R4, R4, 8, mcts_num_read=50, evaluator="formula", endgame=tables, endgame_seed=2)
    per_slot = roots(e2)
    assert code(lambda: e2.attach_endgame_pool(tables, 8, seed=2)) == _lib.EINVAL and e2.table_pool()["n_tables"] == 0
    same_roots(per_slot, roots(e2), what="after a refused pooled attach on a per-slot handle")
    same_roots(per_slot, pooled, slice(0, 4), "the four served slots")
    e2.close()
    # an Endgame handle refuses it too
    e3 = Engine(R4, R4, 8, mcts_num_read=50, evaluator="formula", endgame=g)
    first = roots(e3)
    assert code(lambda: e3.attach_endgame_pool(tables, 8)) == _lib.EINVAL
    same_roots(first, roots(e3), what="after a refused pooled attach on an Endgame handle")
    e3.close()
    g.close()
    tables.close()


# ---------------------------------------------------------------- 6. match play: both seats draw on one pool
def test_match_play_with_a_pool_equals_the_per_slot_attach():
    from dotsboxesaz_amd.engine import Engine
    d, rs = O.dims(R4, R4), np.random.RandomState(4)
    book = [start_with_free(d, rs, 40, M - i % 6) for i in range(32)]
    tables = DeepTables(R4, R4, max_free=M)
    out = []
    for n_tables in (64, None):
        e = Engine(R4, R4, 64, mcts_num_read=24, temperature={0: 1.0}, reuse_tree=False, match_play=True, evaluator="uniform", evaluator2="formula",
                   endgame=tables, endgame_models=(0,), endgame_seed=5, seed=9, endgame_tables=n_tables)
        e.selfplay_set_start(book, 2)
        e.selfplay_start(64, 0)
        e.run()
        c = e.counters()
        assert c["games_finished"] == 64 and c["error_slots"] == 0
        out.append((e.fetch_samples(), e.endgame_stats(), e.table_pool()))
        e.close()
    tables.close()
    (ra, sa, pa), (rb, sb, pb) = out
    same_rows(ra, rb, "match")
    assert sa == sb and sa[0] >= 48
    assert pa["denied"] == 0 and pa["in_use"] == 0 and 1 <= pa["high_water"] <= 64
