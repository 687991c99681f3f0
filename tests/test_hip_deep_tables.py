"""Deep endgames in batches on the GPU (dbaz_tables_* in csrc/solver.hip, DeepTables / score_game_tails(tables=) /
game_tail_targets in dotsboxesaz_amd/endgame.py): every table of a batch against the single-table handle and both against the
numpy recurrence byte for byte, every work split against the numpy recurrence, rows of many games in one launch against DeepEndgame.score bit for bit, the served rule
by table index, the targets against Endgame.targets (F <= 16) and targets_ref.py (F = 17 .. 20), and the two game-level
functions against the game-by-game path.  Pools of at most 16 tables of 1 MiB."""
import numpy as np
import pytest

from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.endgame import DeepEndgame, DeepTables, Endgame, game_tail_targets, score_game_tails
from dotsboxesaz_amd.solver import ILLEGAL
import endgame_ref as ER
import targets_ref as TR
from test_hip_deep_endgame import BOARDS, ROOT_FREE, check_unsolved, random_pi, ref_table, root_of, tail

pytestmark = pytest.mark.gpu

DEPTHS = [20, 20, 17, 16, 12, 5, 4, 3, 1, 0]
KEYS = ("value", "diff", "q", "policy_mass", "n_free", "solved")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def free_of(R, C, x):
    return (np.asarray(x).reshape(-1, 3 * (R + 1) * (C + 1))[:, ER.board(R, C)[0]] == 0).sum(axis=1)


# ---------------------------------------------------------------- 1. every table of a batch, byte for byte
@pytest.mark.parametrize("R,C", BOARDS)
def test_tables_equal_the_single_table_handle(R, C):
    roots = np.stack([root_of(R, C, i % 4, f) for i, f in enumerate(DEPTHS)])  # the two F = 20 roots: games 0 and 1
    assert not np.array_equal(roots[0], roots[1])
    d = DeepEndgame(R, C, max_free=ROOT_FREE)
    want = [(d.solve(r).table(), d.n_free, d.d0) for r in roots]
    assert [w[1] for w in want] == DEPTHS
    for i, f in enumerate(DEPTHS):  # both handle kinds run the same code: every table against the numpy recurrence
        assert np.array_equal(want[i][0], ref_table(R, C, roots[i])), f
    t = DeepTables(R, C, max_free=ROOT_FREE, n_tables=len(DEPTHS))
    assert t.pool_bytes == len(DEPTHS) << 20 and t.n_solved == 0
    for order in (np.arange(len(DEPTHS)), np.random.RandomState(R + C).permutation(len(DEPTHS))):
        assert t.solve(roots[order]) is t and t.n_solved == len(DEPTHS) and t.solve_ms > 0
        assert t.n_free.tolist() == [DEPTHS[j] for j in order] and t.d0.tolist() == [want[j][2] for j in order]
        for i, j in enumerate(order):  # root i of this solve owns table i, whatever group it was solved in
            got = t.table(i)
            assert got.dtype == np.int8 and got.shape == (1 << DEPTHS[j],) and np.array_equal(got, want[j][0]), (i, j)
        deep = list(order).index(1)  # a slice of the second F = 20 table, wherever it stands
        assert np.array_equal(t.table(deep, 12345, 1000), want[1][0][12345:13345]) and t.table(deep, 1 << 20, 0).shape == (0,)
    with pytest.raises(_lib.DbazError) as ei:
        t.table(len(DEPTHS))
    assert ei.value.code == _lib.EINVAL
    d.close()
    t.close()


# ---------------------------------------------------------------- 2. the work split cannot matter
def test_every_work_split_writes_the_same_tables():
    R, C = 6, 6
    roots = np.stack([root_of(R, C, g, 12) for g in range(3)] + [root_of(R, C, 3, 2)])
    want = [ref_table(R, C, r) for r in roots]
    assert want[0].shape == (4096,) and not np.array_equal(want[0], want[1])
    t = DeepTables(R, C, max_free=12, n_tables=4)
    for low_bits in list(range(4, 13)) + [-1, 0]:
        t.solve(roots, low_bits)  # the F = 2 root takes the plain kernel whatever low_bits says
        for i in range(4):
            assert np.array_equal(t.table(i), want[i]), (low_bits, i)
        assert t.d0.tolist() == [int(w[0]) for w in want]
    # an explicit split that one root of a mixed batch cannot take: refused, naming it, and nothing is left solved
    mixed = np.stack([root_of(R, C, 0, 12), root_of(R, C, 1, 5), root_of(R, C, 2, 12)])
    with pytest.raises(_lib.DbazError) as ei:
        t.solve(mixed, 8)
    assert ei.value.code == _lib.EINVAL and "root 1" in str(ei.value) and t.n_solved == 0 and len(t.n_free) == 0
    with pytest.raises(_lib.DbazError) as ei:
        t.score(mixed, np.zeros(3, np.int32))
    assert ei.value.code == _lib.ESTATE
    with pytest.raises(_lib.DbazError) as ei:
        t.table(0)
    assert ei.value.code == _lib.ESTATE
    for bad, word in ((np.stack([mixed[0], root_of(R, C, 0, 13)]), "root 1"), (np.concatenate([roots, roots[:1]]), "5 roots")):
        with pytest.raises(_lib.DbazError) as ei:
            t.solve(bad)
        assert ei.value.code == _lib.EINVAL and word in str(ei.value) and t.n_solved == 0
    assert np.array_equal(t.solve(mixed).table(1), ref_table(R, C, mixed[1])) and t.n_solved == 3  # the handle stays usable
    t.close()


# ---------------------------------------------------------------- 3. rows of many games in one launch, bit for bit
def interleaved(R, C, lo, hi):
    """the rows of the board's four games with lo <= F <= hi, both movers, game g's rows at positions g, g + 4, ...: (x, game)"""
    per = [tail(R, C, g, lo, hi) for g in range(4)]
    n = len(per[0])
    assert all(len(p) == n for p in per)
    x = np.stack(per, axis=1).reshape(4 * n, -1)
    return x, np.tile(np.arange(4, dtype=np.int32), n)


@pytest.mark.parametrize("R,C", BOARDS)
def test_score_equals_the_single_table_handle_bit_for_bit(R, C):
    A = 2 * (R + 1) * (C + 1)
    x, game = interleaved(R, C, 0, ROOT_FREE)
    assert len(x) == 4 * 42 and not np.array_equal(x[0], x[1])
    pi = random_pi(len(x), A, seed=R + 3 * C)
    t = DeepTables(R, C, max_free=ROOT_FREE, n_tables=4).solve(np.stack([root_of(R, C, g) for g in range(4)]))
    got = t.score(x, game, pi)
    assert got["solved"].all() and got["policy_mass"].dtype == np.float32
    d = DeepEndgame(R, C, max_free=ROOT_FREE)
    movers = set()
    for g in range(4):
        want = d.solve(root_of(R, C, g)).score(x[game == g], pi[game == g])
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k][game == g], want[k]), (g, k)
        assert np.array_equal(bits(got["policy_mass"][game == g]), bits(want["policy_mass"]))
        movers |= set(want["value"].tolist())
    assert movers == {-1, 0, 1} or (R, C) == (6, 6)
    none = t.score(x, game)
    assert none["policy_mass"] is None and np.array_equal(none["q"], got["q"]) and np.array_equal(none["value"], got["value"])
    d.close()
    t.close()


# ---------------------------------------------------------------- 4. the served rule
def test_served_rule_by_table_index():
    R, C = 4, 4
    A = 2 * (R + 1) * (C + 1)
    t = DeepTables(R, C, max_free=ROOT_FREE, n_tables=8)
    x, game = interleaved(R, C, 0, 16)
    pi = random_pi(len(x), A, seed=9)
    with pytest.raises(_lib.DbazError) as ei:
        t.score(x, game)
    assert ei.value.code == _lib.ESTATE
    with pytest.raises(_lib.DbazError) as ei:
        t.targets(x, game, pi, np.zeros(len(x), np.float32))
    assert ei.value.code == _lib.ESTATE
    t.solve(np.stack([root_of(R, C, g) for g in range(4)]))
    own = free_of(R, C, x)
    want = t.score(x, game, pi)
    assert want["solved"].all() and np.array_equal(want["n_free"], own)
    # -1, another game's table, and indices the pool has but the solve did not fill (4 .. 7)
    acts = ER.board(R, C)[0]
    root_drawn = np.stack([root_of(R, C, g)[acts] != 0 for g in range(4)])

    def fits(tables):  # the served rule restated: no edge free that the table's root has drawn
        return ~((x[:, acts] == 0) & root_drawn[tables]).any(axis=1)
    table_of = game.copy()
    table_of[0::5] = -1
    table_of[1::5] = (game[1::5] + 1) % 4
    table_of[2::5] = 4 + game[2::5]
    got = t.score(x, table_of, pi)
    off = np.zeros(len(x), bool)
    off[0::5] = off[2::5] = True
    foreign = np.zeros(len(x), bool)
    foreign[1::5] = True
    assert not got["solved"][off].any()
    check_unsolved(got, np.nonzero(off)[0])
    unserved_foreign = foreign & ~got["solved"]
    assert np.array_equal(got["solved"][foreign], fits(table_of % 4)[foreign]) and unserved_foreign.sum() >= 20  # all but the nearly full boards
    check_unsolved(got, np.nonzero(unserved_foreign)[0])
    assert np.array_equal(got["n_free"], own)  # the row's own count in every case
    same = ~off & ~foreign
    for k in KEYS:
        assert np.array_equal(got[k][same], want[k][same]), k
    # a second solve of fewer roots: tables 2 and 3 are no longer served, 0 and 1 hold other games now
    t.solve(np.stack([root_of(R, C, 3), root_of(R, C, 2)]))
    assert t.n_solved == 2
    again = t.score(x, game, pi)
    assert not again["solved"][game >= 2].any() and np.array_equal(again["n_free"], own)
    check_unsolved(again, np.nonzero(game >= 2)[0])
    swapped = t.score(x, 3 - game, pi)  # games 3 and 2 at tables 0 and 1
    for k in KEYS:
        assert np.array_equal(swapped[k][game >= 2], want[k][game >= 2]), k
    assert not swapped["solved"][game < 2].any()
    t.close()


# ---------------------------------------------------------------- 5. training targets from the tables
MODES = [(p, z) for p in ("restrict", "uniform", "keep") for z in (True, False)]


@pytest.mark.parametrize("R,C", BOARDS)
def test_targets_equal_endgame_targets_bit_for_bit(R, C):
    A = 2 * (R + 1) * (C + 1)
    x, game = interleaved(R, C, 0, 16)
    n = len(x)
    rs = np.random.RandomState(7 * R + C)
    pi = random_pi(n, A, seed=R + C)
    z = rs.randint(-1, 2, n).astype(np.float32)
    g = Endgame(R, C)
    t = DeepTables(R, C, max_free=ROOT_FREE, n_tables=4).solve(np.stack([root_of(R, C, k) for k in range(4)]))
    sc = t.score(x, game, pi)
    members = (sc["q"] != ILLEGAL) & (np.sign(np.array([TR.margin_of(R, C, r) for r in x])[:, None] + sc["q"].astype(np.int64)) == sc["value"][:, None])
    unfinished = (sc["q"] != ILLEGAL).any(axis=1)
    assert 8 <= (~unfinished).sum() < n // 2 and members[unfinished].any(axis=1).all()
    empty = np.nonzero(unfinished)[0][::7]  # rows whose pi has no mass on O: the uniform branch of "restrict"
    pi[empty] = np.where(members[empty], 0.0, pi[empty]).astype(np.float32)
    # rows that no table serves: index -1, and another game's table
    table_of = game.copy()
    off = np.zeros(n, bool)
    off[3::5] = True
    table_of[off] = np.where(np.arange(n)[off] % 2 == 0, -1, (game[off] + 2) % 4)
    unserved = off & ~t.score(x, table_of)["solved"]
    assert unserved.sum() >= 10 and (table_of[unserved] == -1).any() and (table_of[unserved] >= 0).any()
    pi0, z0 = pi.copy(), z.copy()
    for pi_mode, z_mode in MODES:
        want_pi, want_z, want = g.targets(x, pi, z, pi_mode, z_mode)
        got_pi, got_z, got = t.targets(x, game, pi, z, pi_mode, z_mode)
        assert got_pi.dtype == np.float32 and got_z.dtype == np.float32 and got_z.shape == z.shape
        assert np.array_equal(bits(got_pi), bits(want_pi)) and np.array_equal(bits(got_z), bits(want_z)), (pi_mode, z_mode)
        for k in ("n_free", "mass", "relabelled"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (pi_mode, z_mode, k)
        assert np.array_equal(got["relabelled"], unfinished) and (got["mass"][empty] == 0).all()
        if pi_mode == "restrict":  # no mass on O: equal shares there
            assert np.array_equal(got_pi[empty], (members[empty] / members[empty].sum(axis=1, keepdims=True)).astype(np.float32))
        # the same call with some rows pointed away from their tables: those come back bit for bit, the others as before
        part_pi, part_z, part = t.targets(x, table_of, pi, z.reshape(n, 1), pi_mode, z_mode)
        assert part_z.shape == (n, 1)
        assert np.array_equal(bits(part_pi[unserved]), bits(pi0[unserved])) and np.array_equal(bits(part_z[unserved, 0]), bits(z0[unserved]))
        assert not part["relabelled"][unserved].any() and (part["mass"][unserved] == 0).all() and np.array_equal(part["n_free"], want["n_free"])
        assert np.array_equal(bits(part_pi[~unserved]), bits(want_pi[~unserved])) and np.array_equal(bits(part_z[~unserved, 0]), bits(want_z[~unserved]))
        assert np.array_equal(bits(pi), bits(pi0)) and np.array_equal(bits(z), bits(z0))  # the caller's arrays are never modified
    # finished games come back bit for bit
    fin_pi, fin_z, _ = t.targets(x, game, pi, z, "uniform", True)
    assert np.array_equal(bits(fin_pi[~unfinished]), bits(pi0[~unfinished])) and np.array_equal(bits(fin_z[~unfinished]), bits(z0[~unfinished]))
    g.close()
    t.close()


@pytest.mark.parametrize("R,C", BOARDS)
def test_targets_beyond_16_equal_the_reference(R, C):
    """F = 17 .. 20: the numpy rule of targets_ref.py on facts taken from the single-table scorer, which the existing tests pin
    against endgame_ref.py: v = value, O = the free a with sign(margin + q[a]) == v"""
    A = 2 * (R + 1) * (C + 1)
    acts, _ = ER.board(R, C)
    x, game = interleaved(R, C, 17, ROOT_FREE)
    n = len(x)
    assert n == 32
    d = DeepEndgame(R, C, max_free=ROOT_FREE)
    facts = [None] * n
    for k in range(4):
        rows = np.nonzero(game == k)[0]
        sc = d.solve(root_of(R, C, k)).score(x[rows])
        assert sc["solved"].all()
        for i, r in enumerate(rows):
            m, v = TR.margin_of(R, C, x[r]), int(sc["value"][i])
            O = [a for a in acts if x[r][a] == 0 and int(np.sign(m + int(sc["q"][i][a]))) == v]
            assert O and (sc["q"][i][[a for a in acts if x[r][a] == 0]] != ILLEGAL).all()
            facts[r] = dict(n_free=int(sc["n_free"][i]), touched=True, finished=False, v=v, O=O)
    pi = random_pi(n, A, seed=5 * R + C)
    pi[3, facts[3]["O"]] = 0.0  # no mass on O
    z = np.random.RandomState(R * C).randint(-1, 2, n).astype(np.float32)
    t = DeepTables(R, C, max_free=ROOT_FREE, n_tables=4).solve(np.stack([root_of(R, C, k) for k in range(4)]))
    for pi_mode, z_mode in MODES:
        want = TR.apply_targets(facts, pi, z, pi_mode, z_mode)
        got_pi, got_z, got = t.targets(x, game, pi, z, pi_mode, z_mode)
        assert np.array_equal(bits(got_pi), bits(want["pi"])) and np.array_equal(bits(got_z), bits(want["z"])), (pi_mode, z_mode)
        assert np.array_equal(got["n_free"], want["n_free"]) and np.array_equal(bits(got["mass"]), bits(want["mass"]))
        assert got["relabelled"].all() and got["mass"][3] == 0
    d.close()
    t.close()


# ---------------------------------------------------------------- 6. / 7. game-ordered rows end to end
_selfplay = {}


def selfplay_rows():
    """the 8 formula-evaluator 4x4 self-play games of test_hip_deep_endgame.py, played once and left unchanged"""
    if not _selfplay:
        from dotsboxesaz_amd.engine import Engine
        e = Engine(4, 4, 8, mcts_num_read=40, evaluator="formula")
        e.selfplay_start(8, 0)
        e.run()
        _selfplay.update({k: np.asarray(v) for k, v in e.fetch_samples().items()})
        e.close()
    return _selfplay


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


ARRAYS = ("value", "policy_mass", "played_optimal", "n_free", "solved")
MEANS = ("optimal_policy_mass", "played_optimal_rate", "z_agreement", "coverage")


@pytest.mark.parametrize("max_free", [16, 20])
def test_score_game_tails_in_chunks_equals_the_game_by_game_path(max_free):
    rows = selfplay_rows()
    n = len(rows["z"])
    assert len(set(rows["game_idx"].tolist())) == 8
    want = score_game_tails(rows, rows=4, cols=4, max_free=max_free)
    got = score_game_tails(rows, rows=4, cols=4, max_free=max_free, tables=3)  # chunks of 3, 3 and 2 games
    assert set(got) == set(want) and got["tables"] == want["tables"] == 8 and got["solve_ms"] > 0
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in MEANS:
        assert same(got[k], want[k]), k
    assert set(got["by_free"]) == set(want["by_free"])
    for k, v in want["by_free"].items():
        assert len(got["by_free"][k]) == max_free + 1 and got["by_free"][k].dtype == v.dtype and same(got["by_free"][k], v), k
    assert got["solved"].sum() > 8 * max_free * 0.5
    # rows in any order, and a handle of the caller's
    perm = np.random.RandomState(max_free).permutation(n)
    pool = DeepTables(4, 4, max_free=max_free, n_tables=3)
    shuffled = score_game_tails({k: v[perm] for k, v in rows.items()}, tables=pool)
    for k in ARRAYS:
        assert np.array_equal(shuffled[k], want[k][perm]), k
    assert shuffled["tables"] == 8 and same(shuffled["coverage"], want["coverage"])
    pool.close()


@pytest.mark.parametrize("max_free", [16, 20])
def test_game_tail_targets_equal_the_calls_by_hand(max_free):
    rows = selfplay_rows()
    n = len(rows["z"])
    x = rows["x"].reshape(n, 75)
    pi = np.asarray(rows["pi"], np.float32).reshape(n, 50)
    z = np.asarray(rows["z"], np.float32)
    left = free_of(4, 4, x)
    game, move = rows["game_idx"].astype(np.int64), rows["move_idx"].astype(np.int64)
    roots, table_of = [], np.full(n, -1, np.int32)
    for k, g in enumerate(sorted(set(game.tolist()))):
        late = np.nonzero((game == g) & (left <= max_free))[0]
        first = late[np.argmin(move[late])]
        roots.append(first)
        table_of[(game == g) & (move >= move[first])] = k
    assert len(roots) == 8 and ((table_of >= 0) == (left <= max_free)).all()
    t = DeepTables(4, 4, max_free=max_free, n_tables=8).solve(x[roots])
    unfinished = (t.score(x, table_of)["q"] != ILLEGAL).any(axis=1)
    for pi_mode, z_mode in (("restrict", True), ("uniform", False)):
        want_pi, want_z, want = t.targets(x, table_of, pi, z, pi_mode, z_mode)
        got_pi, got_z, got = game_tail_targets(rows, rows=4, cols=4, max_free=max_free, tables=3, pi_mode=pi_mode, z_mode=z_mode)
        assert got_pi.shape == (n, 50) and got_z.shape == z.shape and got["tables"] == 8
        assert np.array_equal(bits(got_pi), bits(want_pi)) and np.array_equal(bits(got_z), bits(want_z)), pi_mode
        for k in ("n_free", "mass", "relabelled"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
        before = left > max_free  # the rows before a game's root
        assert before.any() and np.array_equal(bits(got_pi[before]), bits(pi[before])) and np.array_equal(bits(got_z[before]), bits(z[before]))
        assert np.array_equal(got["relabelled"], (left <= max_free) & unfinished) and got["relabelled"].sum() >= 8 * 10
        if z_mode:
            assert np.array_equal(got_z[got["relabelled"]], t.score(x, table_of)["value"][got["relabelled"]].astype(np.float32))
    perm = np.random.RandomState(1).permutation(n)
    p2, z2, i2 = game_tail_targets({k: v[perm] for k, v in rows.items()}, rows=4, cols=4, max_free=max_free, tables=t)
    p1, z1, i1 = game_tail_targets(rows, rows=4, cols=4, max_free=max_free, tables=8)
    assert np.array_equal(bits(p2), bits(p1[perm])) and np.array_equal(bits(z2), bits(z1[perm])) and np.array_equal(i2["relabelled"], i1["relabelled"][perm])
    t.close()


# ---------------------------------------------------------------- 8. device tensors, streams, a solve behind queued calls
def test_device_tensors_streams_and_a_solve_behind_scoring_calls():
    import torch
    R, C = 6, 6
    x1, game = interleaved(R, C, 0, ROOT_FREE)
    x = np.concatenate([x1] * 8)  # 1 344 rows: many workgroups
    table_of = np.tile(game, 8)
    pi = random_pi(len(x), 98, seed=4)
    z = np.random.RandomState(4).randint(-1, 2, len(x)).astype(np.float32)
    roots = np.stack([root_of(R, C, g) for g in range(4)])
    t = DeepTables(R, C, max_free=ROOT_FREE, n_tables=4).solve(torch.as_tensor(roots).reshape(4, 3, 7, 7))
    got = t.score(x, table_of, pi)
    tg = t.targets(x, table_of, pi, z)
    assert got["solved"].all() and np.array_equal(got["value"][:168], got["value"][-168:])
    xt, pt, zt = torch.as_tensor(x).cuda().reshape(len(x), 3, 7, 7), torch.as_tensor(pi).cuda(), torch.as_tensor(z).cuda()
    tt = torch.as_tensor(table_of).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = t.score(xt, tt, pt)
        dev_pi, dev_z, dev_info = t.targets(xt, tt, pt, zt)
        # queued, not waited for: the solve below replaces the tables only after these calls have read them
        t.solve(roots[::-1])
        swapped = t.score(xt, 3 - tt, pt)
    side.synchronize()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values()) and dev_pi.is_cuda and dev_z.is_cuda
    assert all(v.is_cuda for v in dev_info.values())
    for k in got:
        assert np.array_equal(dev[k].cpu().numpy(), got[k]), k
        assert np.array_equal(swapped[k].cpu().numpy(), got[k]), k
    assert np.array_equal(bits(dev_pi.cpu().numpy()), bits(tg[0])) and np.array_equal(bits(dev_z.cpu().numpy()), bits(tg[1]))
    for k in tg[2]:
        assert np.array_equal(dev_info[k].cpu().numpy(), tg[2][k]), k
    assert np.array_equal(pt.cpu().numpy(), pi) and np.array_equal(zt.cpu().numpy(), z)  # the caller's tensors are never modified
    empty = t.score(np.zeros((0, 147), np.int16), np.zeros(0, np.int32), np.zeros((0, 98), np.float32))
    assert [empty[k].shape for k in KEYS] == [(0,), (0,), (0, 98), (0,), (0,), (0,)]
    e_pi, e_z, e_info = t.targets(np.zeros((0, 147), np.int16), np.zeros(0, np.int32), np.zeros((0, 98), np.float32), np.zeros(0, np.float32))
    assert e_pi.shape == (0, 98) and e_z.shape == (0,) and e_info["relabelled"].shape == (0,)
    t.close()
