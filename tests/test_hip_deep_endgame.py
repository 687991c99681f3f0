"""Deep endgames on the GPU (dbaz_deep_* in csrc/solver.hip, DeepEndgame / score_game_tails in dotsboxesaz_amd/endgame.py): one
position's table against the solved 3x3 board byte for byte, every work split against the numpy recurrence, the rows answered
from the table against Endgame.score bit for bit (F <= 16) and against endgame_ref.py (F = 17 .. 20), the served rule, and
score_game_tails against score_endgames on self-play rows."""
import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.endgame import DeepEndgame, Endgame, score_endgames, score_game_tails
from dotsboxesaz_amd.solver import ILLEGAL, Solver
import endgame_ref as ER

pytestmark = pytest.mark.gpu

ROOT_FREE = 20
BOARDS = [(4, 4), (6, 6), (2, 7)]


def random_games(R, C, n_games, seed):
    """tests/test_hip_endgame.py's recipe: feature rows of every position of n_games random games, each played until no edge is
    free (the rows after a game's end, early end included, are finished games), and the number of free edges of every row.  Even
    games: uniformly random play; odd games: a capture while there is one, else a move that leaves no box with three edges while
    there is one, else any."""
    d = O.dims(R, C)
    acts, boxes = ER.board(R, C)
    rs = np.random.RandomState(seed)
    xs = []
    for game in range(n_games):
        s = O.new_state(d)
        for left in range(len(acts), -1, -1):
            x = O.features(d, s).ravel().copy()
            xs.append(x)
            free = [a for a in acts if x[a] == 0]
            assert len(free) == left
            if game % 2:
                drawn = {a: [sum(x[o] != 0 for o in b) for b in boxes if a in b] for a in free}
                free = [a for a in free if 3 in drawn[a]] or [a for a in free if 2 not in drawn[a]] or free
            if free:
                O.play_(d, s, int(free[rs.randint(len(free))]))
    xs = np.array(xs, np.int16)
    return xs, (xs[:, acts] == 0).sum(axis=1)


def other_mover(R, C, x):
    """the same boards with the other player to move: plane 2 holds that player's doubled boxes_to_close"""
    _, boxes = ER.board(R, C)
    HW = (R + 1) * (C + 1)
    closed = sum((x[:, b] != 0).all(axis=1).astype(np.int64) for b in boxes)
    mine = (R * C - x[:, 2 * HW].astype(np.int64)) // 2
    y = x.copy()
    y[:, 2 * HW:] = (R * C - 2 * (closed - mine))[:, None]
    return y


def random_pi(n, A, seed):
    pi = np.random.RandomState(seed).rand(n, A).astype(np.float32)
    return pi / pi.sum(axis=1, keepdims=True)


def reference(R, C, x, pi):
    """endgame_ref of every row, stacked"""
    rows = [ER.endgame_ref(R, C, x[i], pi[i]) for i in range(len(x))]
    return dict(value=np.array([r["value"] for r in rows], np.int8), diff=np.array([r["diff"] for r in rows], np.int8),
                q=np.array([r["q"] for r in rows], np.int8), policy_mass=np.array([r["policy_mass"] for r in rows], np.float32),
                n_free=np.array([r["n_free"] for r in rows], np.int16), finished=np.array([r["finished"] for r in rows], bool))


def ref_table(R, C, x):
    """int8 T[2^F] of the subgame of one feature row, from the numpy recurrence"""
    acts, boxes = ER.board(R, C)
    idx = {a: j for j, a in enumerate(a for a in acts if x[a] == 0)}
    masks = [sum(1 << idx[a] for a in b if a in idx) for b in boxes]
    return ER.subgame(len(idx), [m for m in masks if m])


_games = {}
_deep_ref = {}


def games(R, C):
    """per board, built once and left unchanged: the 4 games of test_hip_endgame.py's case (seed 100 R + C) as (rows [E + 1, 3HW],
    free edges per row E .. 0) each; row E - F of a game is its position with F free edges"""
    if (R, C) not in _games:
        xs, left = random_games(R, C, 4, seed=100 * R + C)
        n = len(xs) // 4
        _games[(R, C)] = [(xs[g * n:(g + 1) * n], left[g * n:(g + 1) * n]) for g in range(4)]
    return _games[(R, C)]


def tail(R, C, game, lo, hi):
    """the rows of one game with lo <= F <= hi, deepest first, each also with the other player to move"""
    xs, left = games(R, C)[game]
    x = xs[(left >= lo) & (left <= hi)]
    return np.concatenate([x, other_mover(R, C, x)])


def root_of(R, C, game, free=ROOT_FREE):
    xs, left = games(R, C)[game]
    return xs[len(left) - 1 - free]


def deep_reference(R, C):
    """(x, pi, endgame_ref) of the rows with F = 17 .. 20 of a board's games, both movers, per game; computed once"""
    if (R, C) not in _deep_ref:
        out = []
        for game in range(4):
            x = tail(R, C, game, 17, ROOT_FREE)
            pi = random_pi(len(x), 2 * (R + 1) * (C + 1), seed=R + C + game)
            out.append((x, pi, reference(R, C, x, pi)))
        _deep_ref[(R, C)] = out
    return _deep_ref[(R, C)]


def check_unsolved(got, rows):
    assert not got["solved"][rows].any()
    assert (got["value"][rows] == 0).all() and (got["diff"][rows] == -128).all() and (got["q"][rows] == ILLEGAL).all()
    if got["policy_mass"] is not None:
        assert (got["policy_mass"][rows] == 0).all()


# ---------------------------------------------------------------- 1. against the solved board, byte for byte
def test_3x3_tables_equal_the_solved_board():
    sv = Solver(3, 3).solve()
    D = sv.table()
    d = DeepEndgame(3, 3, max_free=24)
    xs, left = random_games(3, 3, 1, seed=33)
    assert np.array_equal(left, np.arange(24, -1, -1))
    d.solve(xs[0])
    assert (d.n_free, d.d0, d.table_bytes) == (24, -3, 1 << 24) and d.solve_ms > 0
    assert np.array_equal(d.table(), D)
    assert np.array_equal(d.table(12345, 1000), D[12345:13345])
    for k in (5, 12):  # k edges drawn: the table is the slice of D over the root's free bits
        root_mask = sv.mask_of(xs[k])
        free_bits = [b for b in range(24) if not root_mask >> b & 1]
        assert len(free_bits) == 24 - k
        m = np.arange(1 << len(free_bits), dtype=np.int64)
        spread = np.zeros_like(m)
        for j, b in enumerate(free_bits):
            spread |= ((m >> j) & 1) << b
        got = d.solve(xs[k]).table()
        assert d.n_free == 24 - k and got.shape == m.shape and np.array_equal(got, D[root_mask | spread])
        assert d.d0 == int(D[root_mask])
    sv.close()
    d.close()


# ---------------------------------------------------------------- 2. the work split cannot matter
def test_every_work_split_writes_the_same_table():
    root = root_of(6, 6, 0, 10)
    want = ref_table(6, 6, root)
    assert want.shape == (1024,) and len(set(want.tolist())) > 2
    d = DeepEndgame(6, 6, max_free=12)
    for low_bits in (4, 6, 10, 0, -1):
        assert np.array_equal(d.solve(root, low_bits).table(), want), low_bits
        assert d.n_free == 10 and d.d0 == int(want[0]) and d.table_bytes == 4096
    for bad in (3, 11, 17, -2):  # below SOLVER_MIN_LOW, above F, above SOLVER_MAX_LOW
        with pytest.raises(_lib.DbazError) as ei:
            d.solve(root, bad)
        assert ei.value.code == _lib.EINVAL
    for free in (0, 1, 3):  # F < 4: the plain kernel, whatever low_bits says
        small = root_of(6, 6, 1, free)
        for low_bits in (0, 4):
            got = d.solve(small, low_bits).table()
            assert d.n_free == free and got.shape == (1 << free,) and np.array_equal(got, ref_table(6, 6, small)), (free, low_bits)
    d.close()


# ---------------------------------------------------------------- 3. against Endgame.score, bit for bit
@pytest.mark.parametrize("R,C", BOARDS)
def test_served_rows_equal_endgame_score_bit_for_bit(R, C):
    A = 2 * (R + 1) * (C + 1)
    g, d = Endgame(R, C), DeepEndgame(R, C, max_free=ROOT_FREE)
    finished = 0
    for game in range(4):
        x = tail(R, C, game, 0, 16)
        assert len(x) == 34
        pi = random_pi(len(x), A, seed=10 * R + C + game)
        d.solve(root_of(R, C, game))
        assert d.n_free == ROOT_FREE
        want, got = g.score(x, pi), d.score(x, pi)
        assert got["solved"].all() and want["solved"].all()
        for k in ("value", "diff", "q", "n_free", "policy_mass"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (game, k)
        assert d.score(x)["policy_mass"] is None and np.array_equal(d.score(x)["q"], want["q"])
        fin = (want["q"] == ILLEGAL).all(axis=1)
        finished += int(fin.sum())
        for seed in (0, 7):
            (p0, v0, s0), (p1, v1, s1) = g.policy(x, seed), d.policy(x, seed)
            assert s0.all() and s1.all() and p1.dtype == np.float32 and v1.dtype == np.float32
            assert np.array_equal(p1, p0) and np.array_equal(v1, v0), (game, seed)
            assert np.array_equal(p1.sum(axis=1), (~fin).astype(np.float32))
    assert finished >= 8  # the rows with no edge left, both movers
    g.close()
    d.close()


# ---------------------------------------------------------------- 4. beyond 16 free edges, against the numpy definition
@pytest.mark.parametrize("R,C", BOARDS)
def test_rows_beyond_16_equal_the_reference(R, C):
    d = DeepEndgame(R, C, max_free=ROOT_FREE)
    values = set()
    for game, (x, pi, want) in enumerate(deep_reference(R, C)):
        assert len(x) == 8 and sorted(want["n_free"].tolist()) == [17, 17, 18, 18, 19, 19, 20, 20] and not want["finished"].any()
        got = d.solve(root_of(R, C, game)).score(x, pi)
        assert got["solved"].all()
        for k in ("value", "diff", "q", "n_free"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (game, k)
        # at most 20 f32 additions of terms in [0, 1]: the bound of the existing endgame tests for the same sum
        assert got["policy_mass"].dtype == np.float32 and np.abs(got["policy_mass"] - want["policy_mass"]).max() <= 1e-5
        assert (got["policy_mass"] > 0).all()  # the best move always keeps the result
        p, v, served = d.policy(x, 0)
        best = np.where(want["q"] == want["q"].max(axis=1, keepdims=True), 1, 0).argmax(axis=1)  # the first optimal move
        assert served.all() and np.array_equal(p.argmax(axis=1), best) and np.array_equal(p.sum(axis=1), np.ones(8, np.float32))
        assert np.array_equal(v, want["value"].astype(np.float32))
        values |= set(want["value"].tolist())
    assert len(values) >= 2 if (R, C) == (6, 6) else values >= {-1, 1}
    d.close()


def test_rows_beyond_16_take_every_value():
    assert set().union(*(set(w["value"].tolist()) for b in BOARDS for _, _, w in deep_reference(*b))) == {-1, 0, 1}


# ---------------------------------------------------------------- 5. the served rule
def test_served_rule():
    R, C = 4, 4
    acts, _ = ER.board(R, C)
    A = 2 * (R + 1) * (C + 1)
    d = DeepEndgame(R, C, max_free=ROOT_FREE)
    xs, left = games(R, C)[0]
    with pytest.raises(_lib.DbazError) as ei:
        d.score(xs[-3:])
    assert ei.value.code == _lib.ESTATE
    with pytest.raises(_lib.DbazError) as ei:
        d.policy(xs[-3:])
    assert ei.value.code == _lib.ESTATE
    with pytest.raises(_lib.DbazError) as ei:
        d.table()
    assert ei.value.code == _lib.ESTATE
    root = root_of(R, C, 0)
    d.solve(root)
    own = xs[left == 12][0]                      # served
    foreign = root_of(R, C, 1, 12)               # a row of another game
    assert ((foreign[acts] == 0) & (root[acts] != 0)).any()
    undone = own.copy()                          # one edge free that the root has drawn
    undone[[a for a in acts if root[a] != 0][3]] = 0
    ends = tail(R, C, 0, 0, 16)
    ref = reference(R, C, ends, random_pi(len(ends), A, 1))
    fin = ref["finished"]
    assert (fin & (ref["n_free"] > 0)).any() and (fin & (ref["n_free"] == 0)).sum() == 2, "no early end among the rows"
    x = np.concatenate([[own, foreign, undone, own], ends[fin], [own]])
    pi = random_pi(len(x), A, seed=2)
    got = d.score(x, pi)
    n_fin = int(fin.sum())
    assert got["solved"].tolist() == [True, False, False, True] + [True] * n_fin + [True]
    check_unsolved(got, [1, 2])
    assert got["n_free"].tolist()[:4] == [12, 12, 13, 12]
    alone = d.score(own[None], pi[:1])
    for i in (0, 3, len(x) - 1):  # the served row is the same wherever it stands in the batch
        for k in ("value", "diff", "q"):
            assert np.array_equal(got[k][i], alone[k][0]), (i, k)
    want = ER.endgame_ref(R, C, own, pi[0])
    assert got["value"][0] == want["value"] and got["diff"][0] == want["diff"] and np.array_equal(got["q"][0], want["q"])
    assert abs(got["policy_mass"][0] - want["policy_mass"]) <= 1e-5
    # finished rows, early end included: the result, q all -128, no mass
    rows = np.arange(4, 4 + n_fin)
    assert np.array_equal(got["value"][rows], ref["value"][fin]) and np.array_equal(got["diff"][rows], ref["diff"][fin])
    assert (got["q"][rows] == ILLEGAL).all() and (got["policy_mass"][rows] == 0).all()
    assert np.array_equal(got["n_free"][rows], ref["n_free"][fin])
    p, v, served = d.policy(x, 7)
    assert served.tolist() == got["solved"].tolist() and (p[[1, 2]] == 0).all() and (v[[1, 2]] == 0).all()
    assert (p[rows] == 0).all() and np.array_equal(v[rows], ref["value"][fin].astype(np.float32))
    assert p[0].sum() == 1 and np.array_equal(p[0], p[3]) and want["q"][p[0].argmax()] == want["q"].max()

    # a root with more free edges than the handle holds: refused, no table left behind, and the next root is solved
    with pytest.raises(_lib.DbazError) as ei:
        d.solve(root_of(R, C, 0, ROOT_FREE + 1))
    assert ei.value.code == _lib.EINVAL and "21" in str(ei.value) and d.n_free == -1
    with pytest.raises(_lib.DbazError) as ei:
        d.score(x)
    assert ei.value.code == _lib.ESTATE
    # two solves on one handle, F = 18 then F = 9: the second table is right, and serves its own rows only
    for free in (18, 9):
        r = root_of(R, C, 1, free)
        assert np.array_equal(d.solve(r).table(), ref_table(R, C, r)) and d.n_free == free
    got = d.score(np.stack([root_of(R, C, 1, 9), root_of(R, C, 1, 10), root_of(R, C, 1, 4)]))
    assert got["solved"].tolist() == [True, False, True] and got["n_free"].tolist() == [9, 10, 4]
    d.close()


def test_a_reused_handle_keeps_nothing_of_the_table_before():
    """One handle, three roots of three games: F = 12, then F = 3 (8 bytes at the head of the same 4 096-byte region), then F = 12
    again.  After each solve the table is the new root's, byte for byte, d0 is its first entry, and of the three roots exactly
    those whose free edges are a subset of the current root's are served."""
    R, C = 6, 6
    acts, _ = ER.board(R, C)
    roots = np.stack([root_of(R, C, 0, 12), root_of(R, C, 1, 3), root_of(R, C, 2, 12)])
    free = roots[:, acts] == 0
    d = DeepEndgame(R, C, max_free=12)
    for i, root in enumerate(roots):
        want = ref_table(R, C, root)
        got = d.solve(root).table()
        assert got.shape == (1 << int(free[i].sum()),) and np.array_equal(got, want), i
        assert d.n_free == free[i].sum() and d.d0 == int(want[0]) and d.table_bytes == 4096
        inside = ~(free & ~free[i]).any(axis=1)  # per root: no free edge that the current root has drawn
        assert inside[i] and not inside.all()
        scored = d.score(roots)
        assert scored["solved"].tolist() == inside.tolist(), i
        check_unsolved(scored, np.nonzero(~inside)[0])
        assert scored["diff"][i] == want[0]
    d.close()


def test_a_row_laid_out_for_another_board_is_not_served():
    """The same position on the wrong handle size: 2x7 and 3x5 rows both have 72 values.  A 2x7 position with 20 free edges, read
    as a 3x5 row, still has more free real edges than the 3x5 root has at all: not served, next to a served 3x5 row."""
    strip = root_of(2, 7, 0)
    acts35 = ER.board(3, 5)[0]
    xs, left = random_games(3, 5, 1, seed=35)
    root, later = xs[left == 10][0], xs[left == 6][0]
    assert strip.shape == root.shape == (72,) and (strip[acts35] == 0).sum() > 10
    d = DeepEndgame(3, 5, max_free=12).solve(root)
    got = d.score(np.stack([later, strip, later]))
    assert got["solved"].tolist() == [True, False, True] and got["n_free"][1] == (strip[acts35] == 0).sum()
    check_unsolved(got, [1])
    want = ER.endgame_ref(3, 5, later)
    for i in (0, 2):
        assert got["value"][i] == want["value"] and got["diff"][i] == want["diff"] and np.array_equal(got["q"][i], want["q"])
    d.close()


def test_device_tensors_and_streams():
    import torch
    R, C = 6, 6
    x = np.concatenate([tail(R, C, 0, 0, ROOT_FREE)] * 30)  # 1 260 rows: many workgroups
    pi = random_pi(len(x), 98, seed=4)
    d = DeepEndgame(R, C, max_free=ROOT_FREE).solve(torch.as_tensor(root_of(R, C, 0)).reshape(3, 7, 7))
    got = d.score(x, pi)
    assert got["solved"].all() and np.array_equal(got["value"][:42], got["value"][-42:])
    xt, pt = torch.as_tensor(x).cuda().reshape(len(x), 3, 7, 7), torch.as_tensor(pi).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = d.score(xt, pt)
        pol = d.policy(xt, 7)
    side.synchronize()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values()) and all(t.is_cuda for t in pol)
    for k in got:
        assert np.array_equal(dev[k].cpu().numpy(), got[k]), k
    for a, b in zip(pol, d.policy(x, 7)):
        assert np.array_equal(a.cpu().numpy(), b)
    empty = d.score(np.zeros((0, 147), np.int16), np.zeros((0, 98), np.float32))
    assert [empty[k].shape for k in ("value", "diff", "q", "policy_mass", "n_free", "solved")] == [(0,), (0,), (0, 98), (0,), (0,), (0,)]
    d.close()


# ---------------------------------------------------------------- 6. end to end
def same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def test_score_game_tails_of_selfplay_rows():
    from dotsboxesaz_amd.engine import Engine
    e = Engine(4, 4, 8, mcts_num_read=40, evaluator="formula")
    e.selfplay_start(8, 0)
    e.run()
    rows = e.fetch_samples()
    e.close()
    n = len(rows["z"])
    x = np.asarray(rows["x"]).reshape(n, 75)
    acts, _ = ER.board(4, 4)
    left = (x[:, acts] == 0).sum(axis=1)
    n_games = len(set(rows["game_idx"].tolist()))
    assert n_games == 8
    want = score_endgames(rows, rows=4, cols=4, max_free=16)
    got = score_game_tails(rows, rows=4, cols=4, max_free=16)
    arrays, means = ("value", "policy_mass", "played_optimal", "n_free", "solved"), ("optimal_policy_mass", "played_optimal_rate", "z_agreement", "coverage")
    assert set(got) == set(want) | {"tables", "solve_ms"} and got["tables"] == n_games and got["solve_ms"] > 0
    for k in arrays:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in means:
        assert same(got[k], want[k]), k
    assert set(got["by_free"]) == set(want["by_free"])
    for k, v in want["by_free"].items():
        assert len(got["by_free"][k]) == 17 and got["by_free"][k].dtype == v.dtype and same(got["by_free"][k], v), k
    # rows in any order: the games are found by (game_idx, move_idx)
    perm = np.random.RandomState(0).permutation(n)
    shuffled = score_game_tails({k: np.asarray(v)[perm] for k, v in rows.items()}, rows=4, cols=4, max_free=16)
    for k in arrays:
        assert np.array_equal(shuffled[k], want[k][perm]), k

    deep = score_game_tails(rows, rows=4, cols=4, max_free=20)
    ok = left <= 16
    for k in arrays[:3]:
        assert np.array_equal(deep[k][ok], want[k][ok]), k
    assert np.array_equal(deep["solved"], left <= 20) and np.array_equal(deep["n_free"], left)
    assert deep["coverage"] > want["coverage"] and deep["coverage"] == pytest.approx((left <= 20).mean())
    assert deep["tables"] == n_games and len(deep["by_free"]["rows"]) == 21
    assert np.array_equal(deep["by_free"]["rows"], np.bincount(left[left <= 20], minlength=21))
    idx = np.nonzero((left > 16) & (left <= 20))[0]
    assert len(idx) >= 3 * n_games
    pi = np.asarray(rows["pi"], dtype=np.float32).reshape(n, 50)
    ref = reference(4, 4, x[idx], pi[idx])
    assert not ref["finished"].any()
    assert np.array_equal(deep["value"][idx], ref["value"]) and np.abs(deep["policy_mass"][idx] - ref["policy_mass"]).max() <= 1e-5
    played = np.asarray(rows["played"]).astype(np.int64)[idx]
    q_played = ref["q"][np.arange(len(idx)), played].astype(np.int64)
    e_ = x[idx][:, :50] != 0
    closed = sum(e_[:, b[0]] & e_[:, b[1]] & e_[:, b[2]] & e_[:, b[3]] for b in ER.board(4, 4)[1])
    margin = 2 * ((16 - x[idx][:, 50].astype(np.int64)) // 2) - closed
    assert (q_played != ILLEGAL).all() and np.array_equal(deep["played_optimal"][idx], np.sign(margin + q_played) == ref["value"])
