"""Exact endgame solver on the GPU (csrc/endgame.hip, dotsboxesaz_amd/endgame.py): against the solved 3x3 table byte for byte,
against the numpy yardstick (endgame_ref.py) on boards the table cannot reach, max_free, many rows / streams, and the row report
of self-play rows end to end."""
import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd.endgame import Endgame, score_endgames
from dotsboxesaz_amd.solver import ILLEGAL, Solver
import endgame_ref as ER

pytestmark = pytest.mark.gpu


def random_games(R, C, n_games, seed):
    """feature rows of every position of n_games random games, each played until no edge is free (the rows after a game's end,
    early end included, are finished games), and the number of free edges of every row.  Even games: uniformly random play, whose
    late positions the mover nearly always wins; odd games: a capture while there is one, else a move that leaves no box with three
    edges while there is one, else any, which ends in chains to hand over and late positions of every value."""
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


def random_pi(n, A, seed):
    pi = np.random.RandomState(seed).rand(n, A).astype(np.float32)
    return pi / pi.sum(axis=1, keepdims=True)


def reference(R, C, x, pi):
    """endgame_ref of every row, stacked"""
    rows = [ER.endgame_ref(R, C, x[i], pi[i]) for i in range(len(x))]
    return dict(value=np.array([r["value"] for r in rows], np.int8), diff=np.array([r["diff"] for r in rows], np.int8),
                q=np.array([r["q"] for r in rows], np.int8), policy_mass=np.array([r["policy_mass"] for r in rows], np.float32),
                n_free=np.array([r["n_free"] for r in rows], np.int16), finished=np.array([r["finished"] for r in rows], bool))


_cases = {}


def other_mover(R, C, x):
    """the same boards with the other player to move: plane 2 holds that player's doubled boxes_to_close"""
    _, boxes = ER.board(R, C)
    HW = (R + 1) * (C + 1)
    closed = sum((x[:, b] != 0).all(axis=1).astype(np.int64) for b in boxes)
    mine = (R * C - x[:, 2 * HW].astype(np.int64)) // 2
    y = x.copy()
    y[:, 2 * HW:] = (R * C - 2 * (closed - mine))[:, None]
    return y


def case(R, C):
    """(x, pi, reference, deep rows) of a board, built once and left unchanged: from 4 random games the rows with 16 and 15 free
    edges (4 each) and all 60 rows with 0 .. 14, each also with the other player to move (random play leaves the mover ahead: these
    are the rows the mover loses); deep rows = some with more than 16 free edges"""
    if (R, C) not in _cases:
        xs, left = random_games(R, C, 4, seed=100 * R + C)
        x = xs[left <= 16]
        x = np.concatenate([x, other_mover(R, C, x)])
        pi = random_pi(len(x), 2 * (R + 1) * (C + 1), seed=R + C)
        _cases[(R, C)] = (x, pi, reference(R, C, x, pi), xs[left > 16][::3])
    return _cases[(R, C)]


def check_unsolved(got, rows):
    assert not got["solved"][rows].any()
    assert (got["value"][rows] == 0).all() and (got["diff"][rows] == -128).all() and (got["q"][rows] == ILLEGAL).all()
    if got["policy_mass"] is not None:
        assert (got["policy_mass"][rows] == 0).all()


# ---------------------------------------------------------------- 1. against the solved table, byte for byte
def test_3x3_equals_the_solved_table():
    acts, _ = ER.board(3, 3)
    x, left = random_games(3, 3, 16, seed=33)  # 16 games x 25 rows, n_free 0 .. 24
    assert len(x) == 400
    pi = random_pi(len(x), 32, seed=1)
    sv, g = Solver(3, 3).solve(), Endgame(3, 3)
    want, got = sv.score(x, pi), g.score(x, pi)
    sv.close()
    g.close()
    assert np.array_equal(got["n_free"], left) and got["n_free"].dtype == np.int16
    ok = left <= 16
    assert np.array_equal(got["solved"], ok) and ok.sum() >= 200 and (~ok).sum() >= 100
    for k in ("value", "diff", "q"):
        assert got[k].dtype == np.int8 and np.array_equal(got[k][ok], want[k][ok]), k
    # at most 16 f32 additions of terms in [0, 1]
    assert got["policy_mass"].dtype == np.float32 and np.abs(got["policy_mass"][ok] - want["policy_mass"][ok]).max() <= 1e-5
    check_unsolved(got, ~ok)
    finished = ok & (want["q"] == ILLEGAL).all(axis=1)
    assert finished.sum() >= 16 and (finished & (left > 0)).any(), "no early end among the solved rows"
    assert (~finished & ok).sum() >= 100


# ---------------------------------------------------------------- 2. boards the table cannot reach
@pytest.mark.parametrize("R,C", [(4, 4), (6, 6), (2, 7)])
def test_larger_boards_equal_the_reference(R, C):
    x, pi, want, _ = case(R, C)
    count = np.bincount(want["n_free"], minlength=17)
    assert count[16] >= 4 and count[15] >= 4 and count[:15].sum() >= 40 and count[0] >= 1 and count[1] >= 1
    g = Endgame(R, C)
    got, again = g.score(x, pi), g.score(x)  # again: without pi
    g.close()
    assert got["solved"].all()
    for k in ("value", "diff", "q", "n_free"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, np.nonzero((got[k] != want[k]).reshape(len(x), -1).any(axis=1))[0])
    assert got["policy_mass"].dtype == np.float32 and np.abs(got["policy_mass"] - want["policy_mass"]).max() <= 1e-5
    acts, _ = ER.board(R, C)
    sentinel = np.setdiff1d(np.arange(g.A), acts)
    fin = want["finished"]
    assert fin.any() and (~fin).sum() >= 20 and set(want["value"][~fin]) >= {-1, 1}
    assert (got["q"][:, sentinel] == ILLEGAL).all() and (got["q"][fin] == ILLEGAL).all() and (got["policy_mass"][fin] == 0).all()
    legal = np.zeros(got["q"].shape, bool)
    legal[:, acts] = x[:, acts] == 0
    assert np.array_equal(got["q"][~fin] != ILLEGAL, legal[~fin])
    assert (got["policy_mass"][~fin] > 0).all()  # the best move always keeps the result
    assert again["policy_mass"] is None and np.array_equal(again["q"], got["q"]) and np.array_equal(again["value"], got["value"])


# ---------------------------------------------------------------- 3. max_free
def test_max_free_is_honoured():
    x, pi, want, _ = case(4, 4)
    g = Endgame(4, 4, max_free=10)
    got = g.score(x, pi)
    g.close()
    assert g.max_free == 10 and np.array_equal(got["n_free"], want["n_free"])
    ok = want["n_free"] <= 10
    assert np.array_equal(got["solved"], ok) and ok.sum() >= 40 and set(want["n_free"][~ok]) == set(range(11, 17))
    check_unsolved(got, ~ok)
    full = Endgame(4, 4).score(x, pi)
    for k in ("value", "diff", "q", "policy_mass"):
        assert np.array_equal(got[k][ok], full[k][ok]), k


# ---------------------------------------------------------------- 4. many rows, grid and stream
def test_many_rows_and_streams():
    import torch
    x0, pi0, want, deep = case(6, 6)
    n = 5000
    src = np.arange(n) % len(x0)
    x, pi = x0[src].copy(), pi0[src].copy()
    at = np.array([0, 511, 512, 2048, 3333, 4999])  # unsolved rows among the solved ones
    x[at] = deep[:len(at)]
    ok = np.ones(n, bool)
    ok[at] = False
    acts, _ = ER.board(6, 6)
    g = Endgame(6, 6)
    got = g.score(x, pi)
    assert np.array_equal(got["solved"], ok) and np.array_equal(got["n_free"][at], (deep[:len(at), acts] == 0).sum(axis=1))
    check_unsolved(got, at)
    for k in ("value", "diff", "q", "n_free"):
        assert np.array_equal(got[k][ok], want[k][src][ok]), k
    assert np.abs(got["policy_mass"][ok] - want["policy_mass"][src][ok]).max() <= 1e-5
    # device tensors on another stream: the same bytes
    xt, pt = torch.as_tensor(x).cuda().reshape(n, 3, 7, 7), torch.as_tensor(pi).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = g.score(xt, pt)
    side.synchronize()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values())
    for k in got:
        assert np.array_equal(dev[k].cpu().numpy(), got[k]), k
    empty = g.score(np.zeros((0, 147), np.int16), np.zeros((0, 98), np.float32))
    assert [empty[k].shape for k in ("value", "diff", "q", "policy_mass", "n_free", "solved")] == [(0,), (0,), (0, 98), (0,), (0,), (0,)]
    g.close()


# ---------------------------------------------------------------- 5. end to end
def test_score_endgames_of_selfplay_rows():
    from dotsboxesaz_amd.engine import Engine
    e = Engine(4, 4, 8, mcts_num_read=40, evaluator="formula")
    e.selfplay_start(8, 0)
    e.run()
    rows = e.fetch_samples()
    e.close()
    n = len(rows["z"])
    x = np.asarray(rows["x"]).reshape(n, 75)
    acts, boxes = ER.board(4, 4)
    left = (x[:, acts] == 0).sum(axis=1)
    ok = left <= 16
    got = score_endgames(rows, rows=4, cols=4)
    assert all(len(got[k]) == n for k in ("value", "policy_mass", "played_optimal", "n_free", "solved"))
    assert np.array_equal(got["n_free"], left) and np.array_equal(got["solved"], ok)
    assert got["coverage"] == pytest.approx(ok.mean()) and 0.0 < got["coverage"] < 1.0
    idx = np.nonzero(ok)[0]
    pi = np.asarray(rows["pi"], dtype=np.float32).reshape(n, 50)
    want = reference(4, 4, x[idx], pi[idx])
    assert not want["finished"].any()  # every sample row is a position a move was played from
    assert np.array_equal(got["value"][idx], want["value"]) and np.abs(got["policy_mass"][idx] - want["policy_mass"]).max() <= 1e-5
    played = np.asarray(rows["played"]).astype(np.int64)[idx]
    q_played = want["q"][np.arange(len(idx)), played].astype(np.int64)
    assert (q_played != ILLEGAL).all()
    e_ = x[idx][:, :50] != 0
    closed = sum(e_[:, b[0]] & e_[:, b[1]] & e_[:, b[2]] & e_[:, b[3]] for b in boxes)
    margin = 2 * ((16 - x[idx][:, 50].astype(np.int64)) // 2) - closed
    played_optimal = np.sign(margin + q_played) == want["value"]
    assert np.array_equal(got["played_optimal"][idx], played_optimal) and not got["played_optimal"][~ok].any()
    z_ok = np.asarray(rows["z"]).reshape(n)[idx] == want["value"]
    assert got["optimal_policy_mass"] == pytest.approx(want["policy_mass"].astype(np.float64).mean(), abs=1e-5)
    assert got["played_optimal_rate"] == pytest.approx(played_optimal.mean(), abs=1e-5)
    assert got["z_agreement"] == pytest.approx(z_ok.mean(), abs=1e-5)
    by = got["by_free"]
    assert all(len(by[k]) == 17 for k in ("rows", "played_optimal_rate", "optimal_policy_mass", "z_agreement"))
    assert by["rows"].sum() == ok.sum() and np.array_equal(by["rows"], np.bincount(left[ok], minlength=17))
    for f in range(17):
        at_f = want["n_free"] == f
        if not at_f.any():
            assert all(np.isnan(by[k][f]) for k in ("played_optimal_rate", "optimal_policy_mass", "z_agreement"))
            continue
        assert by["played_optimal_rate"][f] == pytest.approx(played_optimal[at_f].mean(), abs=1e-5)
        assert by["optimal_policy_mass"][f] == pytest.approx(want["policy_mass"][at_f].astype(np.float64).mean(), abs=1e-5)
        assert by["z_agreement"][f] == pytest.approx(z_ok[at_f].mean(), abs=1e-5)
    # a ready handle with a smaller max_free: fewer rows solved, the same values on them
    g = Endgame(4, 4, max_free=8)
    less = score_endgames(rows, endgame=g)
    g.close()
    assert np.array_equal(less["solved"], left <= 8) and len(less["by_free"]["rows"]) == 9
    assert np.array_equal(less["value"][left <= 8], got["value"][left <= 8]) and less["coverage"] < got["coverage"]
