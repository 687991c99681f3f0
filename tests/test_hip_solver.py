"""Exact small-board solver on the GPU (csrc/solver.hip, dotsboxesaz_amd/solver.py): the solved table against the recurrence
restated in numpy, against recorded values of the 3x3 table, against a negamax over the oracle's rules, and the scoring
kernel's q / policy_mass / terminal rows against a host recomputation from the downloaded table."""
import hashlib

import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd._lib import DbazError
from dotsboxesaz_amd.solver import ILLEGAL, Solver, score_samples

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the recurrence, restated
def geometry(R, C):
    """(action index of compact edge i, per box its four compact edges)"""
    H, W = R + 1, C + 1
    HW = H * W
    acts = sorted([l * W + c for l in range(H) for c in range(C)] + [HW + l * W + c for l in range(R) for c in range(W)])
    idx = {a: i for i, a in enumerate(acts)}
    boxes = [[idx[l * W + c], idx[(l + 1) * W + c], idx[HW + l * W + c], idx[HW + l * W + c + 1]] for l in range(R) for c in range(C)]
    return acts, boxes


def move_q(boxes, D, s, e):
    """Q of drawing edge e in the masks s (all with e free): c + D[next] if it completes c > 0 boxes, else -D[next]"""
    c = np.zeros(len(s), np.int16)
    for b in boxes:
        if e in b:
            o = sum(1 << j for j in b if j != e)
            c += (s & np.uint32(o)) == o
    d = D[s | np.uint32(1 << e)].astype(np.int16)
    return np.where(c > 0, c + d, -d)


def best_q(boxes, E, D, s):
    """max Q over the free edges of the masks s (0 for the full mask)"""
    best = np.full(len(s), -128, np.int16)
    for e in range(E):
        free = (s >> np.uint32(e)) & 1 == 0
        best[free] = np.maximum(best[free], move_q(boxes, D, s[free], e))
    best[s == (1 << E) - 1] = 0
    return best


def solve_np(R, C):
    acts, boxes = geometry(R, C)
    E = len(acts)
    m = np.arange(1 << E, dtype=np.uint32)
    pc = np.zeros(1 << E, np.uint8)
    for i in range(E):
        pc += ((m >> np.uint32(i)) & 1).astype(np.uint8)
    D = np.zeros(1 << E, np.int8)
    for k in range(E - 1, -1, -1):
        s = m[pc == k]
        D[s] = best_q(boxes, E, D, s).astype(np.int8)
    return D


_solved = {}


def solved(R, C):
    """(Solver, its table on the host) of a board, solved once per session with the default kernel"""
    if (R, C) not in _solved:
        s = Solver(R, C).solve()
        _solved[(R, C)] = (s, s.table())
    return _solved[(R, C)]


def host_score(R, C, D, x, pi=None):
    """what k_solver_score computes for feature rows x [n, 3*H*W], from the table D on the host (policy mass in float64)"""
    acts, boxes = geometry(R, C)
    E, HW, A = len(acts), (R + 1) * (C + 1), 2 * (R + 1) * (C + 1)
    n = len(x)
    value, diff, q = np.zeros(n, np.int8), np.zeros(n, np.int8), np.full((n, A), ILLEGAL, np.int8)
    mass, terminal = np.zeros(n, np.float64), np.zeros(n, bool)
    for r in range(n):
        mask = sum(1 << i for i, a in enumerate(acts) if x[r, a] != 0)
        closed = sum(all(mask >> j & 1 for j in b) for b in boxes)
        own = int(x[r, 2 * HW])
        mine = (R * C - own) // 2
        theirs = closed - mine
        opp = R * C - 2 * theirs
        margin = mine - theirs
        diff[r] = D[mask]
        if (own == 0 and opp == 0) or own < 0 or opp < 0:
            terminal[r] = True
            value[r] = 0 if (own == 0 and opp == 0) else (1 if own < 0 else -1)
            continue
        value[r] = np.sign(margin + int(D[mask]))
        for i, a in enumerate(acts):
            if mask >> i & 1:
                continue
            q[r, a] = move_q(boxes, D, np.array([mask], np.uint32), i)[0]
            if pi is not None and np.sign(margin + int(q[r, a])) == value[r]:
                mass[r] += float(pi[r, a])
    return dict(value=value, diff=diff, q=q, policy_mass=mass, terminal=terminal)


def random_positions(R, C, n, seed):
    """feature rows of n positions reached by uniformly random legal play of a random number of plies (finished games,
    early end included, among them), and get_result of each"""
    d = O.dims(R, C)
    rs = np.random.RandomState(seed)
    E = 2 * R * C + R + C
    xs, res = [], []
    for i in range(n):
        s = O.new_state(d)
        for _ in range(i % (E + 1)):
            if O.get_result(s) is not None:
                break
            valid = np.nonzero(O.valid_moves(d, s))[0]
            O.play_(d, s, int(valid[rs.randint(len(valid))]))
        xs.append(O.features(d, s).ravel().copy())
        res.append(O.get_result(s))
    return np.array(xs, np.int16), res


# ---------------------------------------------------------------- 1. whole tables vs the numpy restatement
@pytest.mark.parametrize("R,C,d0", [(1, 1, -1), (1, 2, 0), (2, 2, 2), (1, 4, 0), (2, 3, -2), (3, 2, -2)])
def test_table_equals_the_recurrence(R, C, d0):
    want = solve_np(R, C)
    assert want[0] == d0
    s = Solver(R, C)
    E = s.n_edges
    # default, the plain kernel, the smallest subcube (most launches), the largest (fewest), one in between
    for low_bits in sorted({0, -1, 4, min(E, 16), max(4, E // 2)}):
        s.solve(low_bits)
        got = s.table()
        assert got.dtype == np.int8 and got.shape == (1 << E,)
        assert np.array_equal(got, want), "low_bits=%d: %d entries differ" % (low_bits, int((got != want).sum()))
        i = s.info()
        assert i["d0"] == d0 and i["n_edges"] == E and i["table_bytes"] == 1 << E and i["solve_ms"] > 0
    assert np.array_equal(s.table(5, 7), want[5:12])
    if (R, C) == (2, 3):
        assert hashlib.sha256(want.tobytes()).hexdigest() == "8f86a26e378c2af4042b945779083c7e3d8df2def4121b771581882e370d0beb"
    for bad in (-2, 3, 17, E + 1):
        with pytest.raises(DbazError):
            s.solve(bad)
    assert np.array_equal(s.table(), want)  # a refused call leaves the table alone
    s.close()


# ---------------------------------------------------------------- 2. 3x3
def test_3x3_table():
    s, D = solved(3, 3)
    assert s.info()["d0"] == -3 and D[0] == -3  # the second player wins 6-3
    assert int(D.astype(np.int64).sum()) == 62132964
    assert int((D >= 0).sum()) == 14442212
    sha = hashlib.sha256(D.tobytes()).hexdigest()
    assert sha == "0becf594de3c3f3ea6c7b50138a9202d22ff6458fc4365b4730bd667fd004d11"
    # 20 000 random masks, every popcount 0..24 represented, satisfy the recurrence
    rs = np.random.RandomState(7)
    n, E = 20000, 24
    order = np.argsort(rs.rand(n, E), axis=1)
    k = np.arange(n) % (E + 1)
    bits = np.where(np.arange(E)[None, :] < k[:, None], np.uint32(1) << order.astype(np.uint32), np.uint32(0))
    masks = np.bitwise_or.reduce(bits, axis=1).astype(np.uint32)
    pc = sum((masks >> np.uint32(i)) & 1 for i in range(E))
    assert np.array_equal(pc, k) and set(k) == set(range(E + 1))
    _, boxes = geometry(3, 3)
    assert np.array_equal(D[masks].astype(np.int16), best_q(boxes, E, D, masks))
    # solving again (twice on one handle), and with the plain kernel, gives identical bytes
    t = Solver(3, 3)
    for low_bits in (0, 0, -1):
        t.solve(low_bits)
        assert hashlib.sha256(t.table().tobytes()).hexdigest() == sha, low_bits
    t.close()


# ---------------------------------------------------------------- 3. against the rules
def negamax(d, s, memo):
    """true result for the player to move under optimal play by the oracle's rules (early end and draws included)"""
    r = O.get_result(s)
    if r is not None:
        return r
    key = (s.hash_int(), s.b2c2[0], s.b2c2[1], s.to_play)
    if key not in memo:
        best = -2
        for mv in np.nonzero(O.valid_moves(d, s))[0]:
            t = s.copy()
            O.play_(d, t, int(mv))
            v = negamax(d, t, memo)
            best = max(best, v if t.to_play == s.to_play else -v)
            if best == 1:
                break
        memo[key] = best
    return memo[key]


@pytest.mark.parametrize("R,C", [(2, 2), (1, 4)])
def test_value_equals_negamax_over_the_rules(R, C):
    d = O.dims(R, C)
    rs = np.random.RandomState(100 * R + C)
    memo, xs, want = {}, [], []
    for _ in range(40):
        s = O.new_state(d)
        while O.get_result(s) is None:
            xs.append(O.features(d, s).ravel().copy())
            want.append(negamax(d, s, memo))
            valid = np.nonzero(O.valid_moves(d, s))[0]
            O.play_(d, s, int(valid[rs.randint(len(valid))]))
    sv, _ = solved(R, C)
    got = sv.score(np.array(xs, np.int16))["value"]
    want = np.array(want, np.int8)
    assert len(got) == len(want) and set(want) >= {-1, 1}
    assert np.array_equal(got, want), "%d of %d positions differ" % (int((got != want).sum()), len(want))


# ---------------------------------------------------------------- 4. q and policy_mass
@pytest.mark.parametrize("R,C,n", [(2, 3, 300), (3, 3, 300)])
def test_q_and_policy_mass(R, C, n):
    sv, D = solved(R, C)
    x, res = random_positions(R, C, n, seed=R * 10 + C)
    rs = np.random.RandomState(5)
    pi = rs.rand(n, sv.A).astype(np.float32)
    pi /= pi.sum(axis=1, keepdims=True)
    got = sv.score(x, pi)
    want = host_score(R, C, D, x, pi)
    assert np.array_equal(got["q"], want["q"])
    assert np.array_equal(got["diff"], want["diff"]) and np.array_equal(got["value"], want["value"])
    # at most 40 f32 additions of terms in [0, 1]: 40 * 2^-24 ~ 2.4e-6
    assert got["policy_mass"].dtype == np.float32 and np.abs(got["policy_mass"] - want["policy_mass"]).max() <= 1e-5
    # illegal and sentinel slots
    acts, _ = geometry(R, C)
    sentinel = np.setdiff1d(np.arange(sv.A), acts)
    assert (got["q"][:, sentinel] == ILLEGAL).all()
    # finished games: value = get_result, q all -128, no mass
    term = np.array([r is not None for r in res])
    assert term.sum() >= 5 and np.array_equal(term, want["terminal"])
    assert any((x[i, acts] == 0).any() for i in np.nonzero(term)[0]), "no early end among the finished games"
    assert np.array_equal(got["value"][term], np.array([r for r in res if r is not None], np.int8))
    assert (got["q"][term] == ILLEGAL).all() and (got["policy_mass"][term] == 0).all()
    assert np.array_equal(got["q"][~term][:, acts] != ILLEGAL, x[~term][:, acts] == 0)  # legal = free edge
    assert (got["policy_mass"][~term] > 0).all()  # the best move always keeps the result
    # without pi; device tensors in, device tensors out
    import torch
    g2 = sv.score(x)
    assert g2["policy_mass"] is None and np.array_equal(g2["q"], got["q"]) and np.array_equal(g2["value"], got["value"])
    g3 = sv.score(torch.as_tensor(x).cuda().reshape(n, 3, R + 1, C + 1), torch.as_tensor(pi).cuda())
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in g3.values())
    for k_ in ("value", "diff", "q", "policy_mass"):
        assert np.array_equal(g3[k_].cpu().numpy(), got[k_]), k_
    assert sv.mask_of(x[7]) == sv.mask_of(x[7].reshape(3, R + 1, C + 1)) == sum(1 << i for i, a in enumerate(acts) if x[7, a])


# ---------------------------------------------------------------- 5. end to end
def test_score_samples_of_selfplay_rows():
    from dotsboxesaz_amd.engine import Engine
    sv, D = solved(3, 3)
    e = Engine(3, 3, 8, mcts_num_read=40, evaluator="formula")
    e.selfplay_start(8, 0)
    e.run()
    rows = e.fetch_samples()
    e.close()
    n = len(rows["z"])
    assert n >= 8 * 9
    got = score_samples(rows, solver=sv)
    want = host_score(3, 3, D, rows["x"], rows["pi"].astype(np.float32))
    assert len(got["value"]) == len(got["policy_mass"]) == len(got["played_optimal"]) == n
    assert np.array_equal(got["value"], want["value"]) and not want["terminal"].any()
    assert np.abs(got["policy_mass"] - want["policy_mass"]).max() <= 1e-5
    _, boxes = geometry(3, 3)
    acts = list(sv.actions)
    played_optimal = np.zeros(n, bool)
    for r in range(n):
        a = int(rows["played"][r])
        assert want["q"][r, a] != ILLEGAL  # the move played was legal
        mask = sv.mask_of(rows["x"][r])
        closed = sum(all(mask >> j & 1 for j in b) for b in boxes)
        mine = (9 - int(rows["x"][r, 32])) // 2
        played_optimal[r] = np.sign(2 * mine - closed + int(want["q"][r, a])) == want["value"][r]
        assert mask == sv.mask_of([acts_ for acts_ in acts if rows["x"][r, acts_]])
    assert np.array_equal(got["played_optimal"], played_optimal)
    assert abs(got["optimal_policy_mass"] - want["policy_mass"].mean()) <= 1e-5
    assert got["played_optimal_rate"] == pytest.approx(played_optimal.mean())
    assert got["z_agreement"] == pytest.approx((rows["z"] == want["value"]).mean())
    for k_ in ("optimal_policy_mass", "played_optimal_rate", "z_agreement"):
        assert 0.0 <= got[k_] <= 1.0
    # the board size from rows / cols instead of a ready solver: the same figures
    again = score_samples(rows, rows=3, cols=3)
    assert np.array_equal(again["value"], got["value"]) and again["z_agreement"] == got["z_agreement"]
