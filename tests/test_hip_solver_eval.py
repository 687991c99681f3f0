"""The solved table as an evaluator on the GPU (k_solver_eval in csrc/solver.hip; DBAZ_EVAL_SOLVER, dbaz_attach_solver,
dbaz_perfect_policy): the kernel against the numpy restatement (tests/solver_ref.py), the engine's three paths -- sequential
search, match play next to another evaluator, K pending -- bit for bit against the same searches fed by that restatement, and
perfect play end to end.  Every match here searches each move from a fresh root (reuse_tree=False, match play's configuration):
see test_solver_eval_cpu.py for why the one-hot prior needs it."""
import numpy as np
import pytest

from oracle import oracle as O
from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.solver import Solver
import solver_ref as SR
from test_hip_solver import solved

pytestmark = pytest.mark.gpu


def table_of(R, C):
    """(Solver, host table): the device's table (pinned by tests/test_hip_solver.py); where numpy solves the board in a blink,
    the restated recurrence must give the same bytes"""
    sv, D = solved(R, C)
    if 2 * R * C + R + C <= 17:
        assert np.array_equal(D, SR.table(R, C))
    return sv, D


def random_games(R, C, n, seed):
    """(feature rows of every position of n uniformly random games, the finished ones included; get_result of each)"""
    d = O.dims(R, C)
    rs = np.random.RandomState(seed)
    xs, res = [], []
    for _ in range(n):
        s = O.new_state(d)
        while True:
            xs.append(O.features(d, s).ravel().copy())
            res.append(O.get_result(s))
            if res[-1] is not None:
                break
            valid = np.nonzero(O.valid_moves(d, s))[0]
            O.play_(d, s, int(valid[rs.randint(len(valid))]))
    return np.array(xs, np.int16), res


def random_unfinished(d, rs, lo, hi):
    """a random legal move sequence of lo..hi plies (shorter if the game would end) that leaves the game unfinished"""
    moves, s = [], O.new_state(d)
    for _ in range(int(rs.randint(lo, hi + 1))):
        valid = np.nonzero(O.valid_moves(d, s))[0]
        m = int(valid[rs.randint(len(valid))])
        t = s.copy()
        O.play_(d, t, m)
        if O.get_result(t) is not None:
            break
        s = t
        moves.append(m)
    return moves


def value_of(D, R, C, d, moves):
    """true result of the position after `moves` for the player to move there"""
    return int(SR.policy_one(D, R, C, O.features(d, O.state_from_moves(d, moves)).ravel())[1])


def first_rows(got):
    return {int(got["game_idx"][i]): i for i in np.nonzero(got["move_idx"] == 0)[0]}


# ---------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("R,C", [(3, 3), (2, 3), (1, 4), (4, 2)])
def test_policy_equals_the_restatement(R, C):
    sv, D = table_of(R, C)
    x, res = random_games(R, C, 200, seed=10 * R + C)
    term = np.array([r is not None for r in res])
    assert term.sum() == 200 and (x[term][:, sv.actions] == 0).any(), "no early end among the finished games"
    sentinel = np.setdiff1d(np.arange(sv.A), sv.actions)
    picks = {}
    for seed in (0, 1, 7):
        p, v = sv.policy(x, seed)
        wp, wv = SR.policy_ref(D, R, C, x, seed)
        assert p.dtype == np.float32 and v.dtype == np.float32 and p.shape == (len(x), sv.A)
        assert np.array_equal(p.view(np.uint32), wp.view(np.uint32)), "seed %d: %d rows differ" % (seed, int((p != wp).any(axis=1).sum()))
        assert np.array_equal(v, wv)
        assert np.array_equal(np.sort(p, axis=1)[:, -2:][~term], np.tile(np.float32([0, 1]), ((~term).sum(), 1)))  # one 1.0f, zeros
        assert not p[term].any() and np.array_equal(v[term], np.float32([r for r in res if r is not None]))
        assert not p[:, sentinel].any()
        assert (x[np.nonzero(p)[0], np.nonzero(p)[1]] == 0).all()  # the picked edge is free
        picks[seed] = p.argmax(axis=1)
    assert (picks[0] != picks[7]).any() and (picks[1] != picks[7]).any()  # the seed matters where several moves are optimal
    import torch
    pt, vt = sv.policy(torch.as_tensor(x).cuda().reshape(-1, 3, R + 1, C + 1), 7)  # device tensors in, device tensors out
    assert pt.is_cuda and vt.is_cuda and np.array_equal(pt.cpu().numpy().argmax(axis=1), picks[7])
    p0, v0 = sv.policy(x[:0])
    assert p0.shape == (0, sv.A) and v0.shape == (0,)


# ---------------------------------------------------------------- 2. sequential search (float planes) vs the external path
@pytest.mark.parametrize("R,C,seed", [(3, 3, 0), (2, 3, 7)])
@pytest.mark.parametrize("noise", [(0.0, 0.0), (0.8, 0.25)])
def test_search_equals_external_search_fed_by_the_restatement(R, C, seed, noise):
    from dotsboxesaz_amd.engine import Engine
    sv, D = table_of(R, C)
    d = O.dims(R, C)
    E = 2 * R * C + R + C
    rs = np.random.RandomState(100 * R + C + seed)
    starts = [random_unfinished(d, rs, 2, E - 3) for _ in range(64)]
    a = Engine(R, C, 64, mcts_num_read=50, noise=noise, evaluator="solver", solver=sv, solver_seed=seed)
    b = Engine(R, C, 64, mcts_num_read=50, noise=noise, evaluator="external")
    n_eval = [0]

    def evaluate(x):
        n_eval[0] += len(x)
        return SR.policy_ref(D, R, C, x, seed)

    for reads in (1, 7, 50):
        nz = rs.dirichlet([noise[0]] * a.A, 64) if noise[0] > 0 else None
        a.set_positions(starts)
        b.set_positions(starts)
        a.search(reads, nz)
        b.search_external(evaluate, reads, nz)
        ra, rb = a.roots(), b.roots()
        for k in ra:
            assert np.array_equal(ra[k].view(np.uint8), rb[k].view(np.uint8)), (reads, k)
        assert (ra["visits"].sum(axis=1) == reads).all()
    ca = a.counters()
    assert ca["nn_evals"] > 0 and ca["cache_hits"] == 0 and ca["error_slots"] == 0
    a.close()
    b.close()


# ---------------------------------------------------------------- 3. solver vs solver
def book_3x3(n, seed):
    d = O.dims(3, 3)
    rs = np.random.RandomState(seed)
    return [[]] + [random_unfinished(d, rs, 0, 10) for _ in range(n - 1)]  # opening 0: the empty board


def test_solver_against_solver_keeps_every_openings_result():
    from dotsboxesaz_amd.engine import Engine
    sv, D = table_of(3, 3)
    d = O.dims(3, 3)
    book = book_3x3(32, 3)
    e = Engine(3, 3, 64, mcts_num_read=8, temperature={0: 1.0}, reuse_tree=False, match_play=True, evaluator="solver",
               evaluator2="solver", seed=5)
    e.attach_solver(sv, 0, seed=3)
    e.attach_solver(sv, 1, seed=11)
    e.selfplay_set_start(book, 2)
    e.selfplay_start(64, 0)
    e.run()
    c = e.counters()
    assert c["games_finished"] == 64 and c["error_slots"] == 0
    got = e.fetch_samples()
    e.close()
    fr = first_rows(got)
    assert sorted(fr) == list(range(64))
    for g, i in fr.items():
        assert int(got["z"][i]) == value_of(D, 3, 3, d, book[g // 2]), g  # z of the first row: the result for its mover
    assert D[0] == -3 and got["z"][fr[0]] == -1 and got["z"][fr[1]] == -1 and got["player"][fr[0]] == 0  # the second player wins
    # the value never changes hands: z of every row is the true value of its position
    assert np.array_equal(got["z"], sv.score(got["x"])["value"])


# ---------------------------------------------------------------- 4. solver next to another evaluator, rows vs the oracle
def test_solver_against_uniform_rows_equal_the_oracle():
    from dotsboxesaz_amd.engine import Engine
    sv, D = table_of(3, 3)
    d = O.dims(3, 3)
    seed = 5
    e = Engine(3, 3, 16, mcts_num_read=30, noise=(0.0, 0.0), reuse_tree=False, match_play=True, evaluator="uniform", evaluator2="solver",
               solver=sv, solver_seed=seed, seed=77)
    e.selfplay_start(16, 0)
    e.run()
    c = e.counters()
    assert c["games_finished"] == 16 and c["error_slots"] == 0
    got = e.fetch_samples()
    e.close()
    pp = O.selfplay_params(30, noise=(0.0, 0.0), reuse_tree=False)
    cur = {"model": 0, "game": 0}

    def fn(dd, s):
        if cur["model"] == 0:
            return O.eval_formula(dd, s, 1)
        return tuple(a[0] for a in SR.policy_ref(D, 3, 3, O.features(dd, s).ravel()[None], seed))

    ev = O.Evaluator(fn)
    for gi in range(16):
        cur["game"] = gi
        r = np.nonzero(got["game_idx"] == gi)[0]
        ref = O.play_game(d, pp, ev, forced_moves=got["played"][r], on_move=lambda tp: cur.__setitem__("model", tp ^ (cur["game"] & 1)))
        assert ref["n_rows"] == len(r)
        assert np.array_equal(ref["player"], got["player"][r]) and np.array_equal(ref["x"], got["x"][r])
        assert np.array_equal(ref["visits"], got["visits"][r])
        assert np.array_equal(ref["pi"].view(np.uint64), got["pi"][r].view(np.uint64))
        assert np.array_equal(ref["q_value"].view(np.uint32), got["q_value"][r].view(np.uint32))
        assert np.array_equal(ref["z"], got["z"][r].astype(np.int64))
        assert np.array_equal(ref["tree_size"], got["tree_size"][r]) and np.array_equal(ref["terminal_count"], got["terminal_count"][r])
        assert np.array_equal(ref["max_deepness"], got["max_deepness"][r].astype(np.int32))
        # the solver's side (model 1: second to move in even games) never ends below the theoretical result of the empty board
        z_first = int(got["z"][r[0]])  # for player 0, the first to move
        z_solver = -z_first if gi % 2 == 0 else z_first
        assert z_solver >= (1 if gi % 2 == 0 else -1), gi
    # and from wherever the solver first came to move, it got at least that position's value
    model = got["player"] ^ (got["game_idx"] & 1)
    true = sv.score(got["x"])["value"]
    for gi in range(16):
        r = np.nonzero((got["game_idx"] == gi) & (model == 1) & (got["played"] >= 0))[0]
        assert len(r) and (got["z"][r] >= true[r]).all(), gi


# ---------------------------------------------------------------- 5. solver_reads
def test_solver_reads_caps_the_driver_rule():
    from dotsboxesaz_amd.engine import Engine
    sv, _ = table_of(3, 3)
    book = book_3x3(8, 4)
    rows = []
    for reads, cap in ((800, 2), (2, 0)):
        e = Engine(3, 3, 16, mcts_num_read=reads, temperature={0: 1.0}, reuse_tree=False, match_play=True, evaluator="solver",
                   evaluator2="solver", solver=sv, solver_seed=9, solver_reads=cap, seed=21, nodes_per_slot=64)
        e.selfplay_set_start(book, 2)
        e.selfplay_start(16, 0)
        e.run()
        assert e.counters()["games_finished"] == 16
        rows.append(e.fetch_samples())
        e.close()
    assert len(rows[0]["z"]) > 16 * 10 and (rows[0]["visits"].sum(axis=1)[rows[0]["played"] >= 0] == 2).all()
    for k in rows[0]:
        assert np.array_equal(rows[0][k].view(np.uint8), rows[1][k].view(np.uint8)), k
    # explicit read counts are never touched
    e = Engine(3, 3, 2, mcts_num_read=800, evaluator="solver", solver=sv, solver_reads=2)
    e.set_positions([[0], [1, 5]])
    e.search(11)
    assert (e.roots()["visits"].sum(axis=1) == 11).all()
    e.set_positions([[0], [1, 5]])
    e.search()
    assert (e.roots()["visits"].sum(axis=1) == 2).all()
    e.close()


# ---------------------------------------------------------------- 6. K pending
@pytest.mark.parametrize("reads", [8, 37])
def test_pending_waves_equal_the_oracle(reads):
    from dotsboxesaz_amd.engine import Engine
    sv, D = table_of(3, 3)
    d = O.dims(3, 3)
    start = random_unfinished(d, np.random.RandomState(6), 5, 5)
    e = Engine(3, 3, 1, mcts_num_read=800, evaluator="solver", solver=sv, solver_seed=2, max_pending_evals=8)
    e.set_pending(8, virtual_visits=False)
    e.set_positions([start])
    e.search(reads)
    r = e.roots()
    e.close()
    t = O.Tree(d, O.state_from_moves(d, start))
    ev = O.Evaluator(lambda dd, s: tuple(a[0] for a in SR.policy_ref(D, 3, 3, O.features(dd, s).ravel()[None], 2)))
    vis = t.search(reads, ev, max_pending=8)
    _, tv, _, _ = t.root_arrays()
    assert vis.sum() == reads and np.array_equal(r["visits"][0], vis)
    assert np.array_equal(r["total_value"][0].view(np.uint32), tv.view(np.uint32))


# ---------------------------------------------------------------- 7. a network against perfect play
def test_solver_match_counts():
    import torch
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd.self_play import solver_match
    sv, D = table_of(3, 3)
    d = O.dims(3, 3)
    torch.manual_seed(0)
    params = dnn.resnet_params(3, 3, 16, 1)
    params["self_play"] = {"reuse_mcts_tree": True, "noise": [0.8, 0.25],
                           "mcts": {"mcts_num_read": 30, "mcts_cpuct": [1.25, 19652], "temperature": {0: 1.0, 12: 0.02}}}
    book = book_3x3(8, 12)
    out = solver_match(params, 0, 16, 3, 3, openings=book, solver=sv, solver_seed=1, nn_class=dnn.ResNetZero, n_slots=8)
    assert out["games"] == 16 == out["wins"] + out["draws"] + out["losses"] == sum(out["theory"].values())
    assert out["f32_fallback_evals"] == 0
    got = out["samples"]
    fr = first_rows(got)
    assert sorted(fr) == list(range(16))
    held = wins = 0
    th = dict(win=0, draw=0, loss=0)
    for g, i in fr.items():
        v = value_of(D, 3, 3, d, book[g // 2])  # for the mover of the opening
        assert v == int(sv.score(got["x"][i:i + 1])["value"][0])
        network_moves_first = (int(got["player"][i]) ^ (g & 1)) == 0
        theory = v if network_moves_first else -v
        z = int(got["z"][i]) if network_moves_first else -int(got["z"][i])
        th["win" if theory > 0 else "loss" if theory < 0 else "draw"] += 1
        held += z >= theory
        wins += z > 0
    assert out["held"] == held and out["theory"] == th and out["wins"] == wins
    assert out["held_rate"] == held / 16 and out["wins"] <= th["win"]  # nobody beats the table


# ---------------------------------------------------------------- 8. errors (none reaches a kernel; the handle stays usable)
def test_attach_and_search_errors():
    from dotsboxesaz_amd.engine import Engine
    sv, _ = table_of(3, 3)
    e = Engine(3, 3, 2, mcts_num_read=5, evaluator="solver")

    def code(fn):
        with pytest.raises(_lib.DbazError) as ei:
            fn()
        return ei.value.code

    assert code(lambda: e.search(3)) == _lib.ESTATE  # no table attached
    assert code(lambda: e.search_timed(1.0, 3)) == _lib.ESTATE
    assert code(lambda: e.selfplay_start(2, 0)) == _lib.ESTATE
    fresh = Solver(3, 3)
    assert code(lambda: e.attach_solver(fresh)) == _lib.ESTATE  # not solved
    assert code(lambda: fresh.policy(np.zeros((1, fresh.F), np.int16))) == _lib.ESTATE
    fresh.close()
    assert code(lambda: e.attach_solver(sv, 2)) == _lib.EINVAL
    assert code(lambda: e.attach_solver(sv, 1)) == _lib.EINVAL  # model 1's evaluator is the formula
    assert code(lambda: e.attach_solver(sv, 0, reads=-1)) == _lib.EINVAL
    assert code(lambda: Engine(3, 3, 2, evaluator="formula").attach_solver(sv)) == _lib.EINVAL
    assert code(lambda: Engine(2, 3, 2, evaluator="solver", solver=sv)) == _lib.EINVAL  # another board
    assert code(lambda: Engine(3, 3, 2, evaluator="uniform", evaluator2="external", match_play=True)) == _lib.EINVAL  # 4 stays rejected
    assert code(lambda: Engine(3, 3, 2, evaluator="uniform", evaluator2=6, match_play=True)) == _lib.EINVAL
    assert code(lambda: Engine(3, 3, 2, evaluator=6)) == _lib.EINVAL
    assert code(lambda: e.search(3)) == _lib.ESTATE  # none of the refused calls attached anything
    e.attach_solver(sv)
    e.set_positions(None)
    e.search(3)
    assert (e.roots()["visits"].sum(axis=1) == 3).all()
    e.close()
    # evaluator2 without match play is ignored, as for the other kinds
    e = Engine(3, 3, 2, mcts_num_read=5, evaluator="uniform", evaluator2="solver")
    e.set_positions(None)
    e.search(4)
    e.selfplay_start(2, 0)
    e.run()
    assert e.counters()["games_finished"] == 2
    e.close()
    # match play: model 1 without a table is refused where self-play starts
    e = Engine(3, 3, 2, mcts_num_read=5, evaluator="uniform", evaluator2="solver", match_play=True)
    assert code(lambda: e.selfplay_start(2, 0)) == _lib.ESTATE
    e.attach_solver(sv, 1)
    e.selfplay_start(2, 0)
    e.run()
    assert e.counters()["games_finished"] == 2
    e.close()
