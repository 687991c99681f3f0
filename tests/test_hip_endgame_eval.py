"""The endgame solver as an evaluator on the GPU (csrc/endgame.hip).
Stateless form (k_endgame_policy, Endgame.policy): bit for bit against the numpy restatement (endgame_policy_ref.py) on boards with
and without a solved table, with early ends, sentinel slots, unsolved rows, max_free, seeds and streams; and against the solved
3x3 table's evaluator.
Inside the search (dbaz_attach_endgame: k_endgame_table, k_endgame_eval, the routing in tree.hip): the table path against an
external-evaluator engine fed by the restatement, byte for byte; roots above max_free against a handle with nothing attached;
self-play, match play, K pending, endgame_reads and the attach errors.  Every self-play and match here searches each move from a
fresh root without noise: the guarantee's condition."""
import numpy as np
import pytest

from dotsboxesaz_amd.endgame import Endgame
from dotsboxesaz_amd.solver import Solver
import endgame_policy_ref as PR
import endgame_ref as ER

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 7)
_cases = {}


def case(R, C):
    """(rows, free edges per row) of two random games of the board, built once and left unchanged: every row with at most 16 free
    edges (F = 16 .. 0, rows behind an early end included), each also with the other player to move, and every third of the deeper
    ones"""
    if (R, C) not in _cases:
        x, left = PR.random_games(R, C, 2, seed=100 * R + C)
        keep = (left <= 16) | (np.arange(len(x)) % 3 == 0)
        late = left <= 16
        _cases[(R, C)] = (np.concatenate([x[keep], PR.other_mover(R, C, x[late])]), np.concatenate([left[keep], left[late]]))
    return _cases[(R, C)]


def check(R, C, max_free, x, left):
    g = Endgame(R, C, max_free=max_free)
    acts, _ = ER.board(R, C)
    sentinel = np.setdiff1d(np.arange(g.A), acts)
    picks = {}
    for seed in SEEDS:
        p, v, solved = g.policy(x, seed)
        want_p, want_v, want_s = PR.policy(R, C, x, seed, max_free)
        assert p.dtype == np.float32 and p.shape == (len(x), g.A) and v.dtype == np.float32 and solved.dtype == bool
        assert np.array_equal(solved, want_s) and np.array_equal(solved, left <= max_free)
        assert np.array_equal(v, want_v), (seed, np.nonzero(v != want_v)[0])
        assert np.array_equal(p, want_p), (seed, np.nonzero((p != want_p).any(axis=1))[0])
        assert not p[:, sentinel].any() and not p[~solved].any() and not v[~solved].any()
        picks[seed] = p
    g.close()
    return picks


@pytest.mark.parametrize("R,C,max_free", [(3, 3, 16), (3, 3, 8), (4, 4, 16), (2, 7, 16), (6, 6, 16), (6, 6, 11)])
def test_policy_equals_the_restatement(R, C, max_free):
    x, left = case(R, C)
    count = np.bincount(np.minimum(left, 17), minlength=18)
    assert (count[:17] >= 2).all() and count[17] >= 2  # every depth 0 .. 16 and rows that are not solved
    picks = check(R, C, max_free, x, left)
    solved = left <= max_free
    one_hot = picks[0].sum(axis=1) == 1
    assert (one_hot | ~solved | (picks[0].sum(axis=1) == 0)).all()
    assert (solved & ~one_hot & (left > 0)).any(), "no early end among the solved rows"
    assert (one_hot & (left == max_free)).any()
    assert any((picks[s] != picks[0]).any() for s in SEEDS[1:]), "a seeded pick never left the first optimal move"
    assert set(PR.policy(R, C, x, 0, max_free)[1][solved]) >= {-1.0, 1.0}


def test_3x3_equals_the_solved_table_at_seed_0():
    x, left = PR.random_games(3, 3, 16, seed=33)
    sv, g = Solver(3, 3).solve(), Endgame(3, 3)
    want_p, want_v = sv.policy(x, 0)
    p, v, solved = g.policy(x, 0)
    sv.close()
    ok = left <= 16
    assert np.array_equal(solved, ok) and ok.sum() >= 200 and (~ok).sum() >= 100
    assert np.array_equal(p[ok], want_p[ok]) and np.array_equal(v[ok], want_v[ok])
    assert not p[~ok].any() and not v[~ok].any()
    assert set(v[ok]) >= {-1.0, 1.0} and (p[ok].sum(axis=1) == 0).any()
    # k_endgame_score shares the setup and the solve: the pick is one of its best moves and v its value
    sc = g.score(x)
    g.close()
    rows = np.nonzero(ok & (p.sum(axis=1) == 1))[0]
    q = sc["q"].astype(np.int64)
    assert (q[rows, np.argmax(p[rows], axis=1)] == q[rows].max(axis=1)).all() and np.array_equal(v[ok], sc["value"][ok].astype(np.float32))


def test_many_rows_device_tensors_and_streams():
    import torch
    x0, left0 = case(6, 6)
    n = 1500
    src = np.arange(n) % len(x0)
    x = x0[src]
    want_p, want_v, want_s = PR.policy(6, 6, x0, 7)
    g = Endgame(6, 6)
    p, v, solved = g.policy(x, 7)
    assert np.array_equal(p, want_p[src]) and np.array_equal(v, want_v[src]) and np.array_equal(solved, want_s[src])
    xt = torch.as_tensor(x).cuda().reshape(n, 3, 7, 7)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = g.policy(xt, 7)
    side.synchronize()
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in dev)
    for a, b in zip(dev, (p, v, solved)):
        assert np.array_equal(a.cpu().numpy(), b)
    empty = g.policy(np.zeros((0, 147), np.int16))
    assert [t.shape for t in empty] == [(0, 98), (0,), (0,)]
    g.close()


# ---------------------------------------------------------------- the table path on its own, int16 rows
@pytest.mark.parametrize("R,C,max_free", [(4, 4, 16), (6, 6, 16), (2, 7, 9)])
def test_table_path_equals_the_restatement_on_int16_rows(R, C, max_free):
    """k_endgame_table + k_endgame_eval<int16> without an engine: a game's row with F0 free edges is the root, that game's later
    rows (sub-positions of it, finished ones included) and the same with the other player to move are its leaves"""
    x, left = PR.random_games(R, C, 2, seed=100 * R + C)
    per_game = len(x) // 2
    roots, leaves, k = [], [], 2 * 17
    for game in range(2):
        gx, gl = x[game * per_game:(game + 1) * per_game], left[game * per_game:(game + 1) * per_game]
        for f0 in (max_free, max_free - 5, 3, 0, max_free + 1):
            root = gx[gl == f0][0]
            sub = gx[gl <= f0][:17]
            sub = np.concatenate([sub, PR.other_mover(R, C, sub)])
            roots.append(root)
            leaves.append(np.concatenate([sub, np.repeat(root[None], k - len(sub), axis=0)]))
    roots, leaves = np.array(roots), np.array(leaves)
    g = Endgame(R, C, max_free=max_free)
    for seed in SEEDS:
        p, v = g.policy_from(roots, leaves, seed)
        assert p.shape == (len(roots), k, g.A) and v.shape == (len(roots), k) and p.dtype == np.float32 and v.dtype == np.float32
        for i in range(len(roots)):
            want_p, want_v, _ = PR.policy(R, C, leaves[i], seed, max_free)
            if (roots[i][ER.board(R, C)[0]] == 0).sum() > max_free:  # no table: every row of this root is unanswered
                want_p, want_v = np.zeros_like(want_p), np.zeros_like(want_v)
            assert np.array_equal(p[i], want_p) and np.array_equal(v[i], want_v), (seed, i)
        sp, sv, _ = g.policy(leaves.reshape(-1, g.F), seed)  # the stateless kernel on the same rows
        has_table = np.repeat((roots[:, ER.board(R, C)[0]] == 0).sum(axis=1) <= max_free, k)
        assert np.array_equal(p.reshape(-1, g.A)[has_table], sp[has_table]) and np.array_equal(v.reshape(-1)[has_table], sv[has_table])
    assert len(g.last_ms) == 2 and all(t > 0 for t in g.last_ms)
    assert (p.sum(axis=2) == 1).any() and (p.sum(axis=2) == 0).any() and set(v.ravel()) >= {-1.0, 1.0}
    e = g.policy_from(np.zeros((0, g.F), np.int16), np.zeros((0, 1, g.F), np.int16))
    assert e[0].shape == (0, 1, g.A) and e[1].shape == (0, 1)
    g.close()


# ================================================================ the tables inside the search (dbaz_attach_endgame)
from oracle import oracle as O  # noqa: E402
from dotsboxesaz_amd import _lib  # noqa: E402
from dotsboxesaz_amd.endgame import score_endgames  # noqa: E402


def start_with_free(d, rs, n_edges, free):
    """a random legal move sequence that leaves `free` free edges and the game unfinished"""
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


_starts = {}


def starts_below(R, C, max_free):
    """64 starts with F <= max_free, built once: four at max_free, the others cycling through max_free - 1 .. 3"""
    if (R, C, max_free) not in _starts:
        d, rs = O.dims(R, C), np.random.RandomState(7 * R + C + max_free)
        E = 2 * R * C + R + C
        frees = [max_free] * 4 + [max_free - 1 - i % (max_free - 3) for i in range(60)]
        _starts[(R, C, max_free)] = ([start_with_free(d, rs, E, f) for f in frees], np.array(frees))
    return _starts[(R, C, max_free)]


def starts_above(R, C, max_free, n=64, seed=3):
    """starts with F = max_free + 1 .. max_free + 6: their leaves drop below max_free, their roots never do"""
    d, rs = O.dims(R, C), np.random.RandomState(seed)
    E = 2 * R * C + R + C
    frees = [max_free + 1 + i % 6 for i in range(n)]
    return [start_with_free(d, rs, E, f) for f in frees], np.array(frees)


def rows_of(R, C, starts):
    d = O.dims(R, C)
    return np.array([O.features(d, O.state_from_moves(d, m)).ravel() for m in starts], np.int16)


def restated(R, C, seed, max_free):
    def evaluate(x):
        p, v, _ = PR.policy(R, C, x, seed, max_free)
        return p, v
    return evaluate


def same_roots(ra, rb, slots=slice(None), what=""):
    for k in ra:
        assert np.array_equal(np.ascontiguousarray(ra[k][slots]).view(np.uint8), np.ascontiguousarray(rb[k][slots]).view(np.uint8)), (what, k)


# ---------------------------------------------------------------- (b) the table path equals the stateless path
@pytest.mark.parametrize("R,C,max_free,seed", [(4, 4, 16, 0), (3, 3, 8, 7)])
@pytest.mark.parametrize("noise", [(0.0, 0.0), (0.8, 0.25)])
def test_search_equals_external_search_fed_by_the_restatement(R, C, max_free, seed, noise):
    from dotsboxesaz_amd.engine import Engine
    starts, frees = starts_below(R, C, max_free)
    g = Endgame(R, C, max_free=max_free)
    a = Engine(R, C, 64, mcts_num_read=50, noise=noise, evaluator="formula", endgame=g, endgame_seed=seed)
    b = Engine(R, C, 64, mcts_num_read=50, noise=noise, evaluator="external")
    rs = np.random.RandomState(R + C)
    served = 0
    for reads in (1, 7, 50):
        nz = rs.dirichlet([noise[0]] * a.A, 64) if noise[0] > 0 else None
        a.set_positions(starts)
        b.set_positions(starts)
        a.search(reads, nz)
        b.search_external(restated(R, C, seed, max_free), reads, nz)
        ra, rb = a.roots(), b.roots()
        same_roots(ra, rb, what=reads)
        assert (ra["visits"].sum(axis=1) == reads).all()
        served += 64  # the root expansions; every other non-terminal leaf too
        assert a.endgame_stats()[0] == 64 * (1 + (1, 7, 50).index(reads)) and a.endgame_stats()[1] >= served
    c = a.counters()
    assert c["nn_evals"] == 0 and c["error_slots"] == 0
    a.close()
    b.close()
    g.close()


# ---------------------------------------------------------------- (c) nothing else changes
def test_roots_above_max_free_are_untouched_and_mixed_populations():
    from dotsboxesaz_amd.engine import Engine
    R, C, max_free, reads = 4, 4, 10, 30
    above, _ = starts_above(R, C, max_free)
    g = Endgame(R, C, max_free=max_free)
    a = Engine(R, C, 64, mcts_num_read=50, evaluator="formula", endgame=g, endgame_seed=1)
    plain = Engine(R, C, 64, mcts_num_read=50, evaluator="formula")
    ext = Engine(R, C, 64, mcts_num_read=50, evaluator="external")
    a.set_positions(above)
    plain.set_positions(above)
    a.search(reads)
    plain.search(reads)
    same_roots(a.roots(), plain.roots(), what="above")
    assert a.endgame_stats() == (0, 0)
    ca, cp = a.counters(), plain.counters()
    assert ca["expansions"] == cp["expansions"] and ca["terminal_leaves"] == cp["terminal_leaves"]
    # a leaf below max_free under a root above it stays with the base evaluator: some leaves were that deep
    x = rows_of(R, C, above)
    assert ((x[:, ER.board(R, C)[0]] == 0).sum(axis=1) - 1 <= max_free).any()
    # mixed: even slots start below max_free, odd slots above
    below, _ = starts_below(R, C, max_free)
    mixed = [below[i] if i % 2 == 0 else above[i] for i in range(64)]
    for e in (a, plain, ext):
        e.set_positions(mixed)
    a.search(reads)
    plain.search(reads)
    ext.search_external(restated(R, C, 1, max_free), reads)
    ra = a.roots()
    same_roots(ra, ext.roots(), slice(0, 64, 2), "mixed, below")
    same_roots(ra, plain.roots(), slice(1, 64, 2), "mixed, above")
    assert a.endgame_stats()[0] == 32
    for e in (a, plain, ext):
        e.close()
    g.close()


# ---------------------------------------------------------------- (d) self-play keeps the result; one table per game
def check_selfplay_rows(R, C, max_free, got, stats, n_games):
    g = Endgame(R, C, max_free=max_free)
    sc = score_endgames(got, endgame=g)
    g.close()
    n_free, solved = sc["n_free"].astype(np.int64), sc["solved"]
    assert np.array_equal(solved, n_free <= max_free) and solved.any()
    assert len(np.unique(got["game_idx"])) == n_games
    # single model: every move is searched by it, so a game's first table root is its first row with F <= max_free
    z, value = np.asarray(got["z"]).astype(np.int64), sc["value"].astype(np.int64)
    assert np.array_equal(z[solved], value[solved])
    keep = solved & (value >= 0)
    pi = np.asarray(got["pi"], np.float64).reshape(len(z), -1)
    assert keep.sum() > 100 and (pi[keep].max(axis=1) == 1.0).all() and ((pi[keep] != 0).sum(axis=1) == 1).all()
    assert sc["played_optimal"][keep].all() and (sc["policy_mass"][keep] == 1.0).all()
    assert stats[0] == len(np.unique(np.asarray(got["game_idx"])[solved])) and stats[1] > 0


@pytest.mark.parametrize("R,C,max_free", [(5, 5, 16), (2, 7, 10)])
def test_selfplay_keeps_the_result_and_solves_once_per_game(R, C, max_free):
    from dotsboxesaz_amd.engine import Engine
    g = Endgame(R, C, max_free=max_free)
    e = Engine(R, C, 64, mcts_num_read=24, noise=(0.0, 0.0), temperature={0: 1.0}, reuse_tree=False, evaluator="uniform", endgame=g,
               endgame_seed=3, seed=11)
    e.selfplay_start(128, 0)
    e.run()
    c = e.counters()
    assert c["games_finished"] == 128 and c["error_slots"] == 0
    got, stats = e.fetch_samples(), e.endgame_stats()
    check_selfplay_rows(R, C, max_free, got, stats, 128)
    # start positions that already have F <= max_free: one table per game
    d, rs = O.dims(R, C), np.random.RandomState(R)
    E = 2 * R * C + R + C
    book = [start_with_free(d, rs, E, max_free - i % 4) for i in range(16)]
    e.selfplay_set_start(book, 2)
    e.selfplay_start(128, 0)
    e.run()
    c = e.counters()
    assert c["games_finished"] == 128 and c["error_slots"] == 0
    got2, stats2 = e.fetch_samples(), e.endgame_stats()
    assert stats2[0] - stats[0] == 128
    check_selfplay_rows(R, C, max_free, got2, (128, 1), 128)
    assert np.asarray(check_first_rows(R, C, got2, book)).all()
    e.close()
    g.close()


def check_first_rows(R, C, got, book):
    """z of a game's first row is the true value of its opening for the mover"""
    g = Endgame(R, C)
    first = np.nonzero(got["move_idx"] == 0)[0]
    value = g.score(np.asarray(got["x"])[first].reshape(len(first), g.F))["value"]
    g.close()
    assert len(first) == 128
    return np.asarray(got["z"])[first] == value


# ---------------------------------------------------------------- (e) endgame_reads
def test_endgame_reads_caps_the_driver_rule_for_served_searches_only():
    from dotsboxesaz_amd.engine import Engine
    R, C, max_free = 4, 4, 10
    g = Endgame(R, C, max_free=max_free)
    acts, _ = ER.board(R, C)
    e = Engine(R, C, 16, mcts_num_read=40, temperature={0: 1.0}, reuse_tree=False, evaluator="uniform", endgame=g, endgame_reads=3, seed=21)
    e.selfplay_start(16, 0)
    e.run()
    assert e.counters()["games_finished"] == 16
    got = e.fetch_samples()
    x = np.asarray(got["x"]).reshape(len(got["z"]), -1)
    left = (x[:, acts] == 0).sum(axis=1)
    reads = got["visits"].sum(axis=1)
    moved = got["played"] >= 0
    served = moved & (left <= max_free)
    assert served.sum() >= 16 * 5 and (reads[served] == 3).all()  # the rule gives min(4 * F!, 40) >= 4
    assert (reads[moved & (left > max_free)] == 40).all() and (moved & (left > max_free)).sum() > 16 * 10
    # explicit read counts are never touched; the rule without a count is
    below, _ = starts_below(R, C, max_free)
    e2 = Engine(R, C, 64, mcts_num_read=40, evaluator="uniform", endgame=g, endgame_reads=3)
    e2.set_positions(below)
    e2.search(11)
    assert (e2.roots()["visits"].sum(axis=1) == 11).all()
    e2.set_positions(below)
    e2.search()
    assert (e2.roots()["visits"].sum(axis=1) == 3).all()
    e.close()
    e2.close()
    g.close()


# ---------------------------------------------------------------- (f) K pending
@pytest.mark.parametrize("selfplay_pending", [False, True])
def test_pending_waves_find_the_optimal_move(selfplay_pending):
    from dotsboxesaz_amd.engine import Engine
    R, C, max_free, reads = 4, 4, 16, 50
    starts, _ = starts_below(R, C, max_free)
    x = rows_of(R, C, starts)
    g = Endgame(R, C, max_free=max_free)
    value = g.score(x)["value"].astype(np.int64)
    q = g.score(x)["q"].astype(np.int64)
    e = Engine(R, C, 64, mcts_num_read=reads, evaluator="formula", endgame=g, max_pending_evals=8, selfplay_pending=selfplay_pending)
    e.set_positions(starts)
    e.search(reads)
    r = e.roots()
    assert e.counters()["error_slots"] == 0 and e.endgame_stats()[0] == 64
    e.close()
    g.close()
    assert (r["visits"].sum(axis=1) == reads).all()
    top = r["visits"].argmax(axis=1)
    safe = value >= 0
    # the root's value as the search saw it: the sum of the values backed up into the root, for its mover.  root_tv holds one
    # VIRTUAL_LOSS more: the root expansion's backup adds it without a selection having taken it off (mcts.py:108-109, 127)
    at = np.arange(64)
    seen = r["root_tv"] - 1.0
    assert (r["root_nv"] == reads + 1).all()
    assert safe.sum() >= 16 and (q[at, top] == q.max(axis=1))[safe].all()
    assert np.array_equal(np.sign(seen).astype(np.int64), value)


# ---------------------------------------------------------------- (g) match play
def test_match_model_with_endgame_holds_the_theoretical_result():
    from dotsboxesaz_amd.engine import Engine
    R, C = 4, 4
    d, rs = O.dims(R, C), np.random.RandomState(4)
    book = [start_with_free(d, rs, 40, 16 - i % 6) for i in range(32)]
    g = Endgame(R, C)
    e = Engine(R, C, 64, mcts_num_read=24, temperature={0: 1.0}, reuse_tree=False, match_play=True, evaluator="uniform", evaluator2="uniform",
               endgame=g, endgame_models=(0,), endgame_seed=5, seed=9)
    e.selfplay_set_start(book, 2)
    e.selfplay_start(64, 0)
    e.run()
    c = e.counters()
    assert c["games_finished"] == 64 and c["error_slots"] == 0
    got = e.fetch_samples()
    model = got["player"].astype(np.int64) ^ (got["game_idx"].astype(np.int64) & 1)
    searched = np.unique(got["game_idx"][(model == 0) & (got["played"] >= 0)])
    # one per game in which model 0 came to move: its later roots are subsets of its first
    assert e.endgame_stats()[0] == len(searched) and len(searched) >= 48
    e.close()
    first = np.nonzero(got["move_idx"] == 0)[0]
    assert np.array_equal(got["game_idx"][first], np.arange(64))
    v = g.score(np.asarray(got["x"])[first].reshape(64, g.F))["value"].astype(np.int64)
    g.close()
    moves_first = (got["player"][first].astype(np.int64) ^ (got["game_idx"][first] & 1)) == 0  # model 0 is the opening's mover
    z = got["z"][first].astype(np.int64)
    theory, result = np.where(moves_first, v, -v), np.where(moves_first, z, -z)
    assert moves_first.sum() == 32 and set(theory) >= {-1, 1}
    assert (result >= theory).all(), np.nonzero(result < theory)[0]


# ---------------------------------------------------------------- (h) errors
def test_attach_errors_and_borrowed_handle():
    from dotsboxesaz_amd.engine import Engine
    g = Endgame(3, 3, max_free=8)

    def code(fn):
        with pytest.raises(_lib.DbazError) as ei:
            fn()
        return ei.value.code

    e = Engine(3, 3, 2, mcts_num_read=5, evaluator="formula")
    wrong_board = Endgame(2, 3)
    assert code(lambda: e.attach_endgame(wrong_board)) == _lib.EINVAL
    wrong_board.close()
    assert code(lambda: e.attach_endgame(g, 2)) == _lib.EINVAL
    assert code(lambda: e.attach_endgame(g, 1)) == _lib.EINVAL  # no second model without match play
    assert code(lambda: e.attach_endgame(g, 0, reads=-1)) == _lib.EINVAL
    assert code(lambda: Engine(3, 3, 2, evaluator="external", endgame=g)) == _lib.EINVAL
    assert code(lambda: Engine(3, 3, 2, evaluator="solver", endgame=g)) == _lib.EINVAL
    import torch
    if torch.cuda.device_count() > 1:
        other = Endgame(3, 3, device=1)
        assert code(lambda: e.attach_endgame(other)) == _lib.EINVAL
        other.close()
    assert e.endgame_stats() == (0, 0)  # none of the refused calls attached anything
    d, rs = O.dims(3, 3), np.random.RandomState(8)
    starts = [start_with_free(d, rs, 24, 8), start_with_free(d, rs, 24, 6)]
    e.set_positions(starts)
    e.search(5)
    assert e.endgame_stats() == (0, 0)
    e.attach_endgame(g, 0, seed=2)
    e.set_positions(starts)
    e.search(5)
    assert e.endgame_stats()[0] == 2 and e.endgame_stats()[1] >= 2 and (e.roots()["visits"].sum(axis=1) == 5).all()
    # a later attach must fit the slot regions of the first (256 bytes here): a larger or smaller max_free is refused for either
    # model and changes nothing; the same max_free replaces the solver and drops the tables
    first = e.roots()
    for mf in (16, 9, 7):
        other = Endgame(3, 3, max_free=mf)
        assert code(lambda: e.attach_endgame(other, 0, seed=2)) == _lib.EINVAL, mf
        other.close()
    e.set_positions(starts)
    e.search(5)
    same_roots(first, e.roots(), what="after the refused attaches")
    assert e.endgame_stats()[0] == 4
    again = Endgame(3, 3, max_free=8)
    e.attach_endgame(again, 0, seed=2)
    e.search(5)  # the same positions, searched on: their tables were dropped and are solved again
    assert e.endgame_stats()[0] == 6 and e.counters()["error_slots"] == 0
    e.set_positions(starts)
    e.search(5)
    same_roots(first, e.roots(), what="after the re-attach")
    m = Engine(3, 3, 2, mcts_num_read=5, evaluator="formula", evaluator2="uniform", match_play=True, endgame=g, endgame_models=(0,))
    wide = Endgame(3, 3, max_free=16)
    assert code(lambda: m.attach_endgame(wide, 1)) == _lib.EINVAL  # the other model's handle, another max_free
    m.attach_endgame(again, 1)
    m.close()
    wide.close()
    e.close()  # the handles are borrowed: they outlive the engine
    again.close()
    x, left = case(3, 3)
    got = g.score(x)
    assert np.array_equal(got["solved"], left <= 8)
    g.close()
