"""The row-against-table body that every table kind shares (csrc/table_row.h: closed boxes, the ballot of the drawn compact
edges, Q of the free lanes, the members ballot and their float32 sum, the compact-edge rank of an action slot) on boards that
cross its word and chunk loops, which the 6x6 boards of the other files do not: 9x9 (200 action slots: four ballot words, the
last partial; 81 boxes: two chunks), 7x15 (256 = DBAZ_MAX_A slots: every word full; 105 boxes), 1x1 (8 slots, one box: a lane
set almost empty) -- and 2x2, because the first three have an odd number of boxes, so no row of theirs has value 0.

Rows: test_hip_deep_endgame.random_games, 4 games per board, the rows with at most 12 free edges (the finished and early-ended
ones included), each also with the other player to move.  Every output is compared bit for bit with the numpy references
(endgame_ref.py, endgame_policy_ref.py, targets_ref.py on top of the first): Endgame.score / .policy / .policy_from / .targets,
DeepTables(max_free=12).score / .targets with a table_of that names other games' tables and indices out of range, and
DeepEndgame.policy; Endgame and DeepTables also against each other wherever both apply."""
import numpy as np
import pytest

from dotsboxesaz_amd.endgame import DeepEndgame, DeepTables, Endgame
import endgame_policy_ref as PR
import endgame_ref as ER
import targets_ref as TR
from test_hip_deep_endgame import other_mover, random_games, random_pi, reference

BOARDS = [(9, 9), (7, 15), (1, 1), (2, 2)]
MAX_FREE = 12
N_GAMES = 4

_cases = {}
_endgame = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def case(R, C):
    """per board, built once and left unchanged: dict(x [n, 3HW] -- game after game, per game its rows with F <= 12 deepest first,
    then the same with the other mover --, game [n], roots [4, 3HW] the first such row of each game, k rows per game, pi, z,
    ref = endgame_ref of every row, facts = targets_ref.solve_rows, inside [n, 4]: row r's free edges are a subset of root t's)"""
    if (R, C) not in _cases:
        acts, _ = ER.board(R, C)
        xs, left = random_games(R, C, N_GAMES, seed=100 * R + C)
        per = len(xs) // N_GAMES
        parts, roots = [], []
        for g in range(N_GAMES):
            gx, gl = xs[g * per:(g + 1) * per], left[g * per:(g + 1) * per]
            late = gx[gl <= MAX_FREE]
            assert gl[gl <= MAX_FREE][0] == min(MAX_FREE, len(acts))
            roots.append(late[0])
            parts.append(np.concatenate([late, other_mover(R, C, late)]))
        x = np.concatenate(parts)
        k = len(parts[0])
        n, A = len(x), 2 * (R + 1) * (C + 1)
        rs = np.random.RandomState(R * 31 + C)
        pi = random_pi(n, A, seed=R + C)
        pi[::7] = 0.0  # rows without mass anywhere: "restrict" falls back to uniform
        free = x[:, acts] == 0
        root_free = np.array(roots)[:, acts] == 0
        _cases[(R, C)] = dict(x=x, game=np.repeat(np.arange(N_GAMES), k), roots=np.array(roots), k=k, pi=pi,
                              z=rs.choice([-1.0, 0.0, 1.0], size=n).astype(np.float32), ref=reference(R, C, x, pi),
                              facts=TR.solve_rows(R, C, x, 16), inside=~(free[:, None, :] & ~root_free[None, :, :]).any(axis=2))
    return _cases[(R, C)]


def endgame_outputs(R, C):
    """Endgame's answers to a board's rows, computed once: score, targets per pi_mode"""
    if (R, C) not in _endgame:
        c = case(R, C)
        g = Endgame(R, C)
        _endgame[(R, C)] = dict(score=g.score(c["x"], c["pi"]), targets={m: g.targets(c["x"], c["pi"], c["z"], m, True) for m in ("restrict", "uniform")})
        g.close()
    return _endgame[(R, C)]


def test_the_references_cover_every_value_and_sets_of_several_members():
    """no GPU: what the references alone say about these rows"""
    values, several = set(), 0
    for R, C in BOARDS:
        c = case(R, C)
        values |= set(int(v) for v in c["ref"]["value"])
        several += sum(len(f["O"]) > 1 for f in c["facts"])
        assert c["ref"]["finished"].any() and not c["ref"]["finished"].all() and (c["ref"]["n_free"] <= MAX_FREE).all()
        if (R * C) % 2:  # the last box decides: no draw, no value 0
            assert set(int(v) for v in c["ref"]["value"]) == {-1, 1}
    assert values == {-1, 0, 1} and several >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("R,C", BOARDS)
def test_endgame_rows_equal_the_references(R, C):
    c = case(R, C)
    x, ref = c["x"], c["ref"]
    A = 2 * (R + 1) * (C + 1)
    got = endgame_outputs(R, C)
    s = got["score"]
    assert s["solved"].all()
    for key in ("value", "diff", "q", "n_free"):
        assert np.array_equal(s[key], ref[key]), key
    assert np.array_equal(bits(s["policy_mass"]), bits(ref["policy_mass"]))
    for mode in ("restrict", "uniform"):
        want = TR.apply_targets(c["facts"], c["pi"], c["z"], mode, True)
        pi2, z2, info = got["targets"][mode]
        assert np.array_equal(bits(pi2), bits(want["pi"])) and np.array_equal(bits(z2), bits(want["z"])), mode
        assert np.array_equal(bits(info["mass"]), bits(want["mass"])) and np.array_equal(info["relabelled"], want["relabelled"] != 0)
        assert np.array_equal(info["n_free"], want["n_free"]) and want["relabelled"].any() and not want["relabelled"].all()
    g = Endgame(R, C)
    for seed in (0, 7):
        wp, wv, ws = PR.policy(R, C, x, seed, 16)
        p, v, solved = g.policy(x, seed)
        assert ws.all() and solved.all() and np.array_equal(bits(p), bits(wp)) and np.array_equal(bits(v), bits(wv)), seed
        # the table path: one table per game's root, the game's rows answered from it
        fp, fv = g.policy_from(c["roots"], x.reshape(N_GAMES, c["k"], -1), seed)
        assert np.array_equal(bits(fp), bits(wp.reshape(N_GAMES, c["k"], A))) and np.array_equal(bits(fv), bits(wv.reshape(N_GAMES, c["k"]))), seed
    g.close()


def table_of_for(c):
    """each row's own game, except: every 5th row names the next game's table, and three rows an index out of range"""
    t = c["game"].astype(np.int32).copy()
    t[::5] = (t[::5] + 1) % N_GAMES
    t[1], t[len(t) // 2], t[-2] = -1, N_GAMES, 1 << 20
    ok = (t >= 0) & (t < N_GAMES)
    served = ok & c["inside"][np.arange(len(t)), np.where(ok, t, 0)]
    return t, served


@pytest.mark.gpu
@pytest.mark.parametrize("R,C", BOARDS)
def test_deep_tables_rows_equal_the_references_and_endgame(R, C):
    c = case(R, C)
    x, ref, n = c["x"], c["ref"], len(c["x"])
    t, served = table_of_for(c)
    assert served.sum() >= n // 2 and (~served).sum() >= 3
    pool = DeepTables(R, C, max_free=MAX_FREE, n_tables=N_GAMES).solve(c["roots"])
    assert np.array_equal(pool.n_free, [min(MAX_FREE, 2 * R * C + R + C)] * N_GAMES)
    s = pool.score(x, t, c["pi"])
    e = endgame_outputs(R, C)
    assert np.array_equal(s["solved"], served) and np.array_equal(s["n_free"], ref["n_free"])
    for key in ("value", "diff", "q"):
        assert np.array_equal(s[key][served], ref[key][served]), key
        assert np.array_equal(s[key][served], e["score"][key][served]), key
    assert np.array_equal(bits(s["policy_mass"][served]), bits(ref["policy_mass"][served]))
    assert np.array_equal(bits(s["policy_mass"][served]), bits(e["score"]["policy_mass"][served]))
    out = ~served
    assert not s["value"][out].any() and (s["diff"][out] == -128).all() and (s["q"][out] == -128).all() and not s["policy_mass"][out].any()
    facts = [dict(f, touched=f["touched"] and bool(ok)) for f, ok in zip(c["facts"], served)]
    for mode in ("restrict", "uniform"):
        want = TR.apply_targets(facts, c["pi"], c["z"], mode, True)
        pi2, z2, info = pool.targets(x, t, c["pi"], c["z"], mode, True)
        assert np.array_equal(bits(pi2), bits(want["pi"])) and np.array_equal(bits(z2), bits(want["z"])), mode
        assert np.array_equal(bits(info["mass"]), bits(want["mass"])) and np.array_equal(info["relabelled"], want["relabelled"] != 0)
        assert np.array_equal(info["n_free"], want["n_free"])
        epi, ez, einfo = e["targets"][mode]
        assert np.array_equal(bits(pi2[served]), bits(epi[served])) and np.array_equal(bits(z2[served]), bits(ez[served])), mode
        assert np.array_equal(bits(info["mass"][served]), bits(einfo["mass"][served]))
    pool.close()


@pytest.mark.gpu
@pytest.mark.parametrize("R,C", BOARDS)
def test_deep_endgame_policy_equals_the_reference(R, C):
    c = case(R, C)
    x = c["x"]
    d = DeepEndgame(R, C, max_free=MAX_FREE)
    unfinished = [g for g in range(N_GAMES) if not c["ref"]["finished"][c["game"] == g].all()]  # a 9x9 game may end before F = 12
    for game, seed in ((unfinished[0], 0), (unfinished[-1], 7)):
        served = c["inside"][:, game]
        wp, wv, _ = PR.policy(R, C, x, seed, 16)
        wp[~served], wv[~served] = 0.0, 0.0
        p, v, got = d.solve(c["roots"][game]).policy(x, seed)
        assert np.array_equal(got, served) and served[c["game"] == game].all()
        assert np.array_equal(bits(p), bits(wp)) and np.array_equal(bits(v), bits(wv)), (game, seed)
        assert (wp.sum(axis=1) == 1).any() and set(wv[served]) >= {-1.0, 1.0}
    d.close()
