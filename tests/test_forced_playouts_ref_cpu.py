"""tests/forced_playouts_ref.py, the CPU restatement of forced playouts and policy target pruning, checked on its own (no GPU):

* with k = 0 its Python search is the oracle's Tree.search + advance bit for bit (visits, W bit patterns, root priors, TreeStats,
  q) over whole games -- without this the device comparison in test_hip_forced_playouts.py would prove nothing;
* prune() keeps the properties the rule promises on every root of those games at k = 2, and the library's host entry point
  dbaz_prune_visits (no device) gives the same visits on every one of them;
* six deliberate mistakes each change the rows of at least 4 of 8 games, and forcing changes the raw visits of at least 6 of 8.

The seeds of the last two were picked on the CPU so that the right helper against itself differs in 0 of 8 games."""
import numpy as np
import pytest

from oracle import oracle as O
import endgame_selfplay_ref as ESR
import forced_playouts_ref as FR

NOISE = (0.8, 0.25)
K = 2.0
CAP = (0.5, 8)
SEED = 7  # games 0..7 of this seed: see the module docstring


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _vector(rs, valid, noise):
    return rs.dirichlet(np.where(valid, 1.0, 1e-60) * noise[0]) if noise[0] > 0 else None


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("R,C", [(3, 3), (2, 3), (4, 4)])
def test_k0_is_the_oracle_bit_for_bit(R, C, kind):
    """whole games, 8 seeds each: 16 and 48 reads, noise (0.8, 0.25) with scripted vectors and none, tree reuse on and off"""
    d = O.dims(R, C)
    n_roots = 0
    for sims in (16, 48):
        for noise in (NOISE, (0.0, 0.0)):
            for reuse in (True, False):
                for seed in range(8):
                    rs = np.random.RandomState(100 * seed + sims)
                    t, o = FR.Tree(d, O.new_state(d)), O.Tree(d, O.new_state(d))
                    ev = O.Evaluator(kind)
                    while not t.is_terminal:
                        assert not o.is_terminal and t.is_expanded == o.is_expanded
                        valid = t.first.valid
                        reads = ESR._fact_reads(int(valid.sum()), sims)
                        vec = _vector(rs, valid, noise)
                        a = t.search(reads, FR.formula(kind), dirichlet=noise, noise=vec)
                        b = o.search(reads, ev, dirichlet=noise, noise=vec)
                        where = (R, C, kind, sims, noise, reuse, seed, n_roots)
                        assert np.array_equal(a, b), where
                        for x, y in zip(t.root_arrays(), o.root_arrays()):  # priors f64, W f32, visits, player_changed
                            assert x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y)), where
                        sa, sb = t.stats(), o.stats()
                        assert sa[:3] == sb[:3] and np.float32(sa[3]).tobytes() == np.float32(sb[3]).tobytes(), where
                        assert (np.float32(t.tv_none).tobytes(), t.nv_none) == (np.float32(o.root_slot()[0]).tobytes(), o.root_slot()[1])
                        mv = int(rs.choice(len(a), p=a / a.sum()))
                        t.advance(mv, reuse)
                        o.advance(mv, reuse)
                        n_roots += 1
                    assert o.is_terminal
    assert n_roots > 8 * 8 * 6


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("R,C", [(3, 3), (2, 3), (4, 4)])
def test_prune_properties_and_the_library_entry_point(R, C, kind):
    """every root of the same games played with k = 2: c* untouched, 0 <= n' <= n, n' >= n - f or n' = 0 by the single-playout
    clause, k = 0 is the identity, and dbaz_prune_visits (host only) equals the Python prune()"""
    from dotsboxesaz_amd import forced_playouts as FP
    d = O.dims(R, C)
    seen = dict(roots=0, cut=0, single=0)

    def on_root(t, full, active):
        got, a = FR.prune_root(t, K)
        n, P, valid = a["n"], a["P"], a["valid"]
        cand = np.nonzero(valid)[0]
        cs = cand[np.argmax(n[cand])]  # argmax: the first maximum
        assert got[cs] == n[cs] and got[cs] == n.max() and got.sum() > 0
        assert ((0 <= got) & (got <= n)).all() and np.array_equal(got[~valid], n[~valid])
        for c in np.nonzero(got < n)[0]:
            f = FR.forced_count(K, P[c], a["root_N"])
            assert float(f) * float(f) >= K * P[c] * a["root_N"] and (f == 0 or float(f - 1) * float(f - 1) < K * P[c] * a["root_N"])
            assert got[c] >= n[c] - f or (got[c] == 0 and n[c] - f <= 1), (c, got[c], n[c], f)
            assert got[c] != 1
            seen["single"] += int(got[c] == 0 and n[c] - f == 1)
        assert np.array_equal(FR.prune_root(t, 0.0)[0], n)
        lib = FP.prune_visits(**a)
        assert lib.dtype == np.int32 and np.array_equal(lib, got), (a, lib, got)
        a0 = dict(a, k=0.0)
        assert np.array_equal(FP.prune_visits(**a0), n)
        seen["roots"] += 1
        seen["cut"] += int((got < n).any())

    for sims in (16, 48):
        for noise in (NOISE, (0.0, 0.0)):
            for reuse in (True, False):
                for seed in range(8):
                    FR.generate_game(d, np.random.RandomState(100 * seed + sims), seed=seed, game_idx=seed, sims=sims, reuse=reuse,
                                     noise=noise, base_ev=kind, forced_playouts=(K, True), on_root=on_root)
    print("%dx%d kind %d: %d roots, pruning cut visits at %d, the single-playout clause at %d" % (R, C, kind, seen["roots"], seen["cut"],
                                                                                              seen["single"]))
    assert seen["roots"] > 8 * 8 * 6 and seen["cut"] > seen["roots"] // 20


def test_prune_visits_refuses_bad_arguments():
    from dotsboxesaz_amd import forced_playouts as FP
    A = 8
    ok = dict(k=2.0, pbc=1.25, sq=3.0, root_N=9, P=np.full(A, 1.0 / A), W=np.zeros(A, np.float32), n=np.arange(A), same=np.zeros(A, bool),
              valid=np.ones(A, bool))
    assert FP.prune_visits(**ok).shape == (A,)
    for bad in (dict(k=-1.0), dict(k=17.0), dict(k=float("nan")), dict(root_N=-1), dict(n=np.arange(A - 1))):
        with pytest.raises(ValueError):
            FP.prune_visits(**dict(ok, **bad))


def gen(game, *, forced_playouts, cap=None, mistake=None, reuse=True):
    d = O.dims(3, 3)
    return FR.generate_game(d, np.random.RandomState(1000 * SEED + game), seed=SEED, game_idx=game, sims=48, reuse=reuse, noise=NOISE, cap=cap,
                            forced_playouts=forced_playouts, mistake=mistake)


@pytest.mark.parametrize("mistake", FR.MISTAKES)
def test_a_deliberate_mistake_changes_half_the_games(mistake):
    """8 generated 3x3 games (48 reads, noise on, k = 2, pruning on), replayed with the mistake: the right replay differs in 0 of
    8, the wrong one in at least 4.  "forced_on_fast" runs under the playout cap (0.5, 8), where there are fast searches to get
    it wrong on; "prune_before_move_choice" cannot show in a teacher-forced replay, so there the game is generated again from the
    same random stream with the mistake in."""
    d = O.dims(3, 3)
    cap = CAP if mistake == "forced_on_fast" else None
    kw = dict(seed=SEED, sims=48, reuse=True, noise=NOISE, cap=cap, forced_playouts=(K, True))
    changed = 0
    for game in range(8):
        g = gen(game, forced_playouts=(K, True), cap=cap)
        assert FR.rows_differ(FR.replay_game(d, g["played"], g["vectors"], game_idx=game, **kw), g) == -1
        if mistake == "prune_before_move_choice":
            wrong = gen(game, forced_playouts=(K, True), cap=cap, mistake=mistake)
        else:
            wrong = FR.replay_game(d, g["played"], g["vectors"], game_idx=game, mistake=mistake, **kw)
        changed += FR.rows_differ(wrong, g) >= 0
    print("%s: %d of 8 games differ" % (mistake, changed))
    assert changed >= 4


def test_forcing_changes_the_raw_visits():
    """k = 2 against k = 0 on the same moves and vectors: the raw visits differ in at least 6 of 8 games"""
    d = O.dims(3, 3)
    changed = 0
    for game in range(8):
        g = gen(game, forced_playouts=(K, False))
        assert not g["pruned"].any() and np.array_equal(g["visits"], g["raw_visits"])
        off = FR.replay_game(d, g["played"], g["vectors"], seed=SEED, game_idx=game, sims=48, reuse=True, noise=NOISE, forced_playouts=None)
        changed += not np.array_equal(off["raw_visits"], g["raw_visits"])
    print("forcing: %d of 8 games differ" % changed)
    assert changed >= 6


def test_pruning_leaves_the_game_alone():
    """prune on and off: the same moves, raw visits, q and TreeStats; the recorded visits only ever lose"""
    for game in range(4):
        a, b = gen(game, forced_playouts=(K, False)), gen(game, forced_playouts=(K, True))
        assert np.array_equal(a["played"], b["played"]) and np.array_equal(a["raw_visits"], b["raw_visits"])
        for key in ("q_value", "max_deepness", "tree_size", "terminal_count", "z"):
            assert np.array_equal(a[key], b[key])
        assert (b["visits"] <= a["visits"]).all() and b["pruned"].all() and (b["visits"].sum(axis=1) > 0).all()
        assert b["visits_pruned"] == int(a["visits"].sum() - b["visits"].sum()) and b["rows_pruned"] == b["n_rows"]


def test_header_with_gpp_under_sanitizers(tmp_path):
    """csrc/forced_playouts.h is plain C++: tests/forced_playouts_main.cpp built with g++ for the host alone under AddressSanitizer
    and UBSan (no device code, no GPU, no preload), against the Python prune(), forced() and forced_count() on the roots of four
    3x3 games, at k = 2 and at k = 0.5"""
    import os
    import subprocess
    from conftest import REPO
    exe = tmp_path / "forced_playouts"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "dotsboxesaz_amd", "csrc"), os.path.join(REPO, "tests", "forced_playouts_main.cpp"), "-o", str(exe)],
                   check=True)
    roots = []
    for k in (K, 0.5):
        for game in range(4):
            FR.generate_game(O.dims(3, 3), np.random.RandomState(game), seed=SEED, game_idx=game, sims=48, reuse=True, noise=NOISE,
                             forced_playouts=(k, True), on_root=lambda t, full, active, k=k: roots.append((FR.prune_root(t, k), k)))
    text = []
    for (_, a), k in roots:
        text.append("%d %s %s %s %d" % (len(a["n"]), float(k).hex(), float(a["pbc"]).hex(), float(a["sq"]).hex(), a["root_N"]))
        for i in range(len(a["n"])):
            text.append("%s %s %d %d" % (float(a["P"][i]).hex(), float(a["W"][i]).hex(), int(a["n"][i]) | (0x40000000 if a["same"][i] else 0), a["valid"][i]))
    r = subprocess.run([str(exe)], input="\n".join(text) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)  # a sanitizer report has a message
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(roots) > 80
    for line, ((want, a), k) in zip(lines, roots):
        got = np.array(line.split(), dtype=np.int64)
        A = len(a["n"])
        assert np.array_equal(got[:A], want), (a, got[:A], want)
        assert np.array_equal(got[A::2].astype(bool), FR.forced(k, a["P"], a["n"], a["root_N"]))
        assert list(got[A + 1::2]) == [FR.forced_count(k, p, a["root_N"]) for p in a["P"]]
