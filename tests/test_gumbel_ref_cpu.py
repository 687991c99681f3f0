"""tests/gumbel_ref.py, the CPU restatement of the Gumbel root search, checked on its own (no GPU):

* with m = 0 it is forced_playouts_ref at k = 0 bit for bit -- which test_forced_playouts_ref_cpu.py pins to the oracle;
* considered() equals mctx's generator of considered visits (restated here from the paper's appendix) for every m' in 1 .. 32
  and R in 1 .. 200, and so do the library's host entry point (no device) and csrc/gumbel.h built with g++;
* every candidate's final n_s matches the phase budgets, and without tree reuse the m' first simulations visit the m' largest gl;
* six deliberate mistakes each change at least one row of the case table;
* the library's dbaz_gumbel_target and the g++ build of the header give the reference's visits within +-1 count per entry (libm's
  exp and log are not correctly rounded);
* the gap condition: over every decision of every case of CASES -- the table test_hip_gumbel.py plays -- the best score is more
  than 1e-9 above the second, so a last-bit difference between device and host log changes no decision.  The seeds were picked
  here so that this holds;
* the game loop's new arguments (table=, endgame_reads=, served_from=, a LeafSolver as the evaluator) at their defaults change no
  byte of the existing cases;
* the cases of FEATURES -- the table test_hip_gumbel_features.py plays -- keep the gap condition and reach what they are there for
  (a served root with m' > 1, R < m', solved leaves under high roots and right below a Gumbel root, first rows at ply 0 of a
  start position), the six mistakes still show on them, and so do the mistakes only they can show: R not capped by endgame_reads,
  an ignored cap, no table, a zero-prior candidate, the ply counted from the empty board;
* zero priors: the three kinds of root with a formula evaluator whose priors are zeroed on half of the actions, and with the torch
  forward pass of test_hip_gumbel_net.py's network, which also tells which network seeds leave the gap condition room."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
import forced_playouts_ref as FR
import gumbel_ref as GR

SMALL = [c for c in GR.CASE_IDS if c.startswith("3x3")]


def mctx_sequence(max_num_considered_actions, num_simulations):
    """get_sequence_of_considered_visits of the paper's reference implementation"""
    if max_num_considered_actions <= 1:
        return tuple(range(num_simulations))
    log2max = int(math.ceil(math.log2(max_num_considered_actions)))
    sequence = []
    visits = [0] * max_num_considered_actions
    num_considered = max_num_considered_actions
    while len(sequence) < num_simulations:
        num_extra_visits = max(1, int(num_simulations / (log2max * num_considered)))
        for _ in range(num_extra_visits):
            sequence.extend(visits[:num_considered])
            for i in range(num_considered):
                visits[i] += 1
        num_considered = max(2, num_considered // 2)
    return tuple(sequence[:num_simulations])


def test_considered_is_mctx_and_the_library_agrees():
    """fails on a library without the feature: the symbol is missing"""
    from dotsboxesaz_amd import gumbel as G
    for m in range(1, 33):
        for R in range(1, 201):
            want = mctx_sequence(m, R)
            assert tuple(GR.considered(m, R, t) for t in range(R)) == want, (m, R)
            assert tuple(G.considered_visits(m, R)) == want, (m, R)
    assert len(G.considered_visits(4, 0)) == 0
    for bad in ((-1, 4), (257, 4), (4, -1)):
        with pytest.raises(ValueError):
            G.considered_visits(*bad)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("reuse", [True, False])
def test_m0_is_the_forced_reference_at_k0(kind, reuse):
    d = O.dims(3, 3)
    for game in range(4):
        kw = dict(seed=GR.SEED, game_idx=game, sims=32, reuse=reuse, noise=GR.NOISE, cap=(0.5, 8), base_ev=kind)
        a = FR.generate_game(d, np.random.RandomState(game), forced_playouts=None, **kw)
        rs = np.random.RandomState(game)
        b = GR._run(d, gumbel=(0, 0.0, 0.0), choose=lambda i, vis: rs.choice(len(vis), p=vis / vis.sum()),
                    vectors=FR.PCR.dirichlet_vectors(rs, GR.NOISE[0]), **kw)
        assert a["n_rows"] == b["n_rows"] and a["n_search"] == b["n_search"]
        for key in ("x", "player", "visits", "pi", "q_value", "max_deepness", "tree_size", "terminal_count", "played", "reads", "full", "z", "vectors"):
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (game, key)
        assert np.array_equal(b["flags"], np.where(b["full"], 0, 1))


def phase_budgets(m_eff, R):
    """the sorted final visit counts of m' candidates that are visited by the sequence: at each t one candidate at cv visits gets one"""
    cnt = [0] * max(m_eff, 1)
    for t in range(R):
        cv = GR.considered(m_eff, R, t)
        cnt[cnt.index(cv)] += 1
    return sorted(cnt)


@pytest.mark.parametrize("name", SMALL)
def test_phase_budgets_and_the_first_round(name):
    _, R, C, sims, m, reuse, cap, g_mode, ev, _, c_visit, c_scale = GR.case(name)
    d = O.dims(R, C)
    seen = []

    def on_root(t, info, reads, full):
        ns = info["ns"]
        cand = info["C"]
        top = sorted((int(ns[a]) for a in cand), reverse=True)[:max(info["m_eff"], 1)]
        assert sorted(top) == phase_budgets(info["m_eff"], reads), (name, len(seen))
        assert int(ns.sum()) == reads and all(ns[a] == 0 for a in range(d.A) if a not in cand)
        if not reuse:
            # every child starts unvisited with the same completed Q: the first round goes down the gl
            k = min(info["m_eff"], reads)
            by_gl = sorted(cand, key=lambda a: (-info["gl"][a], a))[:k]
            assert info["order"][:k] == by_gl, (name, len(seen))
            assert not info["n0"].any()
        seen.append((info["m_eff"], reuse and bool(info["n0"].any())))

    for gi in range(4):
        GR.play_game(d, g_mode=g_mode, game_idx=gi, seed=GR.SEED, sims=sims, reuse=reuse, gumbel=(m, c_visit, c_scale), cap=cap,
                     base_ev=GR.KIND[ev], on_root=on_root)
    assert len(seen) > 60 and any(me < m for me, _ in seen)  # m > |C| late in a game
    assert not reuse or any(r for _, r in seen)  # n0 is non-zero under tree reuse: n and n_s part


@pytest.mark.parametrize("mistake", GR.MISTAKES)
def test_every_mistake_changes_a_row(mistake):
    changed = 0
    for name in SMALL:
        for a, b in zip(GR.case_games(name, None, 4), GR.case_games(name, mistake, 4)):
            same = a["n_rows"] == b["n_rows"] and all(np.array_equal(a[k], b[k]) for k in ("visits", "played", "q_value", "tree_size", "z"))
            changed += 0 if same else 1
    assert changed >= 1, mistake


@pytest.mark.parametrize("name", GR.CASE_IDS)
def test_gap_condition(name):
    games = GR.case_games(name)
    gap = min(g["min_gap"] for g in games)
    print(name, "minimum gap", gap)
    assert gap > 1e-9
    for g in games:
        v = g["visits"]
        assert (v >= 0).all() and (np.abs(v.sum(axis=1) - (1 << 24)) <= v.shape[1]).all()
        assert np.array_equal(g["flags"], np.where(g["full"], 4, 5))


# ---------------------------------------------------------------- tables, a leaf solver, start positions, zero priors
ROW_KEYS = ("x", "player", "visits", "pi", "q_value", "max_deepness", "tree_size", "terminal_count", "played", "reads", "full", "served", "flags", "z",
            "vectors")


def same_game(a, b, keys=("visits", "played", "q_value", "tree_size", "z")):
    return a["n_rows"] == b["n_rows"] and all(np.array_equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("name", ["3x3-script-m4", "3x3-philox-m2-cap"])
def test_the_new_arguments_at_their_defaults_change_nothing(name):
    """table=None, endgame_reads=0, served_from=None: the game loop as it was, written out here without the new arguments"""
    _, R, C, sims, m, reuse, cap, g_mode, ev, _, c_visit, c_scale = GR.case(name)
    d = O.dims(R, C)
    for gi, want in enumerate(GR.case_games(name, None, 4)):
        gv = GR.gumbel_vectors(np.random.RandomState(1000 + gi)) if g_mode == "script" else None
        t = GR.Tree(d, O.new_state(d))
        gaps, i = [], 0
        while not t.is_terminal:
            valid = t.first.valid
            reads = GR.ESR._fact_reads(int(valid.sum()), sims)
            full = cap is None or GR.PCR.is_full(GR.SEED, gi, i, cap[0])
            reads = reads if full else min(reads, cap[1])
            g = np.asarray(gv(i, valid)) if gv else np.array([GR.philox_g(GR.SEED, gi, i, a) for a in range(d.A)])
            move, vis, _ = t.gsearch(reads, FR.formula(GR.KIND[ev]), m, c_visit, c_scale, g, gaps)
            q = t.stats()[3]
            assert move == want["played"][i] and vis.tobytes() == want["visits"][i].tobytes() and reads == want["reads"][i]
            assert np.float32(q).tobytes() == np.float32(want["q_value"][i]).tobytes() and not want["served"][i]
            t.advance(move, reuse)
            i += 1
        assert i == want["n_rows"] and min(gaps) == want["min_gap"] and want["n_tied_roots"] == 0
        again = GR.play_game(d, g_mode=g_mode, game_idx=gi, seed=GR.SEED, sims=sims, reuse=reuse, gumbel=(m, c_visit, c_scale), cap=cap,
                             base_ev=GR.KIND[ev], table=None, endgame_reads=0, served_from=None)
        for key in ROW_KEYS:
            assert again[key].dtype == want[key].dtype and again[key].tobytes() == want[key].tobytes(), (gi, key)


@pytest.mark.parametrize("name", GR.FEATURE_IDS)
def test_feature_cases_gap_and_reach(name):
    """the gap condition of every case test_hip_gumbel_features.py plays, and that the case reaches what it is there for"""
    f = GR.FEATURES[name]
    games, w = GR.feature_games(name)
    gap = min(g["min_gap"] for g in games.values())
    print(name, "minimum gap", gap)
    assert gap >= 1e-9 and sum(g["n_tied_roots"] for g in games.values()) == 0
    d = O.dims(f["R"], f["C"])
    if "table" in f:
        rows = {k: np.concatenate([g[k] for g in games.values()]) for k in ("served", "m_eff", "R", "n_free", "n0_any", "reads")}
        assert np.array_equal(rows["served"], rows["n_free"] <= f["table"])
        # a served root that another evaluator's leaf expanded earlier keeps that prior under tree reuse: m' > 1
        assert (rows["served"] & (rows["m_eff"] > 1) & rows["n0_any"]).any()
        assert all(g["served"].any() and not g["served"].all() for g in games.values())  # served and unserved rows in one game
        assert sum(g["table_calls"] for g in games.values()) > 0 and sum(g["base_calls"] for g in games.values()) > 0
        short = rows["served"] & (rows["R"] < rows["m_eff"])  # considered() with extra clamped to 1 from the first phase on
        assert short.any() == (0 < f["endgame_reads"] < 8)
        if f["endgame_reads"]:
            assert (rows["reads"][rows["served"]] <= f["endgame_reads"]).all() and (rows["reads"][~rows["served"]] > f["endgame_reads"]).all()
    if "leaf" in f:
        assert sum(w.solved_under_high_roots()) > 0 and w.calls["base"] > 0
        # a solved leaf as a direct child of a Gumbel root: a visited, unfinished child with F <= L under a root with F = L + 1
        direct = []

        def on_root(t, info, reads, full):
            r = t.first
            if int(r.valid.sum()) == f["leaf"] + 1:
                direct.extend(a for a, c in r.children.items() if c.expanded and not c.terminal and info["ns"][a] > 0)

        w2 = GR.LSR.LeafSolver(f["R"], f["C"], f["leaf"], GR.TABLE_SEED, 0)
        for gi in range(2):
            g = GR.play_game(d, g_mode=f["g"], game_idx=gi, seed=GR.SEED, sims=f["sims"], reuse=f["reuse"], gumbel=(f["m"], GR.C_VISIT, GR.C_SCALE),
                             base_ev=w2, on_root=on_root)
            assert same_game(g, games[gi])
        assert len(direct) > 0
    if "starts" in f:
        # the engine's convention (test_hip_selfplay_start.py, Engine.selfplay_set_start): move_idx, scripts and every per-ply stream
        # count plies from the START POSITION -- the first row of a game has move_idx 0 (and move -1) whatever its opening's length
        book = GR.feature_book(name)
        assert sorted(len(b) for b in book) == sorted(f["starts"]) and len({tuple(b) for b in book}) == 3
        used = set()
        for gi, g in games.items():
            si = GR.start_of(gi, 3, 2)
            used.add(si)
            assert np.array_equal(g["x"][0], O.features(d, O.state_from_moves(d, book[si])).ravel())
            if f["g"] == "philox":  # row 0's g is the stream's ply 0
                assert g["vectors"][0][5] == GR.philox_g(GR.SEED, gi, 0, 5) != GR.philox_g(GR.SEED, gi, len(book[si]), 5)
        assert used == {0, 1, 2}


def changed_games(name, **kw):
    right, _ = GR.feature_games(name)
    wrong, _ = GR.feature_games(name, **kw)
    return sum(0 if same_game(right[gi], wrong[gi]) else 1 for gi in wrong)


@pytest.mark.parametrize("mistake", GR.MISTAKES)
def test_every_mistake_changes_a_row_of_a_feature_case(mistake):
    assert sum(changed_games(name, mistake=mistake, n_games=4) for name in ("3x3-table-reads3", "3x3-leaf", "3x3-start-philox")) >= 1, mistake


def test_table_case_needs_the_table_and_the_cap():
    """a reference that ignores endgame_reads, one that treats every root as unserved, and one that keeps the uncapped reads as the
    R of the halving (what begin_search would store before the cap) each differ from the right one"""
    assert changed_games("3x3-table-reads3", endgame_reads=0) >= 1
    assert changed_games("3x3-table-reads3", table=False) >= 1 and changed_games("3x3-table", table=False) >= 1
    # considered(m', R, t) does not depend on R while t < 3, so the cap of 3 cannot show which R is kept; the cap of 12 does
    assert changed_games("3x3-table-reads3", mistake="R_uncapped") == 0 and changed_games("3x3-table-reads12", mistake="R_uncapped") >= 1
    assert changed_games("3x3-table", mistake="R_uncapped") == 0  # without a cap there is nothing to get wrong
    late = changed_games("3x3-table", served_from=((0, 1 << 30), (1, 1 << 30)))  # a game that a dry pool never serves
    assert late == 2


def test_start_case_needs_the_ply_from_the_start_position():
    assert changed_games("3x3-start-philox", mistake="ply_from_empty_board") >= 1
    assert changed_games("6x6-start-script", mistake="ply_from_empty_board") == 0  # scripted g: the stream is not read


# ---- zero priors: a formula evaluator with the priors of a fixed half of the actions set to 0 (a network's softmax can do that)
ZERO = tuple(range(0, 32, 2))


def zeroed(d, st):
    p, v = O.eval_formula(d, st, 0)
    p = np.array(p, np.float32)
    p[list(ZERO)] = 0.0
    return p, v


def zero_prior_games(mistake=None, n_games=4, ev=zeroed, game_idxs=None):
    d = O.dims(3, 3)
    return [GR.play_recording_roots(d, g_mode="philox", game_idx=gi, seed=GR.SEED, sims=32, reuse=True, gumbel=(16, GR.C_VISIT, GR.C_SCALE),
                                    base_ev=ev, mistake=mistake) for gi in (game_idxs or range(n_games))]


def test_zero_priors_three_kinds_of_root():
    """roots with both kinds of valid child, roots without a positive prior, and the change from one to the other inside a game"""
    played = zero_prior_games()
    kinds = [GR.zero_prior_roots(g, roots, ZERO) for g, roots in played]
    assert sum(k[0] for k in kinds) > 0 and sum(k[1] for k in kinds) > 0 and any(k[2] for k in kinds)
    assert min(g["min_gap"] for g, _ in played) >= 1e-9
    wrong = zero_prior_games("zero_prior_candidate")
    assert sum(0 if same_game(a[0], b[0]) else 1 for a, b in zip(played, wrong)) >= 1


# ---- the network cases of test_hip_gumbel_net.py, with the torch model in the engine's place: which seeds have room
@pytest.mark.parametrize("R,C", sorted(GR.NET))
def test_network_seeds_have_room(R, C):
    """the GPU test's own assertion is the one that counts: the engine's network differs from torch's in the last bits, so its games
    may part from these.  Here the same games with the torch forward pass as the evaluator keep every decision 1e-9 off a tie."""
    ev = GR.torch_evaluator(GR.network(R, C), R, C)
    n = GR.NET[(R, C)]
    d = O.dims(R, C)
    games = [GR.play_game(d, g_mode="philox", game_idx=gi, seed=GR.SEED, sims=n["sims"], reuse=True, gumbel=(16, GR.C_VISIT, GR.C_SCALE), base_ev=ev)
             for gi in n["replay"][:1 if R > 3 else 4]]
    gap = min(g["min_gap"] for g in games)
    print("%dx%d network, torch evaluator: minimum gap %g" % (R, C, gap))
    assert gap >= 1e-9


def test_zero_prior_network_reaches_the_three_kinds_of_root():
    ev = GR.torch_evaluator(GR.network(3, 3, zero=True), 3, 3)
    d = O.dims(3, 3)
    p, _ = ev(d, O.new_state(d))
    assert (p[list(GR.NET_ZERO)] == 0).all() and (np.delete(p, list(GR.NET_ZERO)) > 0).all()
    played = zero_prior_games(ev=ev, game_idxs=GR.NET_ZERO_REPLAY)
    kinds = [GR.zero_prior_roots(g, roots, GR.NET_ZERO) for g, roots in played]
    print("zero-prior network, torch evaluator: (mixed, tied, change) per game", kinds, "minimum gap", min(g["min_gap"] for g, _ in played))
    assert sum(k[0] for k in kinds) > 0 and sum(k[1] for k in kinds) > 0 and any(k[2] for k in kinds)
    assert min(g["min_gap"] for g, _ in played) >= 1e-9


def roots_of(name, n_games):
    """(c_visit, c_scale, P, W, n, same, valid, the reference's visits) of every root of a case's first games"""
    _, R, C, sims, m, reuse, cap, g_mode, ev, _, c_visit, c_scale = GR.case(name)
    d = O.dims(R, C)
    roots = []

    def on_root(t, info, reads, full):
        P, W, n, sgn = t.root_arrays()
        valid = t.first.valid.copy()
        roots.append((c_visit, c_scale, P, W, n, sgn > 0, valid, GR.target(c_visit, c_scale, P, W, n, sgn, valid)))

    for gi in range(n_games):
        GR.play_game(d, g_mode=g_mode, game_idx=gi, seed=GR.SEED, sims=sims, reuse=reuse, gumbel=(m, c_visit, c_scale), cap=cap,
                     base_ev=GR.KIND[ev], on_root=on_root)
    return roots


def test_library_target_against_the_reference():
    """fails on a library without the feature: the symbol is missing"""
    from dotsboxesaz_amd import gumbel as G
    roots = roots_of("3x3-script-m4", 4) + roots_of("6x6-philox-m16", 1)
    assert len(roots) > 120
    worst = 0
    for cv, cs, P, W, n, same, valid, want in roots:
        got = G.target(cv, cs, P, W, n, same, valid)
        worst = max(worst, int(np.abs(got.astype(np.int64) - want).max()))
        assert not got[~valid].any()
    print("largest difference in counts", worst)
    assert worst <= 1
    # one valid child: a one-hot target
    P = np.zeros(24)
    P[5] = 1.0
    valid = np.zeros(24, bool)
    valid[[5, 7]] = True
    got = G.target(50.0, 1.0, P, np.zeros(24, np.float32), np.zeros(24, np.int64), np.zeros(24, bool), valid)
    assert got[5] == 1 << 24 and got.sum() == 1 << 24
    for bad in (dict(c_visit=-1.0), dict(c_visit=float("nan")), dict(c_scale=0.0), dict(c_scale=2e3), dict(c_visit=2e6)):
        kw = dict(c_visit=50.0, c_scale=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            G.target(kw["c_visit"], kw["c_scale"], P, np.zeros(24, np.float32), np.zeros(24, np.int64), np.zeros(24, bool), valid)


@pytest.mark.parametrize("sanitize", [False, True])
def test_header_with_gpp(tmp_path, sanitize):
    """csrc/gumbel.h is plain C++: tests/gumbel_main.cpp built with g++ for the host alone (no device code, no GPU, no preload), once
    plainly and once under AddressSanitizer and UBSan: considered() exactly the reference's, the target within +-1 count per entry"""
    from conftest import REPO
    exe = tmp_path / "gumbel"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(REPO, "dotsboxesaz_amd", "csrc"), os.path.join(REPO, "tests", "gumbel_main.cpp"), "-o", str(exe)], check=True)
    seqs = [(m, R) for m in (1, 2, 3, 4, 5, 7, 8, 16, 17, 32, 100, 256) for R in (1, 2, 7, 16, 32, 33, 100, 200, 800)]
    roots = roots_of("3x3-script-m4", 2) + roots_of("6x6-script-m4-noreuse", 1)
    text = ["C %d %d" % s for s in seqs]
    for cv, cs, P, W, n, same, valid, _ in roots:
        text.append("T %d %s %s" % (len(n), float(cv).hex(), float(cs).hex()))
        for i in range(len(n)):
            text.append("%s %s %d %d" % (float(P[i]).hex(), float(W[i]).hex(), int(n[i]) | (0x40000000 if same[i] else 0), valid[i]))
    r = subprocess.run([str(exe)], input="\n".join(text) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)  # a sanitizer report has a message
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(seqs) + len(roots) and len(roots) > 60
    for line, (m, R) in zip(lines, seqs):
        assert [int(x) for x in line.split()] == [GR.considered(m, R, t) for t in range(R)], (m, R)
    for line, root in zip(lines[len(seqs):], roots):
        got = np.array(line.split(), dtype=np.int64)
        assert np.abs(got - root[-1]).max() <= 1, (got, root[-1])
