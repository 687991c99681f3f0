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
  here so that this holds."""
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
    _, R, C, sims, m, reuse, cap, g_mode, ev, _ = next(c for c in GR.CASES if c[0] == name)
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
        GR.play_game(d, g_mode=g_mode, game_idx=gi, seed=GR.SEED, sims=sims, reuse=reuse, gumbel=(m, GR.C_VISIT, GR.C_SCALE), cap=cap,
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


def roots_of(name, n_games):
    """(c_visit, c_scale, P, W, n, same, valid, the reference's visits) of every root of a case's first games"""
    _, R, C, sims, m, reuse, cap, g_mode, ev, _ = next(c for c in GR.CASES if c[0] == name)
    d = O.dims(R, C)
    roots = []

    def on_root(t, info, reads, full):
        P, W, n, sgn = t.root_arrays()
        valid = t.first.valid.copy()
        roots.append((GR.C_VISIT, GR.C_SCALE, P, W, n, sgn > 0, valid, GR.target(GR.C_VISIT, GR.C_SCALE, P, W, n, sgn, valid)))

    for gi in range(n_games):
        GR.play_game(d, g_mode=g_mode, game_idx=gi, seed=GR.SEED, sims=sims, reuse=reuse, gumbel=(m, GR.C_VISIT, GR.C_SCALE), cap=cap,
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
