"""Playout cap randomization restated on the CPU (helper of test_playout_cap_rule.py, test_playout_cap_ref_cpu.py and
test_hip_playout_cap.py), written from the comment of dbaz_selfplay_set_playout_cap in include/dbaz.h.

The rule: the search of game g at ply i under seed s is FULL iff word 0 of Philox4x32-10 with counter (lo32(g), hi32(g), i,
0x33333333) and key (lo32(s), hi32(s)) is below floor(full_prob * 2^32).  Pure Python integers here.

The game: one oracle.Tree, moved on ply by ply as tests/endgame_selfplay_ref.py does it.  Per move the rule gives the reads and
the `dirichlet=` of UCT_search: a full search runs the driver rule's reads with the configured noise (its vector scripted per
ply), a fast one min(driver rule, fast_reads) reads with dirichlet=(0.0, 0.0), whatever vector its ply has.  An endgame table
(endgame_selfplay_ref.Table) serves the searches under late roots and endgame_reads caps them on top.  The plies count from the
game's start position."""
import numpy as np

from oracle import oracle as O
import endgame_selfplay_ref as ESR

M32 = 0xFFFFFFFF
PURPOSE = 0x33333333


def philox4x32_10(ctr, key):
    """the four output words of Philox4x32-10 (the rounds and constants of tree.hip's philox())"""
    c0, c1, c2, c3 = (int(c) & M32 for c in ctr)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def thresh(full_prob):
    return int(np.floor(np.float64(full_prob) * 4294967296.0))


def is_full(seed, game_idx, ply, full_prob):
    if full_prob >= 1.0:
        return True
    g, s = int(game_idx) & 0xFFFFFFFFFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((g & M32, g >> 32, int(ply), PURPOSE), (s & M32, s >> 32))[0]
    return x < thresh(full_prob)


MISTAKES = ("noise_on_fast", "no_fast_budget", "ply_from_empty_board")


def _run(d, choose, *, seed, game_idx, sims, reuse, noise=(0.0, 0.0), vectors=None, cap=None, base_ev=0, start=(), K=1, table=None,
         endgame_reads=0, mistake=None):
    """one game; choose(i, visits) -> the move of ply i (counted from the start position).  vectors(i, valid) -> the float64 [A]
    noise vector of ply i (called for every ply when noise[0] > 0, so that a game's vectors do not depend on the cap).
    cap: (full_prob, fast_reads) or None.  mistake: one of MISTAKES, for the helper's own tests."""
    assert mistake is None or mistake in MISTAKES
    g = ESR._Game(d, base_ev, table, None)
    t = O.Tree(d, O.state_from_moves(d, list(start)))
    keys = ("x", "player", "visits", "pi", "q_value", "max_deepness", "tree_size", "terminal_count", "played", "reads", "full", "served")
    out = {k: [] for k in keys}
    vecs = []
    n_search, i = 0, 0
    while not t.is_terminal:
        st = t.state
        valid = O.valid_moves(d, st).astype(bool)
        F = int(valid.sum())
        reads = ESR._fact_reads(F, sims)
        ply = i + (len(start) if mistake == "ply_from_empty_board" else 0)
        full = cap is None or is_full(seed, game_idx, ply, cap[0])
        if not full and mistake != "no_fast_budget":
            reads = min(reads, cap[1])
        g.use_table = table is not None and F <= table.max_free
        if g.use_table:
            if g.ref is None:
                g.ref = ESR.SlotTablesRef(table.R, table.C, O.features(d, st).ravel()[None], table.seed, table.max_free)
            if endgame_reads > 0:
                reads = min(reads, endgame_reads)
        vec = vectors(i, valid) if noise[0] > 0 else None
        vecs.append(vec)
        noisy = noise[0] > 0 and (full or mistake == "noise_on_fast")
        expanded = t.is_expanded
        vis = t.search(reads, g.ev, dirichlet=tuple(noise) if noisy else (0.0, 0.0), noise=vec if noisy else None, max_pending=K)
        n_search += reads + (0 if expanded else 1)
        md, ts, tc, q = t.stats()
        s = int(vis.sum())
        move = int(choose(i, vis))
        row = dict(x=O.features(d, st).ravel(), player=st.to_play, visits=vis, pi=vis.astype(np.float64) / (s if s else 1.0),
                   q_value=np.float32(q), max_deepness=md, tree_size=ts, terminal_count=tc, played=move, reads=reads, full=full,
                   served=g.use_table)
        for k, v in row.items():
            out[k].append(v)
        t.advance(move, reuse)
        i += 1
    res = {k: np.array(v) for k, v in out.items()}
    res["x"] = res["x"].astype(np.int16).reshape(len(out["x"]), -1)
    term = t.state
    zt = O.get_result(term)
    res["z"] = np.array([zt if p == term.just_played else -zt for p in out["player"]], np.int64)
    res.update(n_rows=i, n_search=n_search, vectors=np.array(vecs, np.float64) if noise[0] > 0 else None)
    return res


def dirichlet_vectors(rs, alpha):
    """the reference's draw (mcts.py:220-222) from the RandomState rs, one per call"""
    return lambda i, valid: rs.dirichlet(np.where(valid, 1.0, 1e-60) * alpha)


def generate_game(d, rs, **kw):
    """a game by these rules with the moves sampled from pi (temperature 1) by the RandomState rs -- and, with noise, its
    per-ply vectors drawn from rs too (result["vectors"])"""
    if kw.get("noise", (0.0, 0.0))[0] > 0 and "vectors" not in kw:
        kw["vectors"] = dirichlet_vectors(rs, kw["noise"][0])
    return _run(d, lambda i, vis: rs.choice(len(vis), p=vis / vis.sum()), **kw)


def replay_game(d, played, vectors=None, **kw):
    """the game with the moves `played` teacher-forced, its noise vectors (float64 [plies, A]) scripted"""
    played = np.asarray(played).astype(np.int64)
    return _run(d, lambda i, vis: played[i], vectors=(lambda i, valid: np.asarray(vectors[i], np.float64)) if vectors is not None else None, **kw)


def rows_differ(ref, rows):
    """the first row at which a game of this module and `rows` (arrays in move order: x, player, visits, pi, q_value, TreeStats,
    z, played) differ bit for bit, or -1"""
    return ESR.rows_differ(ref, rows)
