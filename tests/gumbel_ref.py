"""The Gumbel root search restated on the CPU (helper of test_gumbel_ref_cpu.py and test_hip_gumbel.py).  Three parts:

1. The rule -- considered(), the sum order, the completed Q, sigma, the pick, the move and the target -- written from the comment
   of dbaz_selfplay_set_gumbel in include/dbaz.h alone, in plain Python floats (float64, one rounding per operation), math.log
   and math.exp.
2. The sequential search with that root on top of forced_playouts_ref's Node / Tree (imported, not edited): below the root it is
   that search, which test_forced_playouts_ref_cpu.py pins to the oracle bit for bit.
3. The game loop in the shape of playout_cap_ref._run (same keys), with a mistake= switch for the helper's own tests, and the
   smallest gap between the best and the second score over every decision it makes (selections and moves alike): device and host
   log may differ in the last bit, which changes no decision while that gap is far above an ulp.

CASES is the table the CPU test checks the gap on and the GPU test plays."""
import functools
import math

import numpy as np

from oracle import oracle as O
import endgame_selfplay_ref as ESR
import forced_playouts_ref as FR
import playout_cap_ref as PCR

F32 = np.float32
TAG = 0x44444444
FLAG_FAST, FLAG_GUMBEL = 1, 4
MISTAKES = ("t_from_root_N", "n_for_ns", "g_in_target", "no_vmix", "halving_by_n", "dirichlet_kept")
NOISE = (0.8, 0.25)  # the engine's noise setting in every case: a Gumbel search must not mix it in


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------
def considered(m_eff, R, t):
    if m_eff <= 1:
        return t
    L = 0
    while (1 << L) < m_eff:
        L += 1
    nc, base, pos = m_eff, 0, 0
    while True:
        extra = max(1, R // (L * nc))
        ln = extra * nc
        if t < pos + ln:
            return base + (t - pos) // nc
        pos += ln
        base += extra
        nc = max(2, nc // 2)


def rule_sum(x):
    """lane i of 64 adds entries i, i + 64, i + 128, i + 192 (absent: +0.0); then s = s + s[lane ^ o], o = 32 .. 1"""
    a = np.zeros(256, np.float64)
    a[:len(x)] = x
    a = a.reshape(4, 64)
    s = np.zeros(64, np.float64)
    for j in range(4):
        s = s + a[j]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[idx ^ o]
    return float(s[0])


def u01(a, b):
    return (float(a >> 5) * 67108864.0 + float(b >> 6)) * (1.0 / 9007199254740992.0)


def philox_g(seed, game, ply, a):
    g, s = int(game) & 0xFFFFFFFFFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF
    w = PCR.philox4x32_10((g & PCR.M32, g >> 32, (int(ply) + 65536 * int(a)) & PCR.M32, TAG), (s & PCR.M32, s >> 32))
    u = u01(w[0], w[1])
    lo = 2.0 ** -53
    u = min(max(u, lo), 1.0 - lo)
    return -math.log(-math.log(u))


def q_values(W, n, sgn):
    """q(a) for n(a) > 0 (0.0 elsewhere, never read)"""
    return [(float(W[a]) / float(1 + int(n[a]))) * float(sgn[a]) if n[a] > 0 else 0.0 for a in range(len(n))]


def v_mix(P, q, n, mistake=None):
    if mistake == "no_vmix":
        return 0.0
    num = rule_sum([float(P[a]) * q[a] if n[a] > 0 else 0.0 for a in range(len(n))])
    den = rule_sum([float(P[a]) if n[a] > 0 else 0.0 for a in range(len(n))])
    return num / den if den != 0.0 else 0.0


def sigmas(c_visit, c_scale, P, W, n, sgn, valid, mistake=None):
    q = q_values(W, n, sgn)
    vm = v_mix(P, q, n, mistake)
    n_max = max([int(n[a]) for a in range(len(n)) if valid[a]] or [0])
    return [((c_visit + float(n_max)) * c_scale) * (q[a] if n[a] > 0 else vm) for a in range(len(n))]


def candidates(P, valid):
    C = [a for a in range(len(P)) if valid[a] and P[a] > 0]
    return C if C else [a for a in range(len(P)) if valid[a]]


def logit(p):
    return math.log(float(p)) if p > 0 else -1e30


def first_max(items, gaps):
    """items: [(a, score)] in index order -> the a of the first maximum; the gap to the second score goes into gaps"""
    best = max(s for _, s in items)
    if len(items) > 1:
        sc = sorted((s for _, s in items), reverse=True)
        gaps.append(sc[0] - sc[1])
    return next(a for a, s in items if s == best)


def target(c_visit, c_scale, P, W, n, sgn, valid, g=None, mistake=None):
    """int32 [A]: the row's visits"""
    A = len(P)
    C = candidates(P, valid)
    sg = sigmas(c_visit, c_scale, P, W, n, sgn, valid, mistake)
    x = {a: logit(P[a]) + sg[a] for a in C}
    if mistake == "g_in_target":
        x = {a: (g[a] + logit(P[a])) + sg[a] for a in C}
    M = max(x.values())
    e = [math.exp(x[a] - M) if a in x else 0.0 for a in range(A)]
    se = rule_sum(e)
    out = np.zeros(A, np.int32)
    for a in C:
        out[a] = int(math.floor((e[a] / se) * 16777216.0 + 0.5))
    return out


# ---- 2. the search ----------------------------------------------------------------------------------------------------------
class Tree(FR.Tree):
    """forced_playouts_ref.Tree (k = 0) with the Gumbel rule at the root of gsearch()"""
    gum = None

    def best_child(self, n, k, mistake):
        if self.gum is not None and n is self.first:
            return self.pick(mistake)
        return super().best_child(n, 0.0, None)

    def pick(self, mistake):
        G, r = self.gum, self.first
        nn = r.N
        ns = nn - G["n0"] if mistake != "n_for_ns" else nn
        t = self.nv_none if mistake == "t_from_root_N" else int((nn - G["n0"]).sum())
        sg = sigmas(G["c_visit"], G["c_scale"], r.priors, r.W, nn, r.changed, r.valid, mistake)
        cv = considered(G["m_eff"], G["R"], t)
        el = [a for a in G["C"] if ns[a] == cv]
        if not el:
            lo = min(int(ns[a]) for a in G["C"])
            el = [a for a in G["C"] if ns[a] == lo]
        if mistake == "halving_by_n":
            top = max(int(nn[a]) for a in el)
            el = [a for a in el if nn[a] == top]
        a = first_max([(a, G["gl"][a] + sg[a]) for a in el], G["gaps"])
        G["order"].append(a)
        return a

    def gsearch(self, R, ev, m, c_visit, c_scale, g, gaps, mistake=None, dirichlet=(0.0, 0.0), noise=None):
        """g: float64 [A] (read at the candidates).  Returns (move, the row's visits, info)"""
        if not self.first.expanded:
            self.search_once(ev)
        self.prep_root(dirichlet, noise)
        r = self.first
        C = candidates(r.priors, r.valid)
        gl = {a: float(g[a]) + logit(r.priors[a]) for a in C}
        self.gum = G = dict(C=C, gl=gl, n0=r.N.copy(), R=int(R), m_eff=min(int(m), len(C)), c_visit=float(c_visit), c_scale=float(c_scale),
                            gaps=gaps, order=[])
        for _ in range(int(R)):
            self.search_once(ev, 0.0, mistake)
        self.gum = None
        ns = r.N - G["n0"]
        sg = sigmas(c_visit, c_scale, r.priors, r.W, r.N, r.changed, r.valid, mistake)
        top = max(int(ns[a]) for a in C)
        move = first_max([(a, gl[a] + sg[a]) for a in C if ns[a] == top], gaps)
        vis = target(c_visit, c_scale, r.priors, r.W, r.N, r.changed, r.valid, g, mistake)
        return move, vis, dict(C=C, gl=gl, ns=ns, order=G["order"], m_eff=G["m_eff"], n0=G["n0"])


# ---- 3. the game ------------------------------------------------------------------------------------------------------------
def _run(d, *, seed, game_idx, sims, reuse, gumbel, g_vectors=None, cap=None, base_ev=0, start=(), noise=NOISE, mistake=None, on_root=None,
         scripted=None, choose=None, vectors=None):
    """one game.  gumbel: (m, c_visit, c_scale).  g_vectors(i, valid) -> the scripted float64 [A] g of ply i, None = Philox.
    cap: (full_prob, fast_reads) or None.  scripted: moves that win over the rule's (-1: the rule's).  Keys of the result: those of
    playout_cap_ref._run, plus flags, vectors (the g of every ply), min_gap and n_gumbel.
    m = 0: the rule is off -- the game of forced_playouts_ref._run at k = 0, played on this module's Tree: choose(i, visits) -> the
    move, vectors(i, valid) -> the Dirichlet vector of ply i."""
    assert mistake is None or mistake in MISTAKES
    if gumbel[0] == 0:
        return _run_off(d, choose, seed=seed, game_idx=game_idx, sims=sims, reuse=reuse, noise=noise, vectors=vectors, cap=cap, base_ev=base_ev,
                        start=start)
    ev = FR.formula(base_ev) if isinstance(base_ev, int) else base_ev
    m, c_visit, c_scale = gumbel
    t = Tree(d, O.state_from_moves(d, list(start)))
    keys = ("x", "player", "visits", "pi", "q_value", "max_deepness", "tree_size", "terminal_count", "played", "reads", "full", "served", "flags")
    out = {key: [] for key in keys}
    vecs, gaps = [], []
    n_search, i = 0, 0
    rs = np.random.RandomState(12345 + int(game_idx))  # the Dirichlet draws of the mistake "dirichlet_kept"
    while not t.is_terminal:
        st = t.state
        valid = t.first.valid
        reads = ESR._fact_reads(int(valid.sum()), sims)
        full = cap is None or PCR.is_full(seed, game_idx, i, cap[0])
        if not full:
            reads = min(reads, cap[1])
        if g_vectors is not None:
            g = np.asarray(g_vectors(i, valid), np.float64)
        else:
            g = np.array([philox_g(seed, game_idx, i, a) for a in range(d.A)], np.float64)
        vecs.append(g)
        expanded = t.is_expanded
        kw = {}
        if mistake == "dirichlet_kept" and full:
            kw = dict(dirichlet=tuple(noise), noise=rs.dirichlet(np.where(valid, 1.0, 1e-60) * noise[0]))
        move, vis, info = t.gsearch(reads, ev, m, c_visit, c_scale, g, gaps, mistake, **kw)
        n_search += reads + (0 if expanded else 1)
        if on_root is not None:
            on_root(t, info, reads, full)
        if scripted is not None and scripted[i] >= 0:
            move = int(scripted[i])
        md, ts, tc, q = t.stats()
        s = int(vis.sum())
        row = dict(x=O.features(d, st).ravel(), player=st.to_play, visits=vis, pi=vis.astype(np.float64) / (s if s else 1.0),
                   q_value=np.float32(q), max_deepness=md, tree_size=ts, terminal_count=tc, played=move, reads=reads, full=full,
                   served=False, flags=FLAG_GUMBEL | (0 if full else FLAG_FAST))
        for key, v in row.items():
            out[key].append(v)
        t.advance(move, reuse)
        i += 1
    res = {key: np.array(v) for key, v in out.items()}
    res["x"] = res["x"].astype(np.int16).reshape(len(out["x"]), -1)
    term = t.state
    zt = O.get_result(term)
    res["z"] = np.array([zt if p == term.just_played else -zt for p in out["player"]], np.int64)
    res.update(n_rows=i, n_search=n_search, vectors=np.array(vecs, np.float64), min_gap=min(gaps) if gaps else float("inf"), n_gumbel=i)
    return res


def _run_off(d, choose, *, seed, game_idx, sims, reuse, noise, vectors, cap, base_ev, start):
    """forced_playouts_ref's game loop at k = 0, played on this module's Tree (whose Gumbel state stays None)"""
    saved = FR.Tree
    FR.Tree = Tree
    try:
        res = FR._run(d, choose, seed=seed, game_idx=game_idx, sims=sims, reuse=reuse, noise=noise, vectors=vectors, cap=cap, base_ev=base_ev,
                      start=start, forced_playouts=None)
    finally:
        FR.Tree = saved
    res["flags"] = np.where(res["full"], 0, FLAG_FAST)
    res.update(min_gap=float("inf"), n_gumbel=0)
    return res


def gumbel_vectors(rs):
    """standard Gumbel draws from the RandomState rs, one vector per ply"""
    return lambda i, valid: rs.gumbel(size=len(valid))


def play_game(d, *, g_mode, game_idx, **kw):
    """g_mode "script": the g of every ply drawn from RandomState(1000 + game) (to be scripted into the engine); "philox": the rule's"""
    gv = gumbel_vectors(np.random.RandomState(1000 + int(game_idx))) if g_mode == "script" else None
    return _run(d, game_idx=game_idx, g_vectors=gv, **kw)


# ---- the case table -----------------------------------------------------------------------------------------------------------
SEED = 7
C_VISIT, C_SCALE = 50.0, 1.0
KIND = {"formula": 0, "uniform": 1}
CASES = [
    # name, rows, cols, reads, m, reuse, cap, g, evaluator, games
    ("3x3-script-m4", 3, 3, 32, 4, True, None, "script", "formula", 16),
    ("3x3-philox-m16-noreuse", 3, 3, 16, 16, False, None, "philox", "formula", 16),
    ("3x3-philox-m2-cap", 3, 3, 32, 2, True, (0.5, 8), "philox", "uniform", 16),
    ("3x3-script-m16-cap-noreuse", 3, 3, 32, 16, False, (0.5, 8), "script", "formula", 8),
    ("6x6-philox-m16", 6, 6, 32, 16, True, None, "philox", "formula", 4),
    ("6x6-script-m4-noreuse", 6, 6, 16, 4, False, None, "script", "uniform", 4),
    ("8x8-philox-m16", 8, 8, 16, 16, True, None, "philox", "formula", 4),
    ("10x10-script-m16", 10, 10, 16, 16, True, None, "script", "formula", 2),
]
CASE_IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_games(name, mistake=None, n_games=None):
    """the games of a case, computed once and shared (callers leave them unchanged)"""
    _, R, Cc, sims, m, reuse, cap, g_mode, ev, games = next(c for c in CASES if c[0] == name)
    d = O.dims(R, Cc)
    return [play_game(d, g_mode=g_mode, game_idx=gi, seed=SEED, sims=sims, reuse=reuse, gumbel=(m, C_VISIT, C_SCALE), cap=cap,
                      base_ev=KIND[ev], mistake=mistake) for gi in range(n_games or games)]
