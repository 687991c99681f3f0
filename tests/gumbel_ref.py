"""The Gumbel root search restated on the CPU (helper of test_gumbel_ref_cpu.py, test_hip_gumbel.py, test_hip_gumbel_net.py and
test_hip_gumbel_features.py).  Three parts:

1. The rule -- considered(), the sum order, the completed Q, sigma, the pick, the move and the target -- written from the comment
   of dbaz_selfplay_set_gumbel in include/dbaz.h alone, in plain Python floats (float64, one rounding per operation), math.log
   and math.exp.
2. The sequential search with that root on top of forced_playouts_ref's Node / Tree (imported, not edited): below the root it is
   that search, which test_forced_playouts_ref_cpu.py pins to the oracle bit for bit.
3. The game loop in the shape of playout_cap_ref._run (same keys), with a mistake= switch for the helper's own tests, and the
   smallest gap between the best and the second score over every decision it makes (selections and moves alike): device and host
   log may differ in the last bit, which changes no decision while that gap is far above an ulp.

The game loop also takes an endgame table (endgame_selfplay_ref.Table: the rule of endgame_selfplay_ref._run per search root, on
its _Game), a leaf solver (leaf_solve_ref.LeafSolver as base_ev, told every move after the move's search) and start positions.

CASES is the table the CPU test checks the gap on and the GPU test plays; FEATURES the cases of test_hip_gumbel_features.py."""
import functools
import math

import numpy as np

from oracle import oracle as O
import endgame_selfplay_ref as ESR
import forced_playouts_ref as FR
import leaf_solve_ref as LSR
import playout_cap_ref as PCR

F32 = np.float32
TAG = 0x44444444
FLAG_FAST, FLAG_GUMBEL = 1, 4
MISTAKES = ("t_from_root_N", "n_for_ns", "g_in_target", "no_vmix", "halving_by_n", "dirichlet_kept")
# what only a table, a zero prior or a start position can show: R of the halving not capped by endgame_reads, a valid child with
# P == 0 among the candidates of a root that has positive priors, g drawn at the ply counted from the empty board
MISTAKES_NEW = ("R_uncapped", "zero_prior_candidate", "ply_from_empty_board")
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


def candidates(P, valid, mistake=None):
    C = [a for a in range(len(P)) if valid[a] and P[a] > 0]
    return C if C and mistake != "zero_prior_candidate" else [a for a in range(len(P)) if valid[a]]


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
    C = candidates(P, valid, mistake)
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

    def gsearch(self, R, ev, m, c_visit, c_scale, g, gaps, mistake=None, dirichlet=(0.0, 0.0), noise=None, R_kept=None):
        """g: float64 [A] (read at the candidates).  R_kept: the R of considered() where a mistake makes it another number than the
        reads that are run.  Returns (move, the row's visits, info).
        A root without a positive prior is tied: every score is -1e30 exactly (g and sigma, at most 1e9 * |q|, are absorbed: an ulp
        of 1e30 is 1.4e14), the first index wins every pick, and none of its decisions goes into gaps."""
        if not self.first.expanded:
            self.search_once(ev)
        self.prep_root(dirichlet, noise)
        r = self.first
        C = candidates(r.priors, r.valid, mistake)
        tied = not any(r.valid[a] and r.priors[a] > 0 for a in range(len(r.valid)))
        if tied:
            gaps = []
        gl = {a: float(g[a]) + logit(r.priors[a]) for a in C}
        self.gum = G = dict(C=C, gl=gl, n0=r.N.copy(), R=int(R if R_kept is None else R_kept), m_eff=min(int(m), len(C)), c_visit=float(c_visit),
                            c_scale=float(c_scale), gaps=gaps, order=[])
        for _ in range(int(R)):
            self.search_once(ev, 0.0, mistake)
        self.gum = None
        ns = r.N - G["n0"]
        sg = sigmas(c_visit, c_scale, r.priors, r.W, r.N, r.changed, r.valid, mistake)
        top = max(int(ns[a]) for a in C)
        move = first_max([(a, gl[a] + sg[a]) for a in C if ns[a] == top], gaps)
        vis = target(c_visit, c_scale, r.priors, r.W, r.N, r.changed, r.valid, g, mistake)
        return move, vis, dict(C=C, gl=gl, ns=ns, order=G["order"], m_eff=G["m_eff"], n0=G["n0"], R=G["R"], tied=tied)


# ---- 3. the game ------------------------------------------------------------------------------------------------------------
def _scalar_v(evaluate):
    """a network's v comes as an array of one element: the tree's float32 sums want the element"""
    def ev(d, st):
        p, v = evaluate(d, st)
        return p, np.float32(np.asarray(v).ravel()[0])
    return ev


def _run(d, *, seed, game_idx, sims, reuse, gumbel, g_vectors=None, cap=None, base_ev=0, start=(), noise=NOISE, mistake=None, on_root=None,
         scripted=None, choose=None, vectors=None, table=None, endgame_reads=0, served_from=None):
    """one game.  gumbel: (m, c_visit, c_scale).  g_vectors(i, valid) -> the scripted float64 [A] g of ply i, None = Philox.
    cap: (full_prob, fast_reads) or None.  scripted: moves that win over the rule's (-1: the rule's).  Keys of the result: those of
    playout_cap_ref._run, plus flags, vectors (the g of every ply), min_gap, n_gumbel and n_tied_roots (the roots without a positive
    prior: their decisions are exact ties, which the first index wins, and are not in min_gap).
    base_ev: a formula kind, an evaluate(d, state), or a leaf_solve_ref.LeafSolver, which is told every move after its search.
    table: an endgame_selfplay_ref.Table -- the rule of endgame_selfplay_ref._run per search root: a root with F <= max_free free
    edges (at a ply >= served_from) is served, every leaf its search expands gets the game's table's answer, and its reads are
    min(reads, endgame_reads) when endgame_reads > 0; further keys n_free, m_eff, R, n0_any (per row), base_calls, table_calls and
    first_served.  The plies count from the start position.
    m = 0: the rule is off -- the game of forced_playouts_ref._run at k = 0, played on this module's Tree: choose(i, visits) -> the
    move, vectors(i, valid) -> the Dirichlet vector of ply i."""
    assert mistake is None or mistake in MISTAKES or mistake in MISTAKES_NEW
    if gumbel[0] == 0:
        return _run_off(d, choose, seed=seed, game_idx=game_idx, sims=sims, reuse=reuse, noise=noise, vectors=vectors, cap=cap, base_ev=base_ev,
                        start=start)
    solver = base_ev if isinstance(base_ev, LSR.LeafSolver) else None
    if solver is not None:
        solver.start_game(d, game_idx)
        for mv in start:
            O.play_(d, solver.state, int(mv))
        solver._root()
        ev = solver.evaluate
    else:
        ev = FR.formula(base_ev) if isinstance(base_ev, int) else _scalar_v(base_ev)
    game = ESR._Game(d, ev, table, None)  # the table's answers and the switch per search root; without a table it only counts
    served_from = 0 if served_from is None else served_from
    m, c_visit, c_scale = gumbel
    t = Tree(d, O.state_from_moves(d, list(start)))
    keys = ("x", "player", "visits", "pi", "q_value", "max_deepness", "tree_size", "terminal_count", "played", "reads", "full", "served", "flags",
            "n_free", "m_eff", "R", "n0_any")
    out = {key: [] for key in keys}
    vecs, gaps = [], []
    n_search, i, n_tied, first_served = 0, 0, 0, -1
    rs = np.random.RandomState(12345 + int(game_idx))  # the Dirichlet draws of the mistake "dirichlet_kept"
    while not t.is_terminal:
        st = t.state
        valid = t.first.valid
        F = int(valid.sum())
        reads = rule_reads = ESR._fact_reads(F, sims)
        full = cap is None or PCR.is_full(seed, game_idx, i, cap[0])
        if not full:
            reads = rule_reads = min(reads, cap[1])
        game.use_table = table is not None and F <= table.max_free and i >= served_from
        if game.use_table:
            if first_served < 0:
                first_served = i
            if game.ref is None:
                game.ref = ESR.SlotTablesRef(table.R, table.C, O.features(d, st).ravel()[None], table.seed, table.max_free)
            if endgame_reads > 0:
                reads = min(reads, endgame_reads)
        if g_vectors is not None:
            g = np.asarray(g_vectors(i, valid), np.float64)
        else:
            ply = i + (len(start) if mistake == "ply_from_empty_board" else 0)
            g = np.array([philox_g(seed, game_idx, ply, a) for a in range(d.A)], np.float64)
        vecs.append(g)
        expanded = t.is_expanded
        kw = {}
        if mistake == "dirichlet_kept" and full:
            kw = dict(dirichlet=tuple(noise), noise=rs.dirichlet(np.where(valid, 1.0, 1e-60) * noise[0]))
        if mistake == "R_uncapped":
            kw["R_kept"] = rule_reads
        move, vis, info = t.gsearch(reads, game._evaluate, m, c_visit, c_scale, g, gaps, mistake, **kw)
        n_search += reads + (0 if expanded else 1)
        n_tied += bool(info["tied"])
        info["served"] = game.use_table
        if on_root is not None:
            on_root(t, info, reads, full)
        if scripted is not None and scripted[i] >= 0:
            move = int(scripted[i])
        if solver is not None:
            solver.after_search(move)
        md, ts, tc, q = t.stats()
        s = int(vis.sum())
        row = dict(x=O.features(d, st).ravel(), player=st.to_play, visits=vis, pi=vis.astype(np.float64) / (s if s else 1.0),
                   q_value=np.float32(q), max_deepness=md, tree_size=ts, terminal_count=tc, played=move, reads=reads, full=full,
                   served=game.use_table, flags=FLAG_GUMBEL | (0 if full else FLAG_FAST), n_free=F, m_eff=info["m_eff"], R=info["R"],
                   n0_any=bool(info["n0"].any()))
        for key, v in row.items():
            out[key].append(v)
        t.advance(move, reuse)
        i += 1
    res = {key: np.array(v) for key, v in out.items()}
    res["x"] = res["x"].astype(np.int16).reshape(len(out["x"]), -1)
    term = t.state
    zt = O.get_result(term)
    res["z"] = np.array([zt if p == term.just_played else -zt for p in out["player"]], np.int64)
    res.update(n_rows=i, n_search=n_search, vectors=np.array(vecs, np.float64), min_gap=min(gaps) if gaps else float("inf"), n_gumbel=i,
               n_tied_roots=n_tied, base_calls=game.calls["base"], table_calls=game.calls["table"], first_served=first_served)
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
    # name, rows, cols, reads, m, reuse, cap, g, evaluator, games, c_visit, c_scale
    ("3x3-script-m4", 3, 3, 32, 4, True, None, "script", "formula", 16, C_VISIT, C_SCALE),
    ("3x3-philox-m16-noreuse", 3, 3, 16, 16, False, None, "philox", "formula", 16, C_VISIT, C_SCALE),
    ("3x3-philox-m2-cap", 3, 3, 32, 2, True, (0.5, 8), "philox", "uniform", 16, C_VISIT, C_SCALE),
    ("3x3-script-m16-cap-noreuse", 3, 3, 32, 16, False, (0.5, 8), "script", "formula", 8, C_VISIT, C_SCALE),
    ("6x6-philox-m16", 6, 6, 32, 16, True, None, "philox", "formula", 4, C_VISIT, C_SCALE),
    ("6x6-script-m4-noreuse", 6, 6, 16, 4, False, None, "script", "uniform", 4, C_VISIT, C_SCALE),
    ("8x8-philox-m16", 8, 8, 16, 16, True, None, "philox", "formula", 4, C_VISIT, C_SCALE),
    ("10x10-script-m16", 10, 10, 16, 16, True, None, "script", "formula", 2, C_VISIT, C_SCALE),
    # other boards and constants: one box, a non-square board with an m that is no power of two, and the ends of the constants' ranges
    ("1x1-philox-m256", 1, 1, 32, 256, True, None, "philox", "formula", 16, C_VISIT, C_SCALE),
    ("2x7-script-m3", 2, 7, 16, 3, True, None, "script", "formula", 4, C_VISIT, C_SCALE),
    ("3x3-philox-cvisit0-cscale0.1", 3, 3, 32, 16, True, None, "philox", "formula", 16, 0.0, 0.1),
    ("3x3-philox-cvisit1e6", 3, 3, 32, 16, True, None, "philox", "formula", 16, 1e6, 1.0),
]
CASE_IDS = [c[0] for c in CASES]


def case(name):
    return next(c for c in CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def case_games(name, mistake=None, n_games=None):
    """the games of a case, computed once and shared (callers leave them unchanged)"""
    _, R, Cc, sims, m, reuse, cap, g_mode, ev, games, c_visit, c_scale = case(name)
    d = O.dims(R, Cc)
    return [play_game(d, g_mode=g_mode, game_idx=gi, seed=SEED, sims=sims, reuse=reuse, gumbel=(m, c_visit, c_scale), cap=cap,
                      base_ev=KIND[ev], mistake=mistake) for gi in range(n_games or games)]


# ---- the network cases (test_hip_gumbel_net.py plays these; the reference's evaluator there is the engine itself) -------------------
NET_SEED = {(3, 3): 1, (6, 6): 1, (8, 8): 1, (10, 10): 1}  # torch.manual_seed of the board's network: picked so that the gap condition holds
NET = {
    # slots: above 16 and no multiple of 16 (the full-rounds cut needs n_slots > eval_round); games = slots; replay: fixed game indices
    (3, 3): dict(slots=40, sims=32, replay=(0, 5, 11, 17, 22, 28, 33, 39)),
    (6, 6): dict(slots=24, sims=16, replay=(3, 20)),
    (8, 8): dict(slots=24, sims=16, replay=(17,)),
    (10, 10): dict(slots=24, sims=16, replay=(6,)),
}
NET_ZERO = tuple(range(0, 32, 2))  # 3x3: the actions whose policy bias is -200, half of the 32
NET_ZERO_REPLAY = (0, 3, 6, 9, 12, 15)


def network(R, C, zero=False):
    """the small seeded random network of the other network tests; zero: the bias of the policy head's last layer at -200 on NET_ZERO"""
    import torch
    from dotsboxesaz_amd import nn as dnn
    torch.manual_seed(NET_SEED[(R, C)])
    model = dnn.ResNetZero(dnn.resnet_params(R, C, 32, 2, 4, 8))
    if zero:
        with torch.no_grad():
            model.policy_head.fc.bias[list(NET_ZERO)] = -200.0
    return model


def play_recording_roots(d, **kw):
    """play_game, and per ply (valid, the root's float64 priors, gsearch's info) as the search left them"""
    roots = []
    return play_game(d, on_root=lambda t, info, reads, full: roots.append((t.first.valid.copy(), t.first.priors.copy(), info)), **kw), roots


def zero_prior_roots(g, roots, zero):
    """the three kinds of root in a game whose evaluator gives the actions `zero` a prior of exactly 0, each checked against the rule:
    returns (roots with both kinds of valid child, roots without a positive prior, whether the game changes from one to the other)"""
    mixed, kinds = 0, []
    for i, (valid, P, info) in enumerate(roots):
        z = [a for a in range(len(P)) if valid[a] and P[a] == 0]
        pos = [a for a in range(len(P)) if valid[a] and P[a] > 0]
        assert set(z) <= set(zero) and info["tied"] == (not pos)
        v = g["visits"][i]
        if pos and z:  # a child with P == 0 is no candidate: never visited by this search, never played, 0 in the target
            mixed += 1
            assert not v[z].any() and not info["ns"][z].any() and g["played"][i] not in z
        if not pos:  # every valid child is a candidate at -1e30: a uniform target, and the first valid index wins every pick
            assert len(set(v[z])) == 1 and v[z].sum() == v.sum() and abs(int(v.sum()) - (1 << 24)) <= len(z)
            assert g["played"][i] == z[0] and info["order"][0] == z[0]
        kinds.append(bool(pos))
    tied = sum(1 for k in kinds if not k)
    assert g["n_tied_roots"] == tied
    return mixed, tied, any(a and not b for a, b in zip(kinds, kinds[1:]))


def torch_evaluator(model, R, C):
    """evaluate(d, state) by the oracle's torch forward pass of the same weights, one position at a time, memoised (CPU)"""
    from oracle import nn_ref
    ref = nn_ref.ResNetZeroRef(R, C, 32, 2, head_channels=4, value_fc=8)
    ref.load_state_dict(model.state_dict(), strict=True)
    memo = {}

    def ev(d, st):
        x = O.features(d, st)
        key = x.tobytes()
        if key not in memo:
            p, v = nn_ref.predict_sync(ref, x.astype(np.float32).reshape(1, 3, R + 1, C + 1))
            memo[key] = (p[0].copy(), v[0].copy())
        return memo[key]
    return ev


# ---- the rule next to the other self-play features (test_hip_gumbel_features.py plays these; formula evaluators) ------------------
TABLE_SEED = 3  # endgame_seed: which of several optimal moves gets the prior


def openings(d, n, lengths, seed=11):
    """n legal unfinished openings of the given lengths, drawn by the oracle's rules from RandomState(seed)"""
    rs = np.random.RandomState(seed)
    book = []
    for k in range(n):
        while True:
            s, moves = O.new_state(d), []
            for _ in range(lengths[k]):
                valid = np.nonzero(O.valid_moves(d, s))[0]
                mv = int(valid[rs.randint(len(valid))])
                O.play_(d, s, mv)
                moves.append(mv)
            if O.get_result(s) is None:
                break
        book.append(moves)
    return book


def start_of(game_idx, n_starts, games_per_start):
    """Engine.selfplay_set_start's mapping: game g starts from move_lists[(g // games_per_start) % n_starts]"""
    return (int(game_idx) // games_per_start) % n_starts


FEATURES = {
    # table: the Endgame's max_free; leaf: the leaf solver's L; starts: the openings' lengths (games_per_start = 2);
    # replay: the games the reference plays (all of them by default)
    "3x3-table": dict(R=3, C=3, sims=32, m=16, reuse=True, g="philox", games=16, slots=24, table=8, endgame_reads=0),
    "3x3-table-reads3": dict(R=3, C=3, sims=32, m=16, reuse=True, g="philox", games=16, slots=24, table=8, endgame_reads=3),
    # (a cap of 3 cannot tell which R the halving keeps: considered(m', R, t) is the same for every R while t < 3.  12 can.)
    "3x3-table-reads12": dict(R=3, C=3, sims=32, m=16, reuse=True, g="philox", games=16, slots=24, table=8, endgame_reads=12),
    "4x4-table": dict(R=4, C=4, sims=32, m=16, reuse=True, g="philox", games=16, slots=24, table=12, endgame_reads=0),
    "4x4-table-reads3": dict(R=4, C=4, sims=32, m=16, reuse=True, g="philox", games=16, slots=24, table=12, endgame_reads=3),
    "3x3-leaf": dict(R=3, C=3, sims=32, m=16, reuse=True, g="philox", games=16, slots=8, leaf=6),
    "3x3-leaf-noreuse": dict(R=3, C=3, sims=32, m=16, reuse=False, g="philox", games=16, slots=8, leaf=6),
    "2x7-leaf": dict(R=2, C=7, sims=16, m=16, reuse=True, g="philox", games=4, slots=8, leaf=7),
    "2x7-leaf-noreuse": dict(R=2, C=7, sims=16, m=16, reuse=False, g="philox", games=4, slots=8, leaf=7),
    "3x3-start-philox": dict(R=3, C=3, sims=32, m=16, reuse=True, g="philox", games=12, slots=8, starts=(1, 4, 6)),
    "6x6-start-script": dict(R=6, C=6, sims=16, m=16, reuse=True, g="script", games=6, slots=8, starts=(2, 5, 9)),
    "3x3-40-slots": dict(R=3, C=3, sims=32, m=16, reuse=True, g="philox", games=80, slots=40, replay=(0, 7, 16, 23, 39, 40, 57, 79)),
}
FEATURE_IDS = list(FEATURES)


def feature_book(name):
    f = FEATURES[name]
    return openings(O.dims(f["R"], f["C"]), len(f["starts"]), f["starts"]) if "starts" in f else None


@functools.lru_cache(maxsize=None)
def feature_games(name, mistake=None, n_games=None, table=True, endgame_reads=None, served_from=None):
    """{game index: the game} of a case of FEATURES and its LeafSolver (or None), computed once and shared (callers leave them
    unchanged).  table=False: every root unserved; endgame_reads: another cap than the case's; served_from: ((game, ply), ...)."""
    f = FEATURES[name]
    d = O.dims(f["R"], f["C"])
    tab = ESR.Table(f["R"], f["C"], f["table"], TABLE_SEED) if "table" in f and table else None
    w = LSR.LeafSolver(f["R"], f["C"], f["leaf"], TABLE_SEED, 0) if "leaf" in f else None
    book = feature_book(name)
    late = dict(served_from or ())
    out = {}
    for gi in list(f.get("replay", range(f["games"])))[:n_games]:
        start = book[start_of(gi, len(book), 2)] if book else ()
        out[gi] = play_game(d, g_mode=f["g"], game_idx=gi, seed=SEED, sims=f["sims"], reuse=f["reuse"], gumbel=(f["m"], C_VISIT, C_SCALE),
                            base_ev=w if w is not None else 0, mistake=mistake, start=start, table=tab,
                            endgame_reads=f.get("endgame_reads", 0) if endgame_reads is None else endgame_reads, served_from=late.get(gi))
    return out, w
