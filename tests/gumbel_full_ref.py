"""The full mode of the Gumbel search (dbaz_selfplay_set_gumbel_mode: the rule below the root, and the full v_mix) restated on the CPU
(helper of test_gumbel_full_ref_cpu.py, test_gumbel_full_abi.py and the test_hip_gumbel_full*.py files).  Written from the comment of
dbaz_selfplay_set_gumbel_mode in include/dbaz.h alone, in plain Python floats (float64, one rounding per operation), math.log and
math.exp, on top of gumbel_ref (imported, not edited):

1. The rule on one node: v_mix_full, improved_policy, nonroot_scores / nonroot_pick, target_full.
2. Tree, a subclass of gumbel_ref.Tree: it remembers the float32 value every node got at its expansion, takes the rule's pick in
   best_child below the root, and -- for the time of a gsearch -- puts the full v_mix into the sigmas of the root that gumbel_ref's
   pick, move and target read.
3. run(): gumbel_ref._run's game loop (tables, the leaf solver, start positions and the cap with it) on that Tree, with a mistake=
   switch for the helper's own tests and the statistics of the interior picks.

The error bound of a score, and why a gap of 1e-9 is far from it (u = 2^-53).  A decision below the root compares
s(a) = pi'(a) - n(a) / (1 + S).  The second term is one correctly rounded division of exactly known integers: identical bits on device
and host.  v^, q, v_mix and sigma are +, *, / of identical inputs in a stated order: identical bits too.  The two sides differ only
in log and exp, each within 1 ulp of the true value, so within 2 ulp of each other:
  logit(a) = log P differs by at most 4u |log P| (about 4e-15 for the priors that matter, |log P| <= 10);
  x(a) = logit + sigma is one rounding of two sums that differ by that little: the results differ by at most 4u |log P| + 2u |x|,
    and so does x - M (M is one of the x);
  e(a) = exp(x - M) then differs relatively by that amount plus 4u for exp itself;
  sum e adds A - 1 terms in the same order on both sides: the relative difference of the terms carries over, and roundings that
    fall differently add at most (A - 1) u;  the division adds u.
So pi' differs relatively by about (A + 8) * 2u plus 4u |log P| + 2u |x|.  With pi' <= 1 and |x| of the order of |log P| that is
(A + 8) * 2^-52 <= 6e-14 at A = 242.  Only the constants (c_visit, c_scale) = (1e6, 1) make |x| large: there |x| <= 1e6 and the
rounding of x alone is 2u * 1e6 = 2.2e-10 -- times pi'(1 - pi'), which is what a change of x does to a softmax, and at that scale
the softmax is one-hot to within e^-1e4 unless two q are equal.  1e-9 is above every one of these, 10^4 times above the bound of the
ordinary cases; the gaps measured on the cases are 1e-6 and more.
An exact tie is allowed only between children whose x(a) and n(a) are identical: the device computes identical scores for them too,
and the first index wins on both sides.  inner_pick asserts that."""
import functools
import math

import numpy as np

from oracle import oracle as O
import gumbel_ref as GR

F32 = np.float32
FLAG_FAST, FLAG_GUMBEL, FLAG_FULL = 1, 4, 8
MISTAKES = ("interior_puct", "no_vhat", "vhat_sign", "n_over_S", "no_sigma", "parent_vhat")


# ---- 1. the rule on one node ------------------------------------------------------------------------------------------------------
def v_mix_full(vhat, P, q, n):
    S = int(sum(int(x) for x in n))
    num = GR.rule_sum([float(P[a]) * q[a] if n[a] > 0 else 0.0 for a in range(len(n))])
    den = GR.rule_sum([float(P[a]) if n[a] > 0 else 0.0 for a in range(len(n))])
    return (float(vhat) + float(S) * (num / den)) / (1.0 + float(S)) if den != 0.0 else float(vhat)


def sigmas_full(c_visit, c_scale, vhat, P, W, n, sgn, valid):
    q = GR.q_values(W, n, sgn)
    vm = v_mix_full(vhat, P, q, n)
    n_max = max([int(n[a]) for a in range(len(n)) if valid[a]] or [0])
    return [((c_visit + float(n_max)) * c_scale) * (q[a] if n[a] > 0 else vm) for a in range(len(n))]


def improved_policy(c_visit, c_scale, vhat, P, W, n, sgn, valid, sigma=True):
    """(the candidates, x(a) of each, float64 [A] pi' with 0.0 for every other child)"""
    A = len(P)
    C = GR.candidates(P, valid)
    sg = sigmas_full(c_visit, c_scale, vhat, P, W, n, sgn, valid) if sigma else [0.0] * A
    x = {a: GR.logit(P[a]) + sg[a] for a in C}
    M = max(x.values())
    e = [math.exp(x[a] - M) if a in x else 0.0 for a in range(A)]
    se = GR.rule_sum(e)
    return C, x, [e[a] / se if a in x else 0.0 for a in range(A)]


def nonroot_scores(c_visit, c_scale, vhat, P, W, n, sgn, valid, mistake=None):
    """[(a, score, x(a), n(a))] over the candidates in index order"""
    v = 0.0 if mistake == "no_vhat" else (-float(vhat) if mistake == "vhat_sign" else float(vhat))
    C, x, pi = improved_policy(c_visit, c_scale, v, P, W, n, sgn, valid, sigma=mistake != "no_sigma")
    S = int(sum(int(k) for k in n))
    if mistake == "n_over_S":
        return [(a, pi[a] - (float(n[a]) / float(S) if S else 0.0), x[a], int(n[a])) for a in C]
    return [(a, pi[a] - float(n[a]) / (1.0 + float(S)), x[a], int(n[a])) for a in C]


def nonroot_pick(c_visit, c_scale, vhat, P, W, n, sgn, valid):
    sc = nonroot_scores(c_visit, c_scale, vhat, P, W, n, sgn, valid)
    best = max(s for _, s, _, _ in sc)
    return next(a for a, s, _, _ in sc if s == best)


def target_full(c_visit, c_scale, vhat, P, W, n, sgn, valid):
    C, _, pi = improved_policy(c_visit, c_scale, vhat, P, W, n, sgn, valid)
    out = np.zeros(len(P), np.int32)
    for a in C:
        out[a] = int(math.floor(pi[a] * 16777216.0 + 0.5))
    return out


# ---- 2. the search ----------------------------------------------------------------------------------------------------------------
class Tree(GR.Tree):
    """gumbel_ref.Tree with the rule below the root and the full v_mix at it.  run() plays on a subclass of its own that carries
    full_mistake and fstats."""
    full_mistake = None
    fstats = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.vhat = {}  # node -> the float32 value it got at its expansion

    def select_leaf(self, k, mistake):
        self._leaf, path = super().select_leaf(k, mistake)
        return self._leaf, path

    def search_once(self, ev, k=0.0, mistake=None):
        got = []

        def ev2(d, st):
            p, v = ev(d, st)
            got.append(F32(np.asarray(v).ravel()[0]))
            return p, v

        super().search_once(ev2, k, mistake)
        if not self._leaf.terminal:
            self.vhat[self._leaf] = got[0]

    def best_child(self, n, k, mistake):
        if self.gum is not None and n is not self.first and self.full_mistake != "interior_puct":
            return self.inner_pick(n)
        return super().best_child(n, k, mistake)

    def node_vhat(self, n):
        if self.full_mistake == "parent_vhat" and n.parent is not None:
            return self.vhat[n.parent]
        return self.vhat[n]

    def inner_pick(self, n):
        G, st = self.gum, self.fstats
        sc = nonroot_scores(G["c_visit"], G["c_scale"], self.node_vhat(n), n.priors, n.W, n.N, n.changed, n.valid, self.full_mistake)
        best = max(s for _, s, _, _ in sc)
        top = [(x, k) for _, s, x, k in sc if s == best]
        assert all(t == top[0] for t in top), ("an exact tie between children whose x and n differ", sc)
        lower = [s for _, s, _, _ in sc if s < best]
        if lower:
            st["gaps"].append(best - max(lower))
        st["picks"] += 1
        st["deep"] += (n.deepness - self.first.deepness) >= 3
        st["visited"] += bool(n.N.sum() > 0)
        return next(a for a, s, _, _ in sc if s == best)

    def _root_sigmas(self, c_visit, c_scale, P, W, n, sgn, valid, mistake=None):
        """gumbel_ref.sigmas of the root (its pick, its move and its target call it) with the full v_mix"""
        v = self.vhat[self.first]
        v = 0.0 if self.full_mistake == "no_vhat" else (-float(v) if self.full_mistake == "vhat_sign" else float(v))
        return sigmas_full(c_visit, c_scale, v, P, W, n, sgn, valid)

    def gsearch(self, *a, **kw):
        saved = GR.sigmas
        GR.sigmas = self._root_sigmas
        try:
            return super().gsearch(*a, **kw)
        finally:
            GR.sigmas = saved


# ---- 3. the game ------------------------------------------------------------------------------------------------------------------
def run(d, *, mistake=None, **kw):
    """gumbel_ref._run(d, **kw) in the full mode.  Further keys: min_gap covers the interior picks too; interior_picks, deep_picks
    (at depth >= 3 below the root) and visited_picks (at nodes with S > 0); flags carry bit 3."""
    assert mistake is None or mistake in MISTAKES
    stats = dict(gaps=[], picks=0, deep=0, visited=0)
    cls = type("FullTree", (Tree,), dict(full_mistake=mistake, fstats=stats))
    saved = GR.Tree
    GR.Tree = cls
    try:
        res = GR._run(d, **kw)
    finally:
        GR.Tree = saved
    res["flags"] = res["flags"] | FLAG_FULL
    res.update(min_gap=min([res["min_gap"]] + stats["gaps"]), interior_picks=stats["picks"], deep_picks=stats["deep"],
               visited_picks=stats["visited"])
    return res


def play_game(d, *, g_mode, game_idx, mistake=None, **kw):
    gv = GR.gumbel_vectors(np.random.RandomState(1000 + int(game_idx))) if g_mode == "script" else None
    return run(d, mistake=mistake, game_idx=game_idx, g_vectors=gv, **kw)


SEED = GR.SEED
C_VISIT, C_SCALE = GR.C_VISIT, GR.C_SCALE
CASES = [
    # name, rows, cols, reads, m, reuse, cap, g, evaluator, games, c_visit, c_scale
    ("3x3-script-m4", 3, 3, 32, 4, True, None, "script", "formula", 8, C_VISIT, C_SCALE),
    ("3x3-philox-m16-noreuse", 3, 3, 16, 16, False, None, "philox", "formula", 8, C_VISIT, C_SCALE),
    ("3x3-philox-m2-cap", 3, 3, 32, 2, True, (0.5, 8), "philox", "formula", 8, C_VISIT, C_SCALE),
    ("6x6-philox-m16", 6, 6, 32, 16, True, None, "philox", "formula", 2, C_VISIT, C_SCALE),
    ("2x7-philox-m3", 2, 7, 16, 3, True, None, "philox", "formula", 4, C_VISIT, C_SCALE),
    ("8x8-philox-m2", 8, 8, 16, 2, True, None, "philox", "formula", 1, C_VISIT, C_SCALE),
    ("10x10-philox-m2", 10, 10, 16, 2, True, None, "philox", "formula", 1, C_VISIT, C_SCALE),
    ("3x3-philox-m4-cvisit0-cscale0.1", 3, 3, 32, 4, True, None, "philox", "formula", 8, 0.0, 0.1),
    ("3x3-philox-m4-cvisit1e6", 3, 3, 32, 4, True, None, "philox", "formula", 8, 1e6, 1.0),
]
CASE_IDS = [c[0] for c in CASES]
# the cases each deliberate mistake must change at least half of the games of
MISTAKE_CASES = {
    "interior_puct": ("3x3-script-m4", "6x6-philox-m16"),
    "no_vhat": ("3x3-script-m4",),
    "vhat_sign": ("3x3-script-m4",),
    "n_over_S": ("3x3-script-m4",),
    "no_sigma": ("3x3-script-m4",),
    "parent_vhat": ("3x3-script-m4", "6x6-philox-m16"),
}


def case(name):
    return next(c for c in CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def case_games(name, mistake=None, full=True):
    """the games of a case, computed once and shared (callers leave them unchanged); full=False: the root-only rule of gumbel_ref"""
    _, R, Cc, sims, m, reuse, cap, g_mode, ev, games, c_visit, c_scale = case(name)
    d = O.dims(R, Cc)
    kw = dict(seed=SEED, sims=sims, reuse=reuse, gumbel=(m, c_visit, c_scale), cap=cap, base_ev=GR.KIND[ev])
    if not full:
        return [GR.play_game(d, g_mode=g_mode, game_idx=gi, **kw) for gi in range(games)]
    return [play_game(d, g_mode=g_mode, game_idx=gi, mistake=mistake, **kw) for gi in range(games)]


def games_differ(a, b):
    """do two games differ in a move or in a recorded target"""
    return a["n_rows"] != b["n_rows"] or not np.array_equal(a["played"], b["played"]) or not np.array_equal(a["visits"], b["visits"])


# ---- the network cases (test_hip_gumbel_full_net.py plays these; the reference's evaluator there is the engine itself) ------------------
NET_SEED = {(3, 3): 1, (6, 6): 1, (8, 8): 1, (10, 10): 1}  # torch.manual_seed of the board's network: picked so that the gap condition holds
NET = {
    # slots: above 16 and no multiple of 16 (the full-rounds cut needs n_slots > eval_round); games = slots; replay: fixed game indices.
    # m is below the reads on every board, so that simulations get past the root's children
    (3, 3): dict(slots=40, sims=32, m=4, replay=(0, 11, 22, 39)),
    (6, 6): dict(slots=24, sims=16, m=4, replay=(3, 20)),
    (8, 8): dict(slots=24, sims=16, m=2, replay=(17,)),
    (10, 10): dict(slots=24, sims=16, m=2, replay=(6,)),
}


def network(R, C):
    """the small seeded random network of gumbel_ref.network, with this module's seed"""
    import torch
    from dotsboxesaz_amd import nn as dnn
    torch.manual_seed(NET_SEED[(R, C)])
    return dnn.ResNetZero(dnn.resnet_params(R, C, 32, 2, 4, 8))


# ---- the rule next to the other self-play features (test_hip_gumbel_full_features.py plays these; formula evaluators) ------------------
FEATURES = {
    # table: the Endgame's max_free; leaf: the leaf solver's L; starts: the openings' lengths (games_per_start = 2)
    "3x3-table": dict(R=3, C=3, sims=32, m=4, reuse=True, g="philox", games=8, slots=8, table=8),
    "3x3-leaf": dict(R=3, C=3, sims=32, m=4, reuse=True, g="philox", games=8, slots=8, leaf=6),
    "3x3-start": dict(R=3, C=3, sims=32, m=4, reuse=True, g="philox", games=6, slots=8, starts=(1, 4, 6)),
}
FEATURE_IDS = list(FEATURES)


def feature_book(name):
    f = FEATURES[name]
    return GR.openings(O.dims(f["R"], f["C"]), len(f["starts"]), f["starts"]) if "starts" in f else None


@functools.lru_cache(maxsize=None)
def feature_games(name, full=True):
    """{game index: the game} of a case of FEATURES and its LeafSolver (or None), computed once and shared (callers leave them
    unchanged); full=False: the root-only rule"""
    import endgame_selfplay_ref as ESR
    import leaf_solve_ref as LSR
    f = FEATURES[name]
    d = O.dims(f["R"], f["C"])
    tab = ESR.Table(f["R"], f["C"], f["table"], GR.TABLE_SEED) if "table" in f else None
    w = LSR.LeafSolver(f["R"], f["C"], f["leaf"], GR.TABLE_SEED, 0) if "leaf" in f else None
    book = feature_book(name)
    out = {}
    for gi in range(f["games"]):
        start = book[GR.start_of(gi, len(book), 2)] if book else ()
        kw = dict(g_mode=f["g"], game_idx=gi, seed=SEED, sims=f["sims"], reuse=f["reuse"], gumbel=(f["m"], C_VISIT, C_SCALE),
                  base_ev=w if w is not None else 0, start=start, table=tab)
        out[gi] = play_game(d, **kw) if full else GR.play_game(d, **kw)
    return out, w
