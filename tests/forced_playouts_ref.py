"""Forced playouts and policy target pruning restated on the CPU (helper of test_forced_playouts_ref_cpu.py and
test_hip_forced_playouts.py).  Three parts:

1. The sequential search (one pending evaluation) in Python, written from DESIGN.md section 1 "Semantics restated" and
   oracle/dbaz_oracle.c: float32 child_total_value, int32 visits, the UCB in float64 in the descent's operation order, numpy's
   pairwise prior sums (O.np_sum_f32 / f64), math.log and math.sqrt (libm, as the oracle and the engine's tables use it), the
   first-maximum argmax, the virtual loss, the root-noise mix, and tree reuse with a fresh root slot.  Evaluators are callables
   ev(d, state) -> (p float32 [A], v float32).  With k = 0 it is O.Tree.search + advance bit for bit (pinned by the CPU test).
2. The rule: forced() and prune(), written from the comment of dbaz_selfplay_set_forced_playouts in include/dbaz.h alone.
3. The game loop, in the shape of playout_cap_ref._run (same keys, same rows_differ; cap= through playout_cap_ref.is_full), with
   generate_game / replay_game and a mistake= switch for the helper's own tests."""
import math

import numpy as np

from oracle import oracle as O
import endgame_selfplay_ref as ESR
import playout_cap_ref as PCR

CPUCT = (1.25, 19652)
MISTAKES = ("forced_below_root", "forced_unvisited_too", "N_off_by_one", "prune_best_too", "prune_before_move_choice", "forced_on_fast")
F32 = np.float32


def formula(kind):
    return lambda d, st: O.eval_formula(d, st, kind)


# ---- 1. the search ---------------------------------------------------------------------------------------------------------
class Node:
    __slots__ = ("st", "move", "parent", "tree", "expanded", "terminal", "deepness", "children", "priors", "priors_f64", "W", "N",
                 "changed", "valid", "invalid")

    def __init__(self, tree, st, move, parent):
        A = tree.d.A
        self.st, self.move, self.parent = st, move, parent
        self.tree = None if parent is not None else tree
        self.expanded = False
        self.terminal = O.get_result(st) is not None
        self.children = {}
        self.priors = np.zeros(A, np.float64)
        self.priors_f64 = False
        self.W = np.zeros(A, np.float32)
        self.N = np.zeros(A, np.int32)
        self.changed = np.ones(A, np.int32)
        self.valid = O.valid_moves(tree.d, st).astype(bool)
        self.invalid = np.where(self.valid, 0.0, 1.0)
        self.deepness = (parent.deepness if parent is not None else 0) + 1

    def get_tv(self):
        return self.parent.W[self.move] if self.parent is not None else self.tree.tv_none

    def set_tv(self, v):
        if self.parent is not None:
            self.parent.W[self.move] = v
        else:
            self.tree.tv_none = F32(v)

    def get_nv(self):
        return int(self.parent.N[self.move]) if self.parent is not None else self.tree.nv_none

    def set_nv(self, v):
        if self.parent is not None:
            self.parent.N[self.move] = v
        else:
            self.tree.nv_none = int(v)


def pbc_sq(N, cpuct=CPUCT):
    """the two N-dependent terms of the UCB (mcts.py:92-94), from libm"""
    return math.log((float(N) + cpuct[1] + 1.0) / cpuct[1]) + cpuct[0], math.sqrt(float(N))


def forced(k, P, n, N):
    """bool [A]: the forced test of the header on every child (validity is the caller's)"""
    n = np.asarray(n)
    nf = n.astype(np.float64)
    return (n > 0) & (nf * nf < k * np.asarray(P, np.float64) * float(N))


class Tree:
    """create_root_uct_node / UCT_search / init_mcts_tree, one pending evaluation; forcing by `k` at the root"""

    def __init__(self, d, state, cpuct=CPUCT):
        self.d, self.cpuct = d, cpuct
        self.tv_none, self.nv_none, self.pc_none = F32(0.0), 0, 0
        self.deepness_correction = self.max_deepness = self.terminal_count = self.tree_size = 0
        self.n_search = 0
        self.first = Node(self, state.copy(), -1, None)

    # -- descent
    def best_child(self, n, k, mistake):
        N = n.get_nv()
        pbc0, sq = pbc_sq(N, self.cpuct)
        t = sq / (n.N + 1).astype(np.float64)
        pb_c = pbc0 * t
        prior_score = pb_c * n.priors
        value_score = n.W.astype(np.float64) / (1 + n.N).astype(np.float64)
        value_score = value_score * n.changed.astype(np.float64)
        score = prior_score + value_score
        x = -1e12 * n.invalid + score
        if k > 0 and (n is self.first or mistake == "forced_below_root"):
            vis = n.N
            f = forced(k, n.priors, vis, N + 1 if mistake == "N_off_by_one" else N)
            if mistake == "forced_unvisited_too":
                f = f | ((vis == 0) & (0.0 < k * n.priors * float(N)))
            x = np.where(f & n.valid, 1e20, x)
        return int(np.argmax(x))  # first maximum; the first NaN wins

    def select_leaf(self, k, mistake):
        cur = self.first
        path = [cur]
        while cur.expanded and not cur.terminal:
            cur.set_tv(F32(cur.get_tv()) - F32(1.0))  # VIRTUAL_LOSS
            bm = self.best_child(cur, k, mistake)
            if bm not in cur.children:
                st = cur.st.copy()
                O.play_(self.d, st, bm)
                cur.children[bm] = Node(self, st, bm, cur)
            cur = cur.children[bm]
            path.append(cur)
        return cur, path

    def search_once(self, ev, k=0.0, mistake=None):
        leaf, path = self.select_leaf(k, mistake)
        A = self.d.A
        if not leaf.terminal:
            p, v = ev(self.d, leaf.st)
            p = np.asarray(p, np.float32) * np.where(leaf.valid, F32(1.0), F32(0.0))
            vf = F32(v)
            s = O.np_sum_f32(p)
            if s > 0 and s != F32(1.0):
                p = p / s
        else:
            p = np.zeros(A, np.float32)
            vf = F32(O.get_result(leaf.st))
        leaf.expanded = True
        leaf.priors = p.astype(np.float64)
        leaf.priors_f64 = leaf.terminal
        sw = 1 if leaf.st.to_play == leaf.st.just_played else -1
        if leaf.parent is not None:
            leaf.parent.changed[leaf.move] = sw
        else:
            self.pc_none = sw
        to_play = leaf.st.to_play
        for nd in path:
            v = vf if nd.st.to_play == to_play else -vf
            add = F32(v + F32(1.0))
            nd.set_tv(F32(nd.get_tv()) + add)
            nd.set_nv(nd.get_nv() + 1)
        self.terminal_count += int(leaf.terminal)
        self.max_deepness = max(self.max_deepness, leaf.deepness)
        self.n_search += 1

    def prep_root(self, dirichlet, noise):
        """root prior renormalisation + Dirichlet mix, mcts.py:211-226"""
        root = self.first
        alpha, coeff = float(dirichlet[0]), float(dirichlet[1])
        if not root.priors_f64:
            pf = root.priors.astype(np.float32)
            cpsum = O.np_sum_f32(pf)
            if cpsum != 0:
                probs, probs_f64 = (pf / cpsum).astype(np.float64), False
            else:
                probs, probs_f64 = np.zeros_like(root.priors), True
        else:
            cpsum = O.np_sum_f64(root.priors)
            probs, probs_f64 = (root.priors / cpsum if cpsum != 0 else np.zeros_like(root.priors)), True
        onemc = 1.0 - coeff
        if alpha > 0:
            nz = np.asarray(noise, np.float64) * np.where(root.valid, 1.0, 0.0)
            a = onemc * probs if probs_f64 else (F32(onemc) * probs.astype(np.float32)).astype(np.float64)
            root.priors = a + coeff * nz
            root.priors_f64 = True
        else:
            cn = coeff * 0.0
            if probs_f64:
                root.priors = onemc * probs + cn
            else:
                root.priors = (F32(onemc) * probs.astype(np.float32) + F32(cn)).astype(np.float64)
            root.priors_f64 = probs_f64

    def search(self, num_reads, ev, dirichlet=(0.0, 0.0), noise=None, k=0.0, mistake=None):
        if not self.first.expanded:
            self.search_once(ev)
        self.prep_root(dirichlet, noise)
        for _ in range(int(num_reads)):
            self.search_once(ev, k, mistake)
        return self.first.N.copy()

    # -- init_mcts_tree
    def advance(self, move, reuse_tree=True):
        prev = self.first
        if move not in prev.children:
            st = prev.st.copy()
            O.play_(self.d, st, move)  # ValueError for an illegal move
            prev.children[move] = Node(self, st, move, prev)
        nxt = prev.children[move]
        self.tv_none, self.nv_none, self.pc_none = F32(0.0), 0, 0  # a fresh root slot either way
        self.max_deepness = self.terminal_count = 0
        if reuse_tree:
            nxt.parent, nxt.tree = None, self
            self.first = nxt
            self.deepness_correction = nxt.deepness
            self.tree_size = int(prev.N[move])
        else:
            self.first = Node(self, nxt.st.copy(), -1, None)
            self.first.move = move
            self.deepness_correction = self.tree_size = 0

    # -- what the oracle's Tree hands out
    @property
    def state(self):
        return self.first.st.copy()

    @property
    def is_terminal(self):
        return self.first.terminal

    @property
    def is_expanded(self):
        return self.first.expanded

    def root_arrays(self):
        r = self.first
        return r.priors.copy(), r.W.copy(), r.N.copy(), r.changed.copy()

    def stats(self):
        return (self.max_deepness - self.deepness_correction, self.tree_size, self.terminal_count,
                F32(self.tv_none) / F32(1 + self.nv_none))


# ---- 2. the rule's second half -------------------------------------------------------------------------------------------
def forced_count(k, P, N):
    """the smallest integer f >= 0 with f * f >= k P N"""
    t = k * float(P) * float(N)
    f = 0
    while float(f) * float(f) < t:
        f += 1
    return f


def prune(k, pbc, sq, N, P, W, n, sgn, valid, mistake=None):
    """int32 [A]: n' of every child, steps 1-4 of the header by plain scans.  sgn: +1 / -1 per child (child_player_changed)."""
    n = np.asarray(n).astype(np.int64)
    out = n.copy()
    cand = [i for i in range(len(n)) if valid[i]]
    if not cand:
        return out.astype(np.int32)

    def value(c):
        return (float(W[c]) / float(1 + n[c])) * float(sgn[c])

    def expl(c, m):
        return (pbc * (sq / float(m + 1))) * float(P[c])

    cs = max(cand, key=lambda i: (n[i], -i))  # the first valid child with the most visits
    ustar = expl(cs, n[cs]) + value(cs)
    for c in cand:
        if n[c] <= 0:
            continue
        f = forced_count(k, P[c], N)
        lo = max(0, int(n[c]) - f)
        if c == cs:
            if mistake == "prune_best_too":
                out[c] = lo
            continue
        m = next((m for m in range(lo, int(n[c]) + 1) if expl(c, m) + value(c) < ustar), int(n[c]))
        if m < n[c] and m == 1:
            m = 0
        out[c] = m
    return out.astype(np.int32)


def prune_root(t, k, mistake=None):
    """prune() on the root of a Tree after its search; also the arguments, for a comparison with dbaz_prune_visits"""
    P, W, n, sgn = t.root_arrays()
    N = t.nv_none
    pbc, sq = pbc_sq(N, t.cpuct)
    args = dict(k=k, pbc=pbc, sq=sq, root_N=N, P=P, W=W, n=n, same=sgn > 0, valid=t.first.valid.copy())
    return prune(k, pbc, sq, N, P, W, n, sgn, t.first.valid, mistake), args


# ---- 3. the game ----------------------------------------------------------------------------------------------------------
def _run(d, choose, *, seed, game_idx, sims, reuse, noise=(0.0, 0.0), vectors=None, cap=None, base_ev=0, start=(), forced_playouts=None,
         mistake=None, on_root=None):
    """one game; choose(i, visits) -> the move of ply i from the RAW visits.  forced_playouts: (k, prune) or None.  vectors, cap:
    as in playout_cap_ref._run.  on_root(tree, full, active): called after every search, before the row.  Keys of the result: those
    of playout_cap_ref._run, plus raw_visits, pruned (the row's flag), and the sums rows_pruned / visits_pruned."""
    assert mistake is None or mistake in MISTAKES
    ev = formula(base_ev) if isinstance(base_ev, int) else base_ev
    k, do_prune = (float(forced_playouts[0]), bool(forced_playouts[1])) if forced_playouts else (0.0, False)
    if not k > 0:
        k, do_prune = 0.0, False
    t = Tree(d, O.state_from_moves(d, list(start)))
    keys = ("x", "player", "visits", "pi", "q_value", "max_deepness", "tree_size", "terminal_count", "played", "reads", "full", "served",
            "raw_visits", "pruned")
    out = {key: [] for key in keys}
    vecs = []
    n_search, i, rows_pruned, visits_pruned = 0, 0, 0, 0
    while not t.is_terminal:
        st = t.state
        valid = t.first.valid
        reads = ESR._fact_reads(int(valid.sum()), sims)
        full = cap is None or PCR.is_full(seed, game_idx, i, cap[0])
        if not full:
            reads = min(reads, cap[1])
        vec = vectors(i, valid) if noise[0] > 0 else None
        vecs.append(vec)
        noisy = noise[0] > 0 and full
        active = k > 0 and (full or mistake == "forced_on_fast")
        expanded = t.is_expanded
        raw = t.search(reads, ev, dirichlet=tuple(noise) if noisy else (0.0, 0.0), noise=vec if noisy else None, k=k if active else 0.0,
                       mistake=mistake)
        n_search += reads + (0 if expanded else 1)
        if on_root is not None:
            on_root(t, full, active)
        md, ts, tc, q = t.stats()
        vis, pruned = raw, False
        if active and do_prune:
            vis, _ = prune_root(t, k, mistake)
            pruned = True
            rows_pruned += 1
            visits_pruned += int(raw.sum() - vis.sum())
        move = int(choose(i, vis if mistake == "prune_before_move_choice" else raw))
        s = int(vis.sum())
        row = dict(x=O.features(d, st).ravel(), player=st.to_play, visits=vis, pi=vis.astype(np.float64) / (s if s else 1.0),
                   q_value=np.float32(q), max_deepness=md, tree_size=ts, terminal_count=tc, played=move, reads=reads, full=full,
                   served=False, raw_visits=raw, pruned=pruned)
        for key, v in row.items():
            out[key].append(v)
        t.advance(move, reuse)
        i += 1
    res = {key: np.array(v) for key, v in out.items()}
    res["x"] = res["x"].astype(np.int16).reshape(len(out["x"]), -1)
    term = t.state
    zt = O.get_result(term)
    res["z"] = np.array([zt if p == term.just_played else -zt for p in out["player"]], np.int64)
    res.update(n_rows=i, n_search=n_search, vectors=np.array(vecs, np.float64) if noise[0] > 0 else None, rows_pruned=rows_pruned,
               visits_pruned=visits_pruned)
    return res


def generate_game(d, rs, **kw):
    """a game by these rules with the moves sampled from the raw visits (temperature 1) by the RandomState rs -- and, with noise,
    its per-ply vectors drawn from rs too (result["vectors"])"""
    if kw.get("noise", (0.0, 0.0))[0] > 0 and "vectors" not in kw:
        kw["vectors"] = PCR.dirichlet_vectors(rs, kw["noise"][0])
    return _run(d, lambda i, vis: rs.choice(len(vis), p=vis / vis.sum()), **kw)


def replay_game(d, played, vectors=None, **kw):
    """the game with the moves `played` teacher-forced, its noise vectors (float64 [plies, A]) scripted"""
    played = np.asarray(played).astype(np.int64)
    return _run(d, lambda i, vis: played[i], vectors=(lambda i, valid: np.asarray(vectors[i], np.float64)) if vectors is not None else None, **kw)


def rows_differ(ref, rows):
    """the first row at which a game of this module and `rows` (arrays in move order: x, player, visits, pi, q_value, TreeStats,
    z, played) differ bit for bit, or -1"""
    return ESR.rows_differ(ref, rows)
