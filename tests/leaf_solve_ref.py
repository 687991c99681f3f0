"""The leaf solver's rule replayed on the oracle (helper of test_leaf_solve_ref_cpu.py / test_hip_leaf_solve.py), written from
include/dbaz.h (dbaz_attach_leaf_solver) on top of endgame_selfplay_ref.py and slot_tables_ref.SlotTablesRef.

LeafSolver.evaluate(d, state) is an evaluator for oracle.Tree: an unfinished state with F <= L free real edges gets the one-hot p
and the v of that position's own table (SlotTablesRef(R, C, x[None], seed, 16).one(x): dbaz_exact_policy's answer), every other
state the base evaluator's.  Passed as base_ev to endgame_selfplay_ref's game loop it gives the rule of the header: inside a
table-served search that loop asks the table, everywhere else this wrapper -- the rule looks at the leaf alone.

The game loop (endgame_selfplay_ref._run, unchanged) calls choose(row, visits) once per move, after the move's search: replay()
and generate() hook the wrapper in there.  It keeps the game's state itself and so knows, for the NEXT search, the root's F (the
per-row counts of solved leaves; the deliberate mistake "root") and, in match play, the searching model -- the loop ignores
base_ev under models=, so the match is run without models= and the evaluator of each move is chosen here."""
import numpy as np

from oracle import oracle as O
import endgame_selfplay_ref as SR
from slot_tables_ref import SlotTablesRef

MISTAKES = ("off_by_one", "root", "seed", "sign")


class LeafSolver:
    """base: a formula kind (int), an evaluate(d, state), or in match play a pair of those, one per model.
    leaf_models: the models the solver is attached to (match play).  mistake: one of MISTAKES, for the helper's own tests."""

    def __init__(self, R, C, L, seed=0, base=0, *, match=False, leaf_models=(0,), mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.R, self.C, self.L, self.seed, self.match, self.leaf_models, self.mistake = R, C, int(L), int(seed), match, tuple(leaf_models), mistake
        bases = list(base) if isinstance(base, (tuple, list)) else [base, base]
        self.base = [SR.formula(b) if isinstance(b, int) else b for b in bases]
        self.calls = {"base": 0, "solved": 0}
        self.by_free = [0] * 17
        self.games = []  # per finished game: dict(root_F, solved) per row
        self.state = None

    # ---- the game's own state: what the next search's root is
    def start_game(self, d, game_idx=0):
        self.d, self.game_idx, self.state = d, int(game_idx), O.new_state(d)
        self.rows = dict(root_F=[], solved=[])
        self.games.append(self.rows)
        self._root()

    def _root(self):
        self.root_F = int(O.valid_moves(self.d, self.state).sum())
        self.model = (self.state.to_play ^ (self.game_idx & 1)) & 1 if self.match else 0
        self._solved_before = self.calls["solved"]

    def after_search(self, move):
        self.rows["root_F"].append(self.root_F)
        self.rows["solved"].append(self.calls["solved"] - self._solved_before)
        O.play_(self.d, self.state, int(move))
        self._root()

    # ---- the evaluator
    def solve(self, d, st):
        x = O.features(d, st).ravel()
        seed = self.seed + 1 if self.mistake == "seed" else self.seed
        a, v, served = SlotTablesRef(self.R, self.C, x[None], seed, 16).one(x)
        assert served and a >= 0
        p = np.zeros(d.A, np.float32)
        p[a] = 1.0
        return p, np.float32(-v if self.mistake == "sign" else v)

    def evaluate(self, d, st):
        F = int(O.valid_moves(d, st).sum())
        L = self.L - 1 if self.mistake == "off_by_one" else self.L
        decides = self.root_F if self.mistake == "root" else F
        if self.model in self.leaf_models and O.get_result(st) is None and decides <= L:
            self.calls["solved"] += 1
            self.by_free[F] += 1
            return self.solve(d, st)
        self.calls["base"] += 1
        return self.base[self.model](d, st)

    def solved_under_high_roots(self):
        """per game: the leaves solved in searches whose root had F > L"""
        return [sum(s for f, s in zip(g["root_F"], g["solved"]) if f > self.L) for g in self.games]


def _play(d, w, choose, table, game_idx, **kw):
    w.start_game(d, game_idx)

    def hooked(i, vis):
        move = int(choose(i, vis))
        if move >= 0:
            w.after_search(move)
        return move
    return SR._run(d, hooked, w.evaluate, table, **kw)


def replay(d, rows_of_game, w, table=None, *, sims, reuse, stop_at_mismatch=False, **kw):
    """endgame_selfplay_ref.replay_game with w (a LeafSolver) as the evaluator of every search no table serves; in match play
    (w.match) the model of a move is root_to_play ^ (game_idx & 1), the game's number read from rows_of_game["game_idx"].
    The result's base_calls are the wrapper's calls, solved ones included: w.calls splits them."""
    played = np.asarray(rows_of_game["played"]).astype(np.int64)
    game_idx = int(np.asarray(rows_of_game["game_idx"]).ravel()[0]) if w.match else 0
    return _play(d, w, lambda i, vis: played[i] if i < len(played) else -1, table, game_idx, sims=sims, reuse=reuse,
                 expect=rows_of_game if stop_at_mismatch else None, **kw)


def generate(d, rs, w, table=None, *, sims, reuse, game_idx=0, **kw):
    """endgame_selfplay_ref.generate_game likewise: the moves sampled from pi by the RandomState rs"""
    return _play(d, w, lambda i, vis: rs.choice(len(vis), p=vis / vis.sum()), table, game_idx, sims=sims, reuse=reuse, **kw)
