"""Self-play with an endgame table inside the search, replayed on the oracle (helper of test_endgame_selfplay_ref_cpu.py /
test_hip_endgame_selfplay.py), written from include/dbaz.h (dbaz_attach_endgame, dbaz_attach_tables, dbaz_attach_tables_pool) on
top of oracle.Tree and slot_tables_ref.SlotTablesRef.

A finished game is replayed move by move on one O.Tree, teacher-forced with the moves that were played (the loop of
test_selfplay_driver_in_waves_vs_oracle_wave_search), and the evaluator is chosen PER MOVE by the search ROOT: the search of a
move whose root has F <= max_free free real edges is SERVED -- every leaf it expands, whatever its own F, gets the (p, v) of the
game's table -- and every other search runs with the model's own evaluator.  The tree is the oracle's and knows nothing of this:
with tree reuse a served search descends through nodes that the other evaluator expanded and adds leaves from the table.  The
transposition table needs no counterpart here: it hands a leaf the (p, v) its evaluator would give (utils/proxies.py:35-43).

A game has one table, rooted at its first served root; which root a table has cannot matter (D depends on the free edges only),
so a slot that was denied a region and got one at a later move (served_from) is covered by the same code."""
import numpy as np

from oracle import oracle as O
import endgame_ref as ER
from slot_tables_ref import SlotTablesRef

NEVER = 1 << 30  # served_from of a game that never gets a table


class Table:
    """what an attach fixes: the threshold and the seed that picks among equally good moves; max_free < 0: no attach"""

    def __init__(self, rows, cols, max_free, seed=0):
        self.R, self.C, self.max_free, self.seed = rows, cols, int(max_free), int(seed)


def _fact_reads(n_valid, sims):
    """n_searches = min(4 * factorial(nb_valid_moves), mcts_num_read), self_play.py:64-65"""
    f = 4.0
    for i in range(2, n_valid + 1):
        f *= i
        if f > sims:
            break
    return int(f) if f < sims else sims


def formula(kind):
    """the formula evaluator `kind` (0 = hash, 1 = uniform) as a python evaluate(d, state) -> (p, v)"""
    return lambda d, st: O.eval_formula(d, st, kind)


class _Game:
    """the evaluators of one game: base (per model) and the table, switched per move; counts the calls of either"""

    def __init__(self, d, base, table, models):
        self.d, self.table, self.models = d, table, models
        self.calls = {"base": 0, "table": 0}
        self.ref = None   # SlotTablesRef of the game, built at the first served root
        self.use_table, self.model = False, 0
        if models is not None:
            self.base = [formula(models[0]), formula(models[1])]
        else:
            self.base = [formula(base) if isinstance(base, int) else base] * 2
        self.ev = O.Evaluator(self._evaluate)

    def _evaluate(self, d, st):
        if not self.use_table:
            self.calls["base"] += 1
            return self.base[self.model](d, st)
        self.calls["table"] += 1
        a, v, served = self.ref.one(O.features(d, st).ravel())
        assert served and a >= 0, "a leaf of a served search that the game's table does not hold"
        p = np.zeros(d.A, np.float32)
        p[a] = 1.0
        return p, np.float32(v)


def _run(d, choose, base_ev, table, *, sims, reuse, K=1, served_from=None, endgame_reads=0, models=None, game_idx=0,
         fresh_at_first_served=False, expect=None):
    """one game from the empty board; choose(row index, visits) -> the move.  expect: rows to compare with while playing
    (dict of arrays in move order); the game stops at the first row that differs and the result says where."""
    g = _Game(d, base_ev, table, models)
    served_from = 0 if served_from is None else served_from
    t = O.Tree(d, O.new_state(d))
    out = {k: [] for k in ("x", "player", "visits", "pi", "q_value", "max_deepness", "tree_size", "terminal_count", "played", "reads",
                           "n_free", "served", "root_expanded")}
    n_search, first_served, mismatch = 0, -1, -1

    def is_served(st, i):
        F = int(O.valid_moves(d, st).sum())
        model = (st.to_play ^ (game_idx & 1)) & 1 if models is not None else 0
        ok = table is not None and F <= table.max_free and i >= served_from and (models is None or model in models[2])
        return F, model, ok

    i = 0
    while not t.is_terminal:
        st = t.state
        F, g.model, g.use_table = is_served(st, i)
        reads = _fact_reads(F, sims)
        if g.use_table:
            if first_served < 0:
                first_served = i
            if g.ref is None:
                g.ref = SlotTablesRef(table.R, table.C, O.features(d, st).ravel()[None], table.seed, table.max_free)
                assert len(g.ref.roots) == 1
            if endgame_reads > 0:
                reads = min(reads, endgame_reads)
        expanded = t.is_expanded
        before = t.counters()[0]
        vis = t.search(reads, g.ev, max_pending=K)
        # a root that the tree did not hold expanded costs one search more, which is none of the reads (mcts.py:207-208)
        assert t.counters()[0] - before == reads + (0 if expanded else 1)
        n_search += reads + (0 if expanded else 1)
        md, ts, tc, q = t.stats()
        s = int(vis.sum())
        row = dict(x=O.features(d, st).ravel(), player=st.to_play, visits=vis, pi=vis.astype(np.float64) / (s if s else 1.0),
                   q_value=np.float32(q), max_deepness=md, tree_size=ts, terminal_count=tc, reads=reads, n_free=F, served=g.use_table,
                   root_expanded=expanded)
        move = int(choose(i, vis))
        if move < 0:  # the game that is replayed ended here
            assert expect is not None, "the replayed game has fewer moves than the oracle's"
            mismatch = i
            break
        row["played"] = move
        for k, v in row.items():
            out[k].append(v)
        if expect is not None and not row_equal(row, expect, i):
            mismatch = i
            break
        keep = reuse
        if fresh_at_first_served and first_served < 0:
            nxt = st.copy()
            O.play_(d, nxt, move)
            if O.get_result(nxt) is None and is_served(nxt, i + 1)[2]:
                keep = False
        t.advance(move, keep)
        i += 1
    res = {k: np.array(v) for k, v in out.items()}
    res["x"] = res["x"].astype(np.int16).reshape(len(out["x"]), -1)
    res.update(n_rows=len(out["x"]), base_calls=g.calls["base"], table_calls=g.calls["table"], n_search=n_search,
               first_served=first_served, mismatch=mismatch)
    if mismatch < 0:
        # z: +z_T for rows whose to_play is the terminal state's just_played, -z_T otherwise (self_play.py:105-112)
        term = t.state
        zt = O.get_result(term)
        res["z"] = np.array([zt if p == term.just_played else -zt for p in out["player"]], np.int64)
    return res


COMPARED = ("x", "player", "visits", "pi", "q_value", "tree_size", "terminal_count", "max_deepness")


def row_equal(row, rows, i):
    """row (one replayed row) against row i of `rows` (arrays in move order), bit for bit in every compared field but z"""
    if i >= len(rows["played"]):
        return False
    for k in COMPARED:
        a, b = np.asarray(row[k]), np.asarray(rows[k][i])
        if k == "pi":
            a, b = a.astype(np.float64).view(np.uint64), b.astype(np.float64).view(np.uint64)
        elif k == "q_value":
            a, b = a.astype(np.float32).view(np.uint32), b.astype(np.float32).view(np.uint32)
        else:
            a, b = a.astype(np.int64), b.astype(np.int64)
        if not np.array_equal(a.ravel(), b.ravel()):
            return False
    return True


def rows_differ(ref, rows):
    """the first row at which a finished replay and `rows` (arrays in move order, with z) differ, or -1"""
    if ref["n_rows"] != len(rows["played"]):
        return min(ref["n_rows"], len(rows["played"]))
    for i in range(ref["n_rows"]):
        if not row_equal({k: ref[k][i] for k in COMPARED}, rows, i) or int(ref["z"][i]) != int(rows["z"][i]):
            return i
    return -1


def replay_game(d, rows_of_game, base_ev, table, *, sims, reuse, K=1, served_from=None, endgame_reads=0, models=None,
                fresh_at_first_served=False, stop_at_mismatch=False):
    """Replays one finished game, teacher-forced with rows_of_game["played"] (rows_of_game: dict of arrays in move order; match
    play reads the game's number from rows_of_game["game_idx"]).
      base_ev   the model's own evaluator: a formula kind (int) or evaluate(d, state) -> (p, v); ignored with models
      table     a Table (max_free, seed), or None
      sims      mcts_num_read: a move whose root has F free real edges searches min(4 * F!, sims) reads, a served search
                min(that, endgame_reads) when endgame_reads > 0
      K         max_pending: the searches run in waves of K
      served_from   only moves with index >= served_from are served (a slot that a dry pool denied a table until then)
      models    (kind0, kind1, endgame_models): match play with two formula evaluators; the model of a move is root_to_play ^
                (game_idx & 1), and its search is served only when that model is in endgame_models
      fresh_at_first_served   (a deliberate mistake for the helper's own tests) the first served search starts from a fresh root
      stop_at_mismatch        stop at the first row that differs from rows_of_game; result["mismatch"] is its index, else -1
    Returns a dict: per row x, player, visits, pi, q_value, max_deepness, tree_size, terminal_count, z (from the terminal state),
    reads, n_free, served, root_expanded; n_rows, base_calls, table_calls, n_search (searches, root expansions included),
    first_served (row index or -1)."""
    played = np.asarray(rows_of_game["played"]).astype(np.int64)
    game_idx = int(np.asarray(rows_of_game["game_idx"]).ravel()[0]) if models is not None else 0
    return _run(d, lambda i, vis: played[i] if i < len(played) else -1, base_ev, table, sims=sims, reuse=reuse, K=K, served_from=served_from,
                endgame_reads=endgame_reads, models=models, game_idx=game_idx, fresh_at_first_served=fresh_at_first_served,
                expect=rows_of_game if stop_at_mismatch else None)


def generate_game(d, rs, base_ev, table, *, sims, reuse, **kw):
    """a game played by these rules with the moves sampled from pi (temperature 1) by the RandomState rs: the CPU tests' games
    "generated with the table".  Same result dict as replay_game."""
    return _run(d, lambda i, vis: rs.choice(len(vis), p=vis / vis.sum()), base_ev, table, sims=sims, reuse=reuse, **kw)


def free_edges(R, C, x):
    """free real edges per feature row"""
    acts, _ = ER.board(R, C)
    return (np.asarray(x).reshape(len(x), -1)[:, acts] == 0).sum(axis=1)
