"""The search of each model of a match (dbaz_match_set_search) restated on the CPU (helper of test_gumbel_match_ref_cpu.py,
test_hip_gumbel_match.py and test_hip_gumbel_match_net.py).  Written from the comment of dbaz_match_set_search in include/dbaz.h
alone, on top of gumbel_ref, gumbel_full_ref and the oracle (imported, not edited):

1. Tree, a subclass of gumbel_full_ref.Tree: every node keeps its v^ whichever search expanded it; a search is PUCT (the parent's
   search()), a root-only Gumbel search (gumbel_ref's gsearch, the UCB below the root) or a full one (gumbel_full_ref's).
2. play(): ONE match game.  Per ply the model is to_play ^ (game & 1); its spec gives the reads, min(rule, reads), ahead of the
   table's cap, and the rule.  A PUCT model's visits are the row and its move comes from choose() -- the engine's own row in a replay,
   the way leaf_solve_ref.replay does it, or a RandomState when the helper generates the game.  A Gumbel model runs gsearch with
   g * g_scale; its move and its target are the helper's own.  mistake= switches are for the helper's own tests.
3. min_gap over every Gumbel decision of the game (root picks, moves and the full mode's interior picks), as the two helpers report
   it; the bound 1e-9 and its derivation are in gumbel_full_ref's docstring.

A spec is None (PUCT at the handle's reads) or dict(reads=n, gumbel=(m, c_visit, c_scale[, full[, g_scale]])), as Engine.match_set_search
takes it.  CASES is the table the CPU test checks and the GPU test plays."""
import functools

import numpy as np

from oracle import oracle as O
import endgame_selfplay_ref as ESR
import forced_playouts_ref as FR
import gumbel_full_ref as GF
import gumbel_ref as GR

FLAG_GUMBEL, FLAG_FULL = 4, 8
MISTAKES = ("other_models_constants", "reads_of_other_model", "g_unscaled", "full_for_both", "temperature_move_for_gumbel_seat")
SEED = GR.SEED


def norm_spec(spec):
    """(reads, m, c_visit, c_scale, full, g_scale) of a spec; m = 0: PUCT, and the other Gumbel fields 0 as the getter reads them"""
    spec = spec or {}
    g = spec.get("gumbel")
    if g is None or int(g[0]) == 0:
        return int(spec.get("reads", 0)), 0, 0.0, 0.0, False, 0.0
    g = tuple(g)
    return (int(spec.get("reads", 0)), int(g[0]), float(g[1]), float(g[2]), bool(g[3]) if len(g) > 3 else False,
            float(g[4]) if len(g) > 4 else 1.0)


# ---- 1. the search ----------------------------------------------------------------------------------------------------------------
class Tree(GF.Tree):
    """gumbel_full_ref.Tree whose Gumbel searches are root-only or full one by one (full_now); fstats collects the interior picks"""
    full_now = False

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.fstats = dict(gaps=[], picks=0, deep=0, visited=0)

    def best_child(self, n, k, mistake):
        if self.full_now:
            return GF.Tree.best_child(self, n, k, mistake)
        return GR.Tree.best_child(self, n, k, mistake)  # the rule at the root (while a gsearch runs), the UCB everywhere else

    def gsearch(self, *a, full=False, **kw):
        self.full_now = bool(full)
        try:
            if full:
                return GF.Tree.gsearch(self, *a, **kw)
            return GR.Tree.gsearch(self, *a, **kw)
        finally:
            self.full_now = False


# ---- 2. the game ------------------------------------------------------------------------------------------------------------------
def play(d, choose, *, seed, game_idx, sims, reuse, specs, evs=(0, 0), start=(), g_vectors=None, table=None, table_models=(0,),
         endgame_reads=0, mistake=None):
    """one match game.  choose(i, visits) -> the move of a PUCT ply (< 0: the replayed game ended here).  specs: (spec0, spec1).
    evs: each model's evaluator, a formula kind or evaluate(d, state).  g_vectors(i, valid) -> the scripted g of ply i, None: the
    rule's Philox stream.  table: an endgame_selfplay_ref.Table serving the searches of table_models, capped by endgame_reads.
    No Dirichlet noise (the handles of the cases have none).  Keys: per row x, player, model, visits, pi, q_value, max_deepness,
    tree_size, terminal_count, played, reads, flags, z; n_rows, n_search (root expansions included), n_gumbel, min_gap, ended_early."""
    assert mistake is None or mistake in MISTAKES
    S = [norm_spec(s) for s in specs]
    game = ESR._Game(d, 0, table, None)
    game.base = [FR.formula(e) if isinstance(e, int) else GR._scalar_v(e) for e in evs]
    t = Tree(d, O.state_from_moves(d, list(start)))
    keys = ("x", "player", "model", "visits", "pi", "q_value", "max_deepness", "tree_size", "terminal_count", "played", "reads", "flags")
    out = {key: [] for key in keys}
    gaps = []
    n_search = n_gumbel = i = 0
    ended_early = False
    while not t.is_terminal:
        st = t.state
        valid = t.first.valid
        F = int(valid.sum())
        model = (st.to_play ^ (int(game_idx) & 1)) & 1
        reads_m, m, c_visit, c_scale, full, g_scale = S[model]
        o_reads, o_m, o_cv, o_cs, o_full, _ = S[1 - model]
        if mistake == "reads_of_other_model":
            reads_m = o_reads
        if mistake == "other_models_constants" and m > 0 and o_m > 0:
            m, c_visit, c_scale = o_m, o_cv, o_cs
        if mistake == "full_for_both" and m > 0:
            full = full or (o_m > 0 and o_full)
        if mistake == "g_unscaled":
            g_scale = 1.0
        reads = ESR._fact_reads(F, sims)
        if reads_m > 0:
            reads = min(reads, reads_m)
        game.model = model
        game.use_table = table is not None and model in table_models and F <= table.max_free
        if game.use_table:
            if game.ref is None:
                game.ref = ESR.SlotTablesRef(table.R, table.C, O.features(d, st).ravel()[None], table.seed, table.max_free)
            if endgame_reads > 0:
                reads = min(reads, endgame_reads)
        expanded = t.is_expanded
        if m > 0:
            if g_vectors is not None:
                g = np.asarray(g_vectors(i, valid), np.float64)
            else:
                g = np.array([GR.philox_g(seed, game_idx, i, a) for a in range(d.A)], np.float64)  # (plies count from the start position)
            move, vis, info = t.gsearch(reads, game._evaluate, m, c_visit, c_scale, g_scale * g, gaps, None, full=full)
            assert not info["tied"], "a root without a positive prior: none of the cases has one"
            flags = FLAG_GUMBEL | (FLAG_FULL if full else 0)
            n_gumbel += 1
            if mistake == "temperature_move_for_gumbel_seat":
                move = int(choose(i, vis))
        else:
            vis = t.search(reads, game._evaluate)
            flags = 0
            move = int(choose(i, vis))
        n_search += reads + (0 if expanded else 1)
        if move < 0:
            ended_early = True
            break
        md, ts, tc, q = t.stats()
        s = int(vis.sum())
        row = dict(x=O.features(d, st).ravel(), player=st.to_play, model=model, visits=vis, pi=vis.astype(np.float64) / (s if s else 1.0),
                   q_value=np.float32(q), max_deepness=md, tree_size=ts, terminal_count=tc, played=move, reads=reads, flags=flags)
        for key, v in row.items():
            out[key].append(v)
        t.advance(move, reuse)
        i += 1
    res = {key: np.array(v) for key, v in out.items()}
    res["x"] = res["x"].astype(np.int16).reshape(len(out["x"]), -1)
    if not ended_early:
        term = t.state
        zt = O.get_result(term)
        res["z"] = np.array([zt if p == term.just_played else -zt for p in out["player"]], np.int64)
    res.update(n_rows=i, n_search=n_search, n_gumbel=n_gumbel, min_gap=min(gaps + t.fstats["gaps"]) if gaps or t.fstats["gaps"] else float("inf"),
               interior_picks=t.fstats["picks"], ended_early=ended_early)
    return res


def generate(d, rs, **kw):
    """a game with the PUCT plies' moves sampled from the visits (temperature 1) by the RandomState rs"""
    return play(d, lambda i, vis: rs.choice(len(vis), p=vis / vis.sum()), **kw)


def replay(d, rows_of_game, **kw):
    """the engine's game: the PUCT plies' moves are the rows' (their visits are compared by the caller), the Gumbel plies' are the
    helper's own.  The game's number comes from rows_of_game["game_idx"]."""
    played = np.asarray(rows_of_game["played"]).astype(np.int64)
    game_idx = int(np.asarray(rows_of_game["game_idx"]).ravel()[0])
    return play(d, lambda i, vis: played[i] if i < len(played) else -1, game_idx=game_idx, **kw)


def games_differ(a, b):
    return GF.games_differ(a, b)


def rows_differ(ref, rows):
    """the first row at which a replay and the engine's rows of that game (arrays in move order) differ -- move, visits, q_value bits,
    tree statistics, flag bits, z -- with what differs, or None"""
    n = min(ref["n_rows"], len(rows["played"]))
    for i in range(n):
        for key in ("played", "player", "tree_size", "max_deepness", "terminal_count"):
            if int(ref[key][i]) != int(rows[key][i]):
                return i, key, ref[key][i], rows[key][i]
        if not np.array_equal(ref["x"][i], rows["x"][i]):
            return i, "x"
        if np.float32(ref["q_value"][i]).tobytes() != np.float32(rows["q_value"][i]).tobytes():
            return i, "q_value", ref["q_value"][i], rows["q_value"][i]
        if not np.array_equal(np.asarray(ref["visits"][i]).astype(np.int64), np.asarray(rows["visits"][i]).astype(np.int64)):
            return i, "visits", ref["visits"][i], rows["visits"][i]
        if "flags" in rows and int(ref["flags"][i]) != int(rows["flags"][i]):
            return i, "flags", ref["flags"][i], rows["flags"][i]
    if ref["n_rows"] != len(rows["played"]) or ref["ended_early"]:
        return n, "length", ref["n_rows"], len(rows["played"])
    if not np.array_equal(ref["z"], np.asarray(rows["z"]).astype(np.int64)):
        return n, "z", ref["z"], rows["z"]
    return None


# ---- the engine's side of a comparison (the GPU tests) ---------------------------------------------------------------------------
def game_rows(got, gi):
    r = np.nonzero(got["game_idx"] == gi)[0]
    assert list(got["move_idx"][r]) == list(range(len(r))), gi
    rows = {k: v[r] for k, v in got.items()}
    rows["flags"] = 4 * rows["gumbel"].astype(np.int64) + (8 * rows["gumbel_full"].astype(np.int64) if "gumbel_full" in rows else 0)
    return rows


def played(e, n_games):
    e.selfplay_start(n_games, 0)
    e.run()
    c = e.counters()
    assert c["games_finished"] == n_games and c["error_slots"] == 0 and c["active_slots"] == 0 and c["pool_resets"] == 0
    gm = e.gumbel()
    got = e.fetch_samples()
    assert sorted(set(got["game_idx"])) == list(range(n_games))
    return c, gm, got


def compare_game(ref, rows, what):
    """one replay against the engine's rows of the game, bit for bit: the move, the visits (a PUCT row's counts, a Gumbel row's target
    in units of 2^-24), q_value, the tree statistics, the flag bits and z"""
    n = min(ref["n_rows"], len(rows["played"]))
    for i in range(n):  # row by row: the message names the first ply that differs
        where = what + ("ply", i, "model", int(ref["model"][i]), "reads", int(ref["reads"][i]), "min_gap", ref["min_gap"])
        assert rows["played"][i] == ref["played"][i], where
        assert np.array_equal(rows["x"][i], ref["x"][i]) and rows["player"][i] == ref["player"][i], where
        assert np.float32(rows["q_value"][i]).tobytes() == np.float32(ref["q_value"][i]).tobytes(), where
        for key in ("tree_size", "max_deepness", "terminal_count", "flags"):
            assert rows[key][i] == ref[key][i], where + (key, rows[key][i], ref[key][i])
        assert np.array_equal(rows["visits"][i].astype(np.int64), ref["visits"][i]), where + (rows["visits"][i], ref["visits"][i])
    assert len(rows["played"]) == ref["n_rows"] and not ref["ended_early"], what
    assert np.array_equal(rows["z"], ref["z"]), what


# ---- the case table ---------------------------------------------------------------------------------------------------------------
C_VISIT, C_SCALE = GR.C_VISIT, GR.C_SCALE
TABLE_SEED = GR.TABLE_SEED
KIND = GR.KIND
CASES = {
    # sims: the handle's mcts_num_read; specs: the two models; evs: their formula evaluators; book: the openings' lengths
    # (games_per_start = 2); script: the Gumbel plies' g is scripted; table: Endgame(3, 3, max_free) on model 0
    "a": dict(R=3, C=3, sims=32, reuse=False, games=16, specs=(dict(reads=16, gumbel=(4, C_VISIT, C_SCALE)), dict(reads=24)),
              evs=("formula", "formula")),
    "b": dict(R=3, C=3, sims=32, reuse=True, games=16, specs=(dict(reads=16, gumbel=(4, C_VISIT, C_SCALE)), dict(reads=24)),
              evs=("formula", "formula")),
    "c": dict(R=3, C=3, sims=32, reuse=True, games=16, specs=(dict(reads=32, gumbel=(4, 50.0, 1.0, True)), dict(reads=16, gumbel=(2, 0.0, 0.1))),
              evs=("uniform", "formula")),
    "d": dict(R=3, C=3, sims=32, reuse=True, games=16,
              specs=(dict(reads=16, gumbel=(4, C_VISIT, C_SCALE, False, 0.0)), dict(reads=24, gumbel=(3, C_VISIT, C_SCALE, True, 0.0))),
              evs=("formula", "formula"), book=(1, 2, 3, 4)),
    "e": dict(R=3, C=3, sims=32, reuse=True, games=16, specs=(dict(reads=16, gumbel=(4, C_VISIT, C_SCALE, False, 0.5)), None),
              evs=("formula", "formula"), script=True),
    "f": dict(R=3, C=3, sims=32, reuse=True, games=16, specs=(dict(reads=24, gumbel=(16, C_VISIT, C_SCALE)), None),
              evs=("formula", "formula"), table=8, endgame_reads=12),
    "g": dict(R=6, C=6, sims=16, reuse=True, games=2, specs=(dict(reads=16, gumbel=(4, C_VISIT, C_SCALE)), None), evs=("formula", "formula")),
    "h": dict(R=10, C=10, sims=16, reuse=True, games=2, specs=(dict(reads=16, gumbel=(2, C_VISIT, C_SCALE, True)), None),
              evs=("formula", "formula")),
}
CASE_IDS = list(CASES)
# the case each deliberate mistake must change at least half of the games of
MISTAKE_CASES = {
    "other_models_constants": "c",
    "reads_of_other_model": "a",
    "g_unscaled": "e",
    "full_for_both": "c",
    "temperature_move_for_gumbel_seat": "a",
}


def case_book(name):
    c = CASES[name]
    return GR.openings(O.dims(c["R"], c["C"]), len(c["book"]), c["book"]) if "book" in c else None


def case_kw(name, game_idx):
    """the keywords of play() for one game of a case (everything but choose and mistake)"""
    c = CASES[name]
    book = case_book(name)
    kw = dict(seed=SEED, game_idx=game_idx, sims=c["sims"], reuse=c["reuse"], specs=c["specs"], evs=tuple(KIND[e] for e in c["evs"]),
              start=tuple(book[GR.start_of(game_idx, len(book), 2)]) if book else ())
    if c.get("script"):
        V = script_vectors(name, game_idx)
        kw["g_vectors"] = lambda i, valid: V[i]
    if "table" in c:
        kw.update(table=ESR.Table(c["R"], c["C"], c["table"], TABLE_SEED), endgame_reads=c["endgame_reads"])
    return kw


@functools.lru_cache(maxsize=None)
def case_games(name, mistake=None):
    """the games of a case with the helper's own moves on the PUCT plies (RandomState(500 + game)), computed once and shared"""
    c = CASES[name]
    d = O.dims(c["R"], c["C"])
    return [generate(d, np.random.RandomState(500 + gi), mistake=mistake, **case_kw(name, gi)) for gi in range(c["games"])]


def script_vectors(name, game_idx):
    """float64 [E + 1, A]: the scripted vector of every ply of a game, standard Gumbel draws from RandomState(1000 + game): the g of
    the ply if a Gumbel model searches it, unused otherwise (the handles have no Dirichlet noise)"""
    c = CASES[name]
    d = O.dims(c["R"], c["C"])
    E = 2 * c["R"] * c["C"] + c["R"] + c["C"]
    return np.random.RandomState(1000 + int(game_idx)).gumbel(size=(E + 1, d.A))
