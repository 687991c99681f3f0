"""numpy-level wrapper of the HIP engine handle (one handle per GPU / rank)."""
import ctypes as C

import numpy as np

from . import _lib

_p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731


def _temperature_items(temperature):
    temperature = {0: 1.0, 12: 0.02} if temperature is None else temperature
    items = sorted((int(k), float(v)) for k, v in dict(temperature).items())
    if len(items) > 8:
        raise ValueError("at most 8 temperature schedule entries")
    return items


def _dense_from_grouped(w, channels):
    """Conv2d(groups=g) weight [C][C/g][kh][kw] (the reference's n_groups, nn.py:61-71) -> the dense [C][C][kh][kw] weight of the
    same function: output group i sees input group i only, every other product is an exact zero."""
    cpg = w.shape[1]
    if channels % cpg:
        raise ValueError("grouped conv weight %s does not divide %d channels" % (w.shape, channels))
    dense = np.zeros((channels, channels) + w.shape[2:], np.float32)
    for g in range(channels // cpg):
        dense[g * cpg:(g + 1) * cpg, g * cpg:(g + 1) * cpg] = w[g * cpg:(g + 1) * cpg]
    return dense


class Engine:
    """Self-play rollout engine on one MI355X.

    Parameters mirror the reference's configuration (configuration.py:82-100):
    mcts_num_read, cpuct=(c, base), noise=(alpha, coeff), temperature={ply: T},
    reuse_tree.  `evaluator` is one of "formula", "uniform", "resnet", "simplenn",
    "external", "solver".  nn_precision: None = 1 (f16x3 split MFMA, f32-grade) for "resnet", 0 (exact f32 MFMA) otherwise.
    evaluator="solver" (or evaluator2="solver" in match play): perfect play from the solved table of `solver`, a solved
    dotsboxesaz_amd.solver.Solver of this board and device (boards of at most 31 edges); the Engine keeps a reference to it.
    solver_seed picks among equally good moves (0 = the lowest action), solver_reads > 0 caps the driver rule's reads of the
    searches the table serves (attach_solver).
    endgame=Endgame(rows, cols, max_free) (dotsboxesaz_amd.endgame): the models in endgame_models, whatever network or formula
    evaluates them, answer every leaf under a search root with at most max_free free edges from that root's exact table, solved
    once per game (attach_endgame); endgame_seed picks among equally good moves, endgame_reads > 0 caps the driver rule's reads of
    the searches the tables serve.  The Engine keeps a reference to the handle.
    endgame=DeepTables(rows, cols, max_free=M) means the same for any M <= 31 that fits in memory (n_slots x 2^M bytes): the slot
    tables are solved in HBM by the deep solver's kernels (dbaz_attach_tables).  A handle's attaches are all of one kind.
    endgame_tables=N with a DeepTables (dbaz_attach_tables_pool): N regions of 2^M bytes that the slots share, 1 <= N <= n_slots,
    handed out on the device in ascending slot order and taken back when a game ends.  A slot that finds the pool dry searches
    that move with its model's own evaluator (table_pool()["denied"]; run() warns).  None: one region per slot.
    endgame_wait=True with endgame_tables=N (dbaz_attach_tables_pool_wait): a slot that finds the pool dry waits for a region
    instead -- it selects nothing until a game that ends gives one back -- so no search is denied, the rows are those of
    endgame_tables=None for every N >= 1, and endgame_reads may be given.  The idle slot-passes are table_pool_waits()["waited"].
    Self-play and match play only: search() and search_timed() are refused (ESTATE) on such an Engine.
    leaf_endgame=Endgame(rows, cols, max_free=M) (dbaz_attach_leaf_solver): the models in leaf_models solve every leaf with at
    most leaf_free (None: M) free edges that no table serves from scratch, whatever the root (attach_leaf_solver); the seed is
    endgame_seed.  It works alone or next to any endgame= above; leaf_solves() counts the solved leaves.
    playout_cap=(full_prob, fast_reads): playout cap randomization (selfplay_set_playout_cap); None: off.
    forced_playouts=(k, prune): forced playouts and policy target pruning at the root of the self-play driver's full searches
    (selfplay_set_forced_playouts); None: off.
    gumbel=(m, c_visit, c_scale): Gumbel root search in every search of the self-play driver (selfplay_set_gumbel; the usual setting
    is (16, 50.0, 1.0)); None: off.  gumbel=(m, c_visit, c_scale, True): the full mode -- the rule below the root too.
    match_search=(spec0, spec1): the search of each model of a match_play handle (match_set_search); a spec is None (today's search)
    or dict(reads=n, gumbel=(m, c_visit, c_scale[, full[, g_scale]])), either key optional.
    """

    EVALUATORS = {"formula": _lib.EVAL_FORMULA_HASH, "uniform": _lib.EVAL_FORMULA_UNIFORM,
                  "resnet": _lib.EVAL_RESNET, "simplenn": _lib.EVAL_SIMPLENN, "external": _lib.EVAL_EXTERNAL,
                  "solver": _lib.EVAL_SOLVER}

    def __init__(self, rows, cols, n_slots, mcts_num_read=800, cpuct=(1.25, 19652), noise=(0.0, 0.0),
                 temperature=None, reuse_tree=True, evaluator="formula", nodes_per_slot=0, seed=0, device=0,
                 max_out_rows=0, nn_precision=None, match_play=False, evaluator2="formula", transposition_cache=True,
                 max_pending_evals=1, selfplay_pending=False, eval_round=0, eval_defer_max=0, debug_flags=0, solver=None, solver_seed=0,
                 solver_reads=0, endgame=None, endgame_models=(0,), endgame_seed=0, endgame_reads=0, endgame_tables=None, playout_cap=None,
                 forced_playouts=None, gumbel=None, endgame_wait=False, leaf_endgame=None, leaf_free=None, leaf_models=(0,), match_search=None):
        self._L = _lib.load()
        self.rows, self.cols = int(rows), int(cols)
        self.H, self.W = self.rows + 1, self.cols + 1
        self.A = 2 * self.H * self.W
        self.F = 3 * self.H * self.W
        self.E = 2 * self.rows * self.cols + self.rows + self.cols
        self.n_slots = int(n_slots)
        cfg = _lib.Config()
        cfg.rows, cfg.cols, cfg.n_slots, cfg.nodes_per_slot = self.rows, self.cols, self.n_slots, int(nodes_per_slot)
        cfg.mcts_num_read = int(mcts_num_read)
        cfg.cpuct, cfg.cpuct_base = float(cpuct[0]), float(cpuct[1])
        cfg.noise_alpha, cfg.noise_coeff = float(noise[0]), float(noise[1])
        cfg.reuse_tree = int(bool(reuse_tree))
        items = _temperature_items(temperature)
        cfg.n_temp = len(items)
        for i, (k, v) in enumerate(items):
            cfg.temp_idx[i], cfg.temp_val[i] = k, v
        cfg.evaluator = self.EVALUATORS[evaluator] if isinstance(evaluator, str) else int(evaluator)
        cfg.device, cfg.seed, cfg.max_out_rows = int(device), int(seed), int(max_out_rows)
        # None: the advertised mode of the network -- f16x3 (f32-grade, exact-f32 safety net on the device) for ResNetZero, exact f32
        # for SimpleNN (whose f16x3 path has no safety net) and the formula evaluators
        if nn_precision is None:
            nn_precision = 1 if cfg.evaluator == _lib.EVAL_RESNET else 0
        cfg.nn_precision = int(nn_precision)
        cfg.match_play = int(bool(match_play))
        cfg.evaluator2 = self.EVALUATORS[evaluator2] if isinstance(evaluator2, str) else int(evaluator2)
        # True: on for network evaluators; False: off; "force": on for the formula evaluators too (parity tests)
        cfg.transposition_cache = 2 if transposition_cache == "force" else (0 if transposition_cache else 1)
        cfg.max_pending_evals = int(max_pending_evals)
        # self-play searches in waves of max_pending_evals simulations per game (self_play.py:27-30's max_async_searches)
        cfg.selfplay_pending = int(bool(selfplay_pending))
        # "full rounds only": 0 = the network's own round, -1 = off, r > 0 = rounds of r leaves (tests)
        cfg.eval_round, cfg.eval_defer_max = int(eval_round), int(eval_defer_max)
        cfg.debug_flags = int(debug_flags)
        self.cfg = cfg
        self._drained = []
        self.h = C.c_void_p()
        rc = self._L.dbaz_create(C.byref(cfg), C.byref(self.h))
        if rc != _lib.OK:
            _lib.check(None, rc)
        self.nodes_per_slot = int(self._L.dbaz_nodes_per_slot(self.h))  # the pool size in effect (0 asked for the default rule)
        self._solvers = {}
        if solver is not None:
            try:
                for model in range(2 if cfg.match_play else 1):
                    if (cfg.evaluator2 if model else cfg.evaluator) == _lib.EVAL_SOLVER:
                        self.attach_solver(solver, model, solver_seed, solver_reads)
            except Exception:
                self.close()
                raise
        self._endgames = {}
        if endgame_wait and (endgame is None or endgame_tables is None):
            self.close()
            raise _lib.DbazError(_lib.EINVAL, "endgame_wait=True is the wait mode of a pool of tables: it needs endgame=DeepTables(...) and endgame_tables=N")
        if endgame is not None:
            try:
                for model in endgame_models:
                    if endgame_tables is None:
                        self.attach_endgame(endgame, model, endgame_seed, endgame_reads)
                    elif endgame_wait:
                        self.attach_endgame_pool_wait(endgame, endgame_tables, model, endgame_seed, endgame_reads)
                    else:
                        self.attach_endgame_pool(endgame, endgame_tables, model, endgame_seed, endgame_reads)
            except Exception:
                self.close()
                raise
        self._leaf_solvers = {}
        if leaf_endgame is not None:
            try:
                for model in leaf_models:
                    self.attach_leaf_solver(leaf_endgame, leaf_free, model, endgame_seed)
            except Exception:
                self.close()
                raise
        if playout_cap is not None:
            try:
                self.selfplay_set_playout_cap(*playout_cap)
            except Exception:
                self.close()
                raise
        if forced_playouts is not None:
            try:
                self.selfplay_set_forced_playouts(*forced_playouts)
            except Exception:
                self.close()
                raise
        if gumbel is not None:
            try:
                self.selfplay_set_gumbel(*gumbel)
            except Exception:
                self.close()
                raise
        if match_search is not None:
            try:
                for model, spec in enumerate(match_search):
                    spec = spec or {}
                    self.match_set_search(model, spec.get("reads", 0), spec.get("gumbel"))
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self._L.dbaz_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        _lib.check(self.h, rc)

    def attach_solver(self, solver, model=0, seed=0, reads=0):
        """dbaz_attach_solver: model 0 / 1 (its evaluator must be "solver") answers from `solver`'s table, which the engine
        borrows -- the Solver is kept alive with the Engine.  seed: which of several optimal moves gets the prior (0 = the lowest
        action index); reads > 0: searches the table serves run min(driver rule, reads) reads."""
        self._ck(self._L.dbaz_attach_solver(self.h, int(model), solver.h, C.c_uint64(int(seed)), int(reads)))
        self._solvers[int(model)] = solver

    def attach_endgame(self, endgame, model=0, seed=0, reads=0):
        """dbaz_attach_endgame: model 0 / 1 (any evaluator but "external" and "solver") answers the leaves under a search root with
        at most endgame.max_free free edges from that root's exact table, which the engine solves once per game and keeps per slot
        (n_slots x 2^max_free bytes of device memory).  The Endgame is borrowed and kept alive with the Engine.  seed: which of
        several optimal moves gets the prior (0 = the lowest action index); reads > 0: searches the tables serve run
        min(driver rule, reads) reads.
        endgame: an endgame.Endgame (max_free <= 16, solved in LDS) or an endgame.DeepTables (dbaz_attach_tables: max_free <= 31,
        solved in HBM; its own pool is not used); every attach of one Engine is of the same kind and max_free."""
        # the handle's class names its entry (Endgame.ATTACH, DeepTables.ATTACH): the C side cannot tell the two handle types apart
        attach = getattr(self._L, endgame.ATTACH)
        self._ck(attach(self.h, int(model), endgame.h, C.c_uint64(int(seed)), int(reads)))
        self._endgames[int(model)] = endgame

    def attach_endgame_pool(self, endgame, tables, model=0, seed=0, reads=0):
        """dbaz_attach_tables_pool: attach_endgame with a DeepTables whose slot tables are `tables` regions of 2^max_free bytes that
        the slots share (1 .. n_slots; tables << max_free bytes of device memory).  A region is handed to a slot when its search
        root first has at most max_free free edges -- in ascending slot order when several ask in one pass -- and goes back when
        the slot's game ends; a slot that finds the pool dry searches that move with its model's own evaluator and is counted
        (table_pool()).  reads must be 0.  Every attach of one Engine is pooled or not, with one max_free and one `tables`:
        DbazError (EINVAL) otherwise, also for an Endgame, and nothing changes."""
        self._attach_pool("dbaz_attach_tables_pool", endgame, tables, model, seed, reads)

    def attach_endgame_pool_wait(self, endgame, tables, model=0, seed=0, reads=0):
        """dbaz_attach_tables_pool_wait: attach_endgame_pool in wait mode.  A slot that finds the pool dry is not denied: its request
        stands, it selects nothing and spends none of its reads until a pass grants it a region (waiting slots and new askers
        together, in ascending slot order), and then searches as if its search had started in that pass.  The rows are those of
        attach_endgame for every `tables` >= 1; reads means what it means for attach_endgame.  table_pool()["denied"] stays 0 and
        table_pool_waits() counts the waiting.  The self-play driver only: search() and search_timed() raise DbazError (ESTATE)
        afterwards.  An Engine's pooled attaches are all of one mode: DbazError (EINVAL) otherwise, and nothing changes.
        (A method of its own: attach_endgame_pool keeps its parameters.)"""
        self._attach_pool("dbaz_attach_tables_pool_wait", endgame, tables, model, seed, reads)

    def _attach_pool(self, entry, endgame, tables, model, seed, reads):
        if endgame.ATTACH != "dbaz_attach_tables":  # the C side cannot tell the two handle types apart
            raise _lib.DbazError(_lib.EINVAL, "a pool of tables needs a DeepTables, not a %s" % type(endgame).__name__)
        self._ck(getattr(self._L, entry)(self.h, int(model), endgame.h, int(tables), C.c_uint64(int(seed)), int(reads)))
        self._endgames[int(model)] = endgame

    def attach_leaf_solver(self, endgame, leaf_free=None, model=0, seed=0):
        """dbaz_attach_leaf_solver: model 0 / 1 (any evaluator but "external" and "solver") solves every non-terminal leaf with at
        most leaf_free free edges (None: endgame.max_free) that no slot table serves from scratch -- Endgame.policy's (p, v) for
        `seed`, bit for bit -- instead of evaluating it; the rule looks at the leaf alone, not at the root.  endgame: an
        endgame.Endgame, borrowed and kept alive with the Engine; it may be attached as endgame= as well.  endgame=None detaches
        the model.  DbazError (EINVAL) for a leaf_free outside 1 .. endgame.max_free, (ESTATE) while a search is open or games
        are being played; nothing changes then."""
        if endgame is not None and getattr(endgame, "ATTACH", None) != "dbaz_attach_endgame":  # the C side cannot tell the handle types apart
            raise _lib.DbazError(_lib.EINVAL, "a leaf solver needs an Endgame, not a %s" % type(endgame).__name__)
        if leaf_free is not None and int(leaf_free) < 1:
            raise _lib.DbazError(_lib.EINVAL, "leaf_free %r: 1 .. the Endgame's max_free, or None" % (leaf_free,))
        self._ck(self._L.dbaz_attach_leaf_solver(self.h, int(model), endgame.h if endgame is not None else None,
                                                 0 if leaf_free is None else int(leaf_free), C.c_uint64(int(seed))))
        self._leaf_solvers[int(model)] = endgame

    def leaf_solves(self):
        """dbaz_get_leaf_solves: dict(total, by_free) -- the leaves solved from scratch since the first attach_leaf_solver, by_free
        a list of 17 counts for F = 0 .. 16; zeros without an attach.  Waits for the queued work."""
        by = (C.c_int64 * 17)()
        self._ck(self._L.dbaz_get_leaf_solves(self.h, by))
        by = [int(v) for v in by]
        return dict(total=sum(by), by_free=by)

    def table_pool_waits(self):
        """dbaz_get_table_pool_waits: dict(wait_mode, waiting, waited) after the queued work is done -- whether the pool is in wait
        mode, the slots waiting for a region now, and the slot-passes spent waiting since the first attach (what table_pool()'s
        `denied` would have counted).  Zeros without a pooled attach."""
        mode, now, total = C.c_int32(), C.c_int32(), C.c_int64()
        self._ck(self._L.dbaz_get_table_pool_waits(self.h, C.byref(mode), C.byref(now), C.byref(total)))
        return dict(wait_mode=int(mode.value), waiting=int(now.value), waited=int(total.value))

    def table_pool(self):
        """dbaz_get_table_pool: dict(n_tables, in_use, high_water, denied) of the pool of tables after the queued work is done;
        n_tables 0 (and zeros) without a pooled attach.  high_water and denied count since the first attach."""
        n, use, high, den = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._ck(self._L.dbaz_get_table_pool(self.h, C.byref(n), C.byref(use), C.byref(high), C.byref(den)))
        return dict(n_tables=int(n.value), in_use=int(use.value), high_water=int(high.value), denied=int(den.value))

    def endgame_stats(self):
        """(tables_solved, leaves_served) since the first attach_endgame; (0, 0) without one"""
        t, n = C.c_int64(), C.c_int64()
        self._L.dbaz_get_endgame_stats(self.h, C.byref(t), C.byref(n))
        return int(t.value), int(n.value)

    def slot_table(self, slot):
        """dbaz_get_slot_table: dict(valid, n_free, game, free_edges, table, table_index) of a slot's endgame table after the
        queued work is done -- free_edges uint64 [4] by action index, table int8 [2^n_free] (empty without a valid table),
        table_index the region that holds it (dbaz_get_slot_table_index: the slot's own index, or with a pool of tables one of
        its regions, -1 for none).  DbazError (EINVAL) without an attach or for a slot outside 0 .. n_slots - 1."""
        valid, n_free, game = C.c_int32(), C.c_int32(), C.c_int64()
        fe = np.zeros(4, np.uint64)
        self._ck(self._L.dbaz_get_slot_table(self.h, int(slot), C.byref(valid), C.byref(n_free), C.byref(game), _p(fe), None, 0, 0))
        table = np.empty((1 << n_free.value) if valid.value else 0, np.int8)
        if len(table):
            self._ck(self._L.dbaz_get_slot_table(self.h, int(slot), None, None, None, None, _p(table), 0, len(table)))
        at = C.c_int32()
        self._ck(self._L.dbaz_get_slot_table_index(self.h, int(slot), C.byref(at)))
        return dict(valid=bool(valid.value), n_free=int(n_free.value), game=int(game.value), free_edges=fe, table=table, table_index=int(at.value))

    # ---------------------------------------------------------------- rules (G1-G6)
    def rules_init(self, n):
        st = dict(edges=np.zeros((n, 4), np.uint64), b2c2=np.zeros((n, 2), np.int16),
                  to_play=np.zeros(n, np.int8), just_played=np.zeros(n, np.int8))
        self._ck(self._L.dbaz_rules_init(self.h, n, _p(st["edges"]), _p(st["b2c2"]), _p(st["to_play"]),
                                         _p(st["just_played"])))
        return st

    def rules_valid_moves(self, st):
        n = len(st["to_play"])
        out = np.zeros((n, self.A), np.uint8)
        self._ck(self._L.dbaz_rules_valid_moves(self.h, n, _p(st["edges"]), _p(out)))
        return out.astype(bool)

    def rules_play(self, st, moves):
        """In-place play_ on every state; returns (n_closed int8[n], closed_lc int8[n,4]).
        Raises ValueError if any move is illegal (legal ones are still applied)."""
        n = len(st["to_play"])
        moves = np.ascontiguousarray(moves, np.int32)
        nc = np.zeros(n, np.int8)
        lc = np.zeros((n, 4), np.int8)
        self._ck(self._L.dbaz_rules_play(self.h, n, _p(st["edges"]), _p(st["b2c2"]), _p(st["to_play"]),
                                         _p(st["just_played"]), _p(moves), _p(nc), _p(lc)))
        return nc, lc

    def rules_play_status(self, st, moves):
        """Like rules_play but returns n_closed (-1 = illegal) instead of raising."""
        n = len(st["to_play"])
        moves = np.ascontiguousarray(moves, np.int32)
        nc = np.zeros(n, np.int8)
        lc = np.zeros((n, 4), np.int8)
        rc = self._L.dbaz_rules_play(self.h, n, _p(st["edges"]), _p(st["b2c2"]), _p(st["to_play"]),
                                     _p(st["just_played"]), _p(moves), _p(nc), _p(lc))
        if rc not in (_lib.OK, _lib.EILLEGAL):
            self._ck(rc)
        return nc, lc

    def rules_result(self, st):
        n = len(st["to_play"])
        out = np.zeros(n, np.int8)
        self._ck(self._L.dbaz_rules_result(self.h, n, _p(st["b2c2"]), _p(st["to_play"]), _p(out)))
        return out

    def rules_features(self, st):
        n = len(st["to_play"])
        out = np.zeros((n, 3, self.H, self.W), np.int16)
        self._ck(self._L.dbaz_rules_features(self.h, n, _p(st["edges"]), _p(st["b2c2"]), _p(st["to_play"]), _p(out)))
        return out

    # ---------------------------------------------------------------- network (N1-N3)
    def load_state_dict(self, state_dict, kind="resnet", channels=64, blocks=20, head_channels=16, value_fc=8, model=0):
        """state_dict: mapping of the reference's key names to arrays (torch tensors or numpy).
        model: 0 or 1 (the two players of match play)."""
        self._ck(self._L.dbaz_nn_select_model(self.h, int(model)))
        try:
            self._load_state_dict(state_dict, kind, channels, blocks, head_channels, value_fc)
        finally:
            self._L.dbaz_nn_select_model(self.h, 0)

    def _load_state_dict(self, state_dict, kind, channels, blocks, head_channels, value_fc):
        self._ck(self._L.dbaz_nn_configure(self.h, self.EVALUATORS[kind], channels, blocks, head_channels, value_fc))
        for k, v in state_dict.items():
            if k.endswith("num_batches_tracked"):
                continue
            a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            a = np.ascontiguousarray(a, np.float32)
            if kind == "resnet" and ".resblocks." in k and k.endswith(".weight") and a.ndim == 4 and a.shape[0] == channels \
                    and a.shape[1] < channels:
                a = _dense_from_grouped(a, channels)
            self._ck(self._L.dbaz_nn_set_tensor(self.h, k.encode(), _p(a), a.size))
        self._ck(self._L.dbaz_nn_commit(self.h))

    def predict(self, X):
        """NeuralNetWrapper.predict_sync: X [n,3,H,W] -> (p [n,A], v [n,1]) float32."""
        X = np.ascontiguousarray(X, np.float32)
        n = X.shape[0]
        assert X.shape[1:] == (3, self.H, self.W), X.shape
        p = np.zeros((n, self.A), np.float32)
        v = np.zeros((n, 1), np.float32)
        self._ck(self._L.dbaz_nn_predict(self.h, n, _p(X), _p(p), _p(v)))
        return p, v

    # ---------------------------------------------------------------- search (M1-M9)
    def set_search_params(self, cpuct=(1.25, 19652), dirichlet=(0.0, 0.0)):
        self._ck(self._L.dbaz_set_search_params(self.h, float(cpuct[0]), float(cpuct[1]), float(dirichlet[0]),
                                                float(dirichlet[1])))

    def set_positions(self, move_lists=None):
        if move_lists is None:
            self._ck(self._L.dbaz_set_positions(self.h, None, None))
            return
        assert len(move_lists) == self.n_slots
        off = np.zeros(self.n_slots + 1, np.int32)
        off[1:] = np.cumsum([len(m) for m in move_lists])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(m, np.int16).ravel() for m in move_lists] +
                                                   [np.zeros(1, np.int16)]), np.int16)
        self._ck(self._L.dbaz_set_positions(self.h, _p(flat), _p(off)))

    def _search_args(self, num_reads, noise):
        nr = None
        if num_reads is not None:
            nr = np.ascontiguousarray(np.broadcast_to(np.asarray(num_reads, np.int32), (self.n_slots,)), np.int32)
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(noise, np.float64)
            assert nz.shape == (self.n_slots, self.A)
        return nr, nz

    def search(self, num_reads=None, noise=None):
        nr, nz = self._search_args(num_reads, noise)
        self._ck(self._L.dbaz_search(self.h, _p(nr), _p(nz)))

    def set_pending(self, k, virtual_visits=True):
        """max_pending_evals of the following searches (1..the handle's max_pending_evals).  virtual_visits=False: the
        reference's bookkeeping (visits added at backup); True: also counted on the path at selection time."""
        self._ck(self._L.dbaz_set_pending(self.h, int(k), int(bool(virtual_visits))))

    def search_timed(self, time_limit, num_reads=None, noise=None):
        """UCT_search with its wall-clock cut-off (seconds; None / 0 = the reference's 120 s default)."""
        nr, nz = self._search_args(num_reads, noise)
        self._ck(self._L.dbaz_search_timed(self.h, _p(nr), _p(nz), float(time_limit or 0.0)))

    def search_external(self, evaluate, num_reads=None, noise=None):
        """UCT_search with a host evaluator: evaluate(x int16 [m,3,H,W]) -> (p [m,A], v [m])."""
        nr, nz = self._search_args(num_reads, noise)
        self._ck(self._L.dbaz_search_begin(self.h, _p(nr), _p(nz)))
        x = np.zeros((self.n_slots, 3, self.H, self.W), np.int16)
        need = np.zeros(self.n_slots, np.uint8)
        na = C.c_int32()
        P = np.zeros((self.n_slots, self.A), np.float32)
        V = np.zeros(self.n_slots, np.float32)
        while True:
            self._ck(self._L.dbaz_select(self.h, C.byref(na), _p(x), _p(need)))
            if na.value == 0:
                break
            idx = np.nonzero(need)[0]
            if len(idx):
                p, v = evaluate(x[idx])
                P[idx] = np.asarray(p, np.float32)
                V[idx] = np.asarray(v, np.float32).reshape(-1)
            self._ck(self._L.dbaz_expand_backup(self.h, _p(P), _p(V)))

    def roots(self):
        n, A = self.n_slots, self.A
        out = dict(priors=np.zeros((n, A), np.float64), total_value=np.zeros((n, A), np.float32),
                   visits=np.zeros((n, A), np.int32), changed=np.zeros((n, A), np.int32),
                   stats=np.zeros((n, 3), np.int32), q=np.zeros(n, np.float32), root_tv=np.zeros(n, np.float32),
                   root_nv=np.zeros(n, np.int32))
        self._ck(self._L.dbaz_get_roots(self.h, _p(out["priors"]), _p(out["total_value"]), _p(out["visits"]),
                                        _p(out["changed"]), _p(out["stats"]), _p(out["q"]), _p(out["root_tv"]),
                                        _p(out["root_nv"])))
        return out

    def root_states(self):
        n = self.n_slots
        out = dict(edges=np.zeros((n, 4), np.uint64), b2c2=np.zeros((n, 2), np.int16), to_play=np.zeros(n, np.int8),
                   just_played=np.zeros(n, np.int8), result=np.zeros(n, np.int8), expanded=np.zeros(n, np.int8))
        self._ck(self._L.dbaz_get_root_states(self.h, _p(out["edges"]), _p(out["b2c2"]), _p(out["to_play"]),
                                              _p(out["just_played"]), _p(out["result"]), _p(out["expanded"])))
        return out

    def advance(self, moves, reuse_tree=True):
        mv = np.ascontiguousarray(np.broadcast_to(np.asarray(moves, np.int32), (self.n_slots,)), np.int32)
        self._ck(self._L.dbaz_advance(self.h, _p(mv), int(bool(reuse_tree))))

    # ---------------------------------------------------------------- self-play (D1-D3)
    def selfplay_script(self, game_idx, moves, noise=None):
        mv = np.ascontiguousarray(moves, np.int16)
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(noise, np.float64)
            assert nz.shape == (len(mv), self.A)
        self._ck(self._L.dbaz_selfplay_script(self.h, int(game_idx), _p(mv), len(mv), _p(nz)))

    def selfplay_fastforward(self, plies):
        pl = np.ascontiguousarray(plies, np.int32)
        assert pl.shape == (self.n_slots,)
        self._ck(self._L.dbaz_selfplay_fastforward(self.h, _p(pl)))

    def selfplay_stagger(self, first_reads):
        """Benchmark population: read budget of each slot's first search (0 = the driver rule)."""
        fr = np.ascontiguousarray(first_reads, np.int32)
        assert fr.shape == (self.n_slots,)
        self._ck(self._L.dbaz_selfplay_stagger(self.h, _p(fr)))

    def selfplay_quickplay(self, plies, reads):
        """Benchmark population: the first plies[i] plies of slot i's first game use `reads` simulations per move."""
        pl = np.ascontiguousarray(plies, np.int32)
        assert pl.shape == (self.n_slots,)
        self._ck(self._L.dbaz_selfplay_quickplay(self.h, _p(pl), int(reads)))

    def selfplay_set_start(self, move_lists, games_per_start=1):
        """Start positions of the NEXT selfplay_start (SelfPlay.play_games(game_state, idxs)): move_lists is a list of move
        sequences from the empty board (one flat sequence = one start for every game; None or [] = none, the empty board).
        Game g starts from move_lists[(g // games_per_start) % len(move_lists)], g being the absolute game index; move_idx,
        temperature schedule and scripts count plies from the start position.  ValueError for an illegal move (names start
        and ply), DbazError for a finished start or while games are being played."""
        if move_lists is None or len(move_lists) == 0:
            self._ck(self._L.dbaz_selfplay_set_start(self.h, None, None, 0, int(games_per_start)))
            return
        if np.ndim(move_lists[0]) == 0:
            move_lists = [move_lists]
        off = np.zeros(len(move_lists) + 1, np.int32)
        off[1:] = np.cumsum([len(m) for m in move_lists])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(m, np.int16).ravel() for m in move_lists] +
                                                   [np.zeros(1, np.int16)]), np.int16)
        self._ck(self._L.dbaz_selfplay_set_start(self.h, _p(flat), _p(off), len(move_lists), int(games_per_start)))

    def selfplay_set_playout_cap(self, full_prob, fast_reads=0):
        """dbaz_selfplay_set_playout_cap: playout cap randomization for every later selfplay_start.  A search the self-play
        driver starts is a full one -- today's search, its row a training target -- with probability full_prob, decided by
        playout_cap.is_full(seed, game_idx, ply, full_prob); every other one runs min(driver rule, fast_reads) reads without
        root noise and marks its row (bit 0 of "pad"; fetch_samples()["full"] is False).  full_prob >= 1.0: off (the default);
        0: every search fast.  DbazError: EINVAL for full_prob outside [0, 1], fast_reads < 1 with full_prob < 1 or a
        match_play handle, ESTATE while games are being played; a failed call changes nothing."""
        self._ck(self._L.dbaz_selfplay_set_playout_cap(self.h, C.c_double(float(full_prob)), int(fast_reads)))

    def playout_cap(self):
        """dbaz_get_playout_cap: dict(full_prob, fast_reads, full_searches, fast_searches) -- the setting (1.0, 0 when off) and
        the searches the driver started since the last selfplay_start, after the queued work is done."""
        p, n, a, b = C.c_double(), C.c_int32(), C.c_int64(), C.c_int64()
        self._ck(self._L.dbaz_get_playout_cap(self.h, C.byref(p), C.byref(n), C.byref(a), C.byref(b)))
        return dict(full_prob=float(p.value), fast_reads=int(n.value), full_searches=int(a.value), fast_searches=int(b.value))

    def selfplay_set_forced_playouts(self, k, prune=True):
        """dbaz_selfplay_set_forced_playouts: forced playouts and policy target pruning (Wu 2019, section 3.2) for every later
        selfplay_start.  In a full search of the self-play driver every visited root child gets at least sqrt(k P N) playouts;
        with prune those are taken out of the recorded visits again wherever PUCT alone would not have spent them (the row's
        bit 1 of "pad"; fetch_samples()["pruned"] is True).  The game, the tree, q_value and TreeStats are untouched by the
        pruning.  k = 0: off (the default).  The rule is stated in full in include/dbaz.h; forced_playouts.prune_visits is its
        second half on the host.  DbazError: EINVAL for k outside [0, 16], prune not a bool, a match_play handle or
        selfplay_pending; ESTATE while games are being played; a failed call changes nothing."""
        self._ck(self._L.dbaz_selfplay_set_forced_playouts(self.h, C.c_double(float(k)), int(prune)))

    def forced_playouts(self):
        """dbaz_get_forced_playouts: dict(k, prune, rows_pruned, visits_pruned) -- the setting (0.0, False when off) and the rows
        pruning ran on and the visits it took out of them since the last selfplay_start, after the queued work is done."""
        k, p, a, b = C.c_double(), C.c_int32(), C.c_int64(), C.c_int64()
        self._ck(self._L.dbaz_get_forced_playouts(self.h, C.byref(k), C.byref(p), C.byref(a), C.byref(b)))
        return dict(k=float(k.value), prune=bool(p.value), rows_pruned=int(a.value), visits_pruned=int(b.value))

    def selfplay_set_gumbel(self, m=16, c_visit=50.0, c_scale=1.0, full=False):
        """dbaz_selfplay_set_gumbel: the Gumbel root search (Danihelka et al., ICLR 2022) for every later selfplay_start.  Every
        search of the self-play driver, full or fast, samples its candidates by Gumbel-top-m, spends its reads by sequential
        halving and records softmax(logits + sigma(completed Q)) as the row's target: visits = round(pi' * 2^24), bit 2 of "pad"
        (fetch_samples()["gumbel"] is True).  The move is the rule's own (no temperature).  A vector scripted through
        selfplay_script is the search's g.  m = 0: off (the default).  The rule is stated in full in include/dbaz.h;
        gumbel.considered_visits and gumbel.target are its host mirrors.  DbazError: EINVAL for m outside [0, 256], c_visit outside
        [0, 1e6], c_scale outside (0, 1e3], a match_play handle, selfplay_pending or forced playouts on; ESTATE while games are
        being played; a failed call changes nothing.
        full=True (dbaz_selfplay_set_gumbel_mode, looked at while m > 0): the paper's "Full Gumbel" -- below the root every level takes
        argmax pi'(a) - n(a) / (1 + sum n) instead of the UCB's pick, and unvisited children are completed with the full v_mix around
        the node's own value; the rows carry bit 3 beside bit 2 (fetch_samples()["gumbel_full"]).  gumbel.improved_policy,
        gumbel.nonroot_pick and gumbel.target(..., v=) are its host mirrors.  The mode is set only once (m, c_visit, c_scale) was
        accepted, and a mode the handle refuses leaves those as they were."""
        mode, m0, cv0, cs0 = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
        self._ck(self._L.dbaz_get_gumbel_mode(self.h, C.byref(mode)))
        self._ck(self._L.dbaz_get_gumbel(self.h, C.byref(m0), C.byref(cv0), C.byref(cs0), None, None))  # the setting alone: no device work
        self._ck(self._L.dbaz_selfplay_set_gumbel(self.h, int(m), C.c_double(float(c_visit)), C.c_double(float(c_scale))))
        if bool(full) != bool(mode.value):
            try:
                self._ck(self._L.dbaz_selfplay_set_gumbel_mode(self.h, 1 if full else 0))
            except _lib.DbazError:
                self._L.dbaz_selfplay_set_gumbel(self.h, m0, cv0, cs0)
                raise

    def gumbel(self):
        """dbaz_get_gumbel: dict(m, c_visit, c_scale, searches, rows) -- the setting (0, 0.0, 0.0 when off) and the Gumbel searches
        started and rows written since the last selfplay_start, after the queued work is done.  On a handle with the full mode on
        (dbaz_get_gumbel_mode) the dict also has full=True; a handle in the root-only mode reports what it always did."""
        m, cv, cs, a, b, mode = C.c_int32(), C.c_double(), C.c_double(), C.c_int64(), C.c_int64(), C.c_int32()
        self._ck(self._L.dbaz_get_gumbel(self.h, C.byref(m), C.byref(cv), C.byref(cs), C.byref(a), C.byref(b)))
        self._ck(self._L.dbaz_get_gumbel_mode(self.h, C.byref(mode)))
        out = dict(m=int(m.value), c_visit=float(cv.value), c_scale=float(cs.value), searches=int(a.value), rows=int(b.value))
        if mode.value:
            out["full"] = True
        return out

    def match_set_search(self, model, reads=0, gumbel=None):
        """dbaz_match_set_search: the search of one model of a match_play handle, for every later selfplay_start.  reads: the model's
        read budget (0: mcts_num_read; a search runs min(rule, reads) reads, a PUCT model's too).  gumbel=(m, c_visit, c_scale[, full[,
        g_scale]]): every search by this model is a Gumbel search with these constants, root-only or full, its noise g scaled by
        g_scale (default 1.0; 0.0 is the paper's deterministic evaluation search); None: PUCT as today.  The model of a move is
        root.to_play XOR (game_idx & 1).  The rule is stated in full in include/dbaz.h.  DbazError: EINVAL for a handle without
        match_play, a model outside {0, 1} or an argument out of range; ESTATE while games are being played; a failed
        call changes nothing."""
        g = tuple(gumbel) if gumbel is not None else (0, 0.0, 0.0)
        if not 3 <= len(g) <= 5:
            raise _lib.DbazError(_lib.EINVAL, "gumbel=(m, c_visit, c_scale[, full[, g_scale]])")
        full = int(bool(g[3])) if len(g) > 3 else 0
        g_scale = float(g[4]) if len(g) > 4 else 1.0
        self._ck(self._L.dbaz_match_set_search(self.h, int(model), int(reads), int(g[0]), C.c_double(float(g[1])), C.c_double(float(g[2])),
                                               full, C.c_double(g_scale)))

    def match_search(self, model):
        """dbaz_match_get_search: dict(reads, m, c_visit, c_scale, full, g_scale) of one model of a match_play handle (all 0 for a
        model never told; the Gumbel fields read 0 while m = 0)."""
        r, m, mode, cv, cs, gs = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double(), C.c_double(), C.c_double()
        self._ck(self._L.dbaz_match_get_search(self.h, int(model), C.byref(r), C.byref(m), C.byref(cv), C.byref(cs), C.byref(mode), C.byref(gs)))
        return dict(reads=int(r.value), m=int(m.value), c_visit=float(cv.value), c_scale=float(cs.value), full=bool(mode.value),
                    g_scale=float(gs.value))

    def selfplay_start(self, n_games, first_game_idx=0):
        self._ck(self._L.dbaz_selfplay_start(self.h, int(n_games), int(first_game_idx)))

    def step(self, k=1):
        self._ck(self._L.dbaz_step(self.h, int(k)))

    def run(self, max_steps=0):
        """Play until every game is finished.  Finished rows that do not fit the device
        output buffer are drained to the host on the way; fetch_samples() returns them all."""
        while True:
            self._ck(self._L.dbaz_run(self.h, int(max_steps)))
            c = self.counters()
            if max_steps or c["active_slots"] == 0 or c["blocked_slots"] < c["active_slots"]:
                self._warn_pool_resets(c)
                self._warn_tables_denied()
                return
            self._drained.append(self._fetch_once())

    def _warn_pool_resets(self, c):
        """The reference's trees are unbounded; a slot's node pool is not: a move whose reused subtree would not leave
        mcts_num_read + 2 nodes free starts from a fresh root instead (counters()["pool_resets"]).  Said once per handle."""
        n = int(c.get("pool_resets", 0))
        if n and not getattr(self, "_warned_resets", False):
            import warnings
            self._warned_resets = True
            warnings.warn("%d of %d moves were searched from a fresh root because the reused subtree did not leave mcts_num_read + 2 "
                          "nodes of the slot's pool free: raise nodes_per_slot (now %d) to keep the reference's tree reuse on every move"
                          % (n, int(c.get("moves_played", 0)), self.nodes_per_slot))

    def _warn_tables_denied(self):
        """A pool of tables that runs dry changes results as pool_resets do: the slot searches that move without its exact table
        (table_pool()["denied"]).  Said once per handle."""
        if not getattr(self, "_endgames", None) or getattr(self, "_warned_denied", False):
            return
        p = self.table_pool()
        if p["denied"]:
            import warnings
            self._warned_denied = True
            warnings.warn("%d searches with at most max_free free edges found the pool of %d tables dry and ran on the model's own evaluator: "
                          "raise endgame_tables (most held at once: %d) for exact endgames in every game" % (p["denied"], p["n_tables"], p["high_water"]))

    def sync(self):
        self._ck(self._L.dbaz_sync(self.h))

    def timing_begin(self):
        self._ck(self._L.dbaz_timing_begin(self.h))

    def timing_end(self):
        self._ck(self._L.dbaz_timing_end(self.h))

    def counters(self):
        c = _lib.Counters()
        self._ck(self._L.dbaz_get_counters(self.h, C.byref(c)))
        return {k: getattr(c, k) for k, _ in _lib.Counters._fields_}

    def fetch_samples(self):
        """Rows of SelfPlay.get_datasets for the games finished so far (drains the buffer),
        sorted by (game_idx, move_idx)."""
        parts = self._drained + [self._fetch_once()]
        self._drained = []
        out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        order = np.lexsort((out["move_idx"], out["game_idx"]))
        out = {k: v[order] for k, v in out.items()}
        prob = C.c_double()
        self._ck(self._L.dbaz_get_playout_cap(self.h, C.byref(prob), None, None, None))  # the setting alone: no device work
        if prob.value < 1.0:
            # dbaz_fetch_samples keeps its 13 arrays: the column is the rule restated on the host from (seed, game, ply)
            from . import playout_cap as PC
            out["full"] = PC.is_full(self.cfg.seed, out["game_idx"], out["move_idx"], prob.value)
        flags = out.pop("_flags")
        prune = C.c_int32()
        self._ck(self._L.dbaz_get_forced_playouts(self.h, None, C.byref(prune), None, None))  # the setting alone: no device work
        if prune.value or (flags & 2).any():
            out["pruned"] = (flags & 2) != 0  # ROW_FLAG_PRUNED, read from the rows themselves
        gm = C.c_int32()
        self._ck(self._L.dbaz_get_gumbel(self.h, C.byref(gm), None, None, None, None))  # the setting alone: no device work
        mfull = False
        if self.cfg.match_play:  # a match handle's setting is per model (match_set_search)
            ms = [self.match_search(k) for k in (0, 1)]
            gm.value = max(x["m"] for x in ms)
            mfull = any(x["m"] > 0 and x["full"] for x in ms)
        if gm.value or (flags & 4).any():
            out["gumbel"] = (flags & 4) != 0  # ROW_FLAG_GUMBEL: visits are the target pi' in units of 2^-24
        mode = C.c_int32()
        self._ck(self._L.dbaz_get_gumbel_mode(self.h, C.byref(mode)))
        if mfull or (not self.cfg.match_play and gm.value and mode.value) or (flags & 8).any():
            out["gumbel_full"] = (flags & 8) != 0  # ROW_FLAG_GUMBEL_FULL: the search ran the rule below the root too
        return out

    def _fetch_once(self):
        n = C.c_int32()
        self._ck(self._L.dbaz_fetch_samples(self.h, 0, C.byref(n), *([None] * 13)))
        m = n.value
        flags = np.zeros(m, np.int16)  # the rows' flag words, in the order of the rows below (taken first: it drains nothing)
        if m:
            self._ck(self._L.dbaz_fetch_row_flags(self.h, m, C.byref(n), _p(flags)))
        out = dict(game_idx=np.zeros(m, np.int32), move_idx=np.zeros(m, np.int16), move=np.zeros(m, np.int16),
                   player=np.zeros(m, np.int8), x=np.zeros((m, self.F), np.int16), visits=np.zeros((m, self.A), np.int32),
                   pi=np.zeros((m, self.A), np.float64), z=np.zeros(m, np.int8), max_deepness=np.zeros(m, np.int16),
                   tree_size=np.zeros(m, np.int32), terminal_count=np.zeros(m, np.int32),
                   q_value=np.zeros(m, np.float32), played=np.zeros(m, np.int16))
        if m:
            self._ck(self._L.dbaz_fetch_samples(
                self.h, m, C.byref(n), _p(out["game_idx"]), _p(out["move_idx"]), _p(out["move"]), _p(out["player"]),
                _p(out["x"]), _p(out["visits"]), _p(out["pi"]), _p(out["z"]), _p(out["max_deepness"]),
                _p(out["tree_size"]), _p(out["terminal_count"]), _p(out["q_value"]), _p(out["played"])))
        out["_flags"] = flags
        return out

    def replay_rows_dev(self):
        """(device pointer, n_rows, row_bytes) of the packed finished rows (for the RCCL all-gather)."""
        ptr, n, rb = C.c_void_p(), C.c_int32(), C.c_int32()
        self._ck(self._L.dbaz_replay_rows_dev(self.h, C.byref(ptr), C.byref(n), C.byref(rb)))
        return ptr.value, n.value, rb.value

    # ---- training data path: replay rows in HBM -> dataset -> batches in HBM
    @property
    def row_bytes(self):
        return (28 + self.F * 2 + self.A * 4 + 7) // 8 * 8

    def replay_rows_clear(self):
        """Empty the finished-row buffer (the caller keeps the rows it took with replay_rows_dev on the device)."""
        self._ck(self._L.dbaz_replay_rows_clear(self.h))

    def dataset_select(self, which):
        """Address dataset `which` (0..3) with the following dataset_* calls."""
        self._ck(self._L.dbaz_dataset_select(self.h, C.c_int32(which)))
        self._ds_cur = int(which)

    def dataset_begin(self):
        self._ck(self._L.dbaz_dataset_begin(self.h))

    def dataset_add_rows(self, rows, sel=None):
        """rows: (device pointer, n_rows, row_bytes) as returned by replay_rows_dev(), or any object
        with data_ptr()/shape (a torch uint8 CUDA tensor [n, row_bytes], e.g. the all-gathered
        replay).  sel: host int32 row indices in dataset order (None = all rows)."""
        if isinstance(rows, tuple):
            ptr, n, rb = rows
        else:
            if not rows.is_cuda or not rows.is_contiguous():
                raise ValueError("replay rows must be a contiguous CUDA tensor")
            ptr, n, rb = rows.data_ptr(), int(rows.shape[0]), int(rows.shape[1])
        s, ns = None, 0
        if sel is not None:
            s = np.ascontiguousarray(sel, dtype=np.int32)
            ns = len(s)
        self._ck(self._L.dbaz_dataset_add_rows(self.h, C.c_void_p(ptr), C.c_int64(n), C.c_int32(rb), C.c_void_p(_p(s)),
                                               C.c_int64(ns)))

    def dataset_finish(self, pos_average=False, order=None):
        """order: dataset order as a permutation of the staged rows (None = staging order)."""
        n = C.c_int64()
        o = np.ascontiguousarray(order, dtype=np.int32) if order is not None else None
        self._ck(self._L.dbaz_dataset_finish(self.h, C.c_int32(1 if pos_average else 0), C.c_void_p(_p(o)), C.byref(n)))
        self._ds_sizes = getattr(self, "_ds_sizes", {})
        self._ds_sizes[getattr(self, "_ds_cur", 0)] = n.value
        return n.value

    def dataset_fetch(self):
        """Host copies (features int16 [n,3HW], policy float32 [n,A], value float32 [n])."""
        n = getattr(self, "_ds_sizes", {}).get(getattr(self, "_ds_cur", 0), 0)
        x = np.empty((n, self.F), dtype=np.int16)
        pi = np.empty((n, self.A), dtype=np.float32)
        z = np.empty(n, dtype=np.float32)
        self._ck(self._L.dbaz_dataset_fetch(self.h, C.c_void_p(_p(x)), C.c_void_p(_p(pi)), C.c_void_p(_p(z))))
        return x, pi, z

    def dataset_exact_targets(self, endgame, pi_mode="restrict", z_mode=True):
        """dbaz_dataset_exact_targets: the selected dataset's rows of unfinished games with at most endgame.max_free free edges
        get their solved z and pi in place (Endgame.targets' rule and mode names); returns when done.  Returns dict(rows,
        relabelled, finished: rows within max_free left alone because the game was over, z_changed: relabelled rows whose z
        differed from the solved value, by_free: int64 [17], the relabelled rows per number of free edges)."""
        from .endgame import target_modes
        pm, zm = target_modes(pi_mode, z_mode)
        st = np.zeros(4 + 17, dtype=np.int64)
        self._ck(self._L.dbaz_dataset_exact_targets(self.h, endgame.h, C.c_int32(pm), C.c_int32(zm), C.c_void_p(_p(st))))
        return dict(rows=int(st[0]), relabelled=int(st[1]), finished=int(st[2]), z_changed=int(st[3]), by_free=st[4:].copy())

    def dataset_batch(self, idx, sym=0):
        """Rows idx of the dataset under symmetry sym as torch CUDA tensors
        (boards float32 [n,3,H,W], pi [n,A], z [n,1]) -- written by the HIP kernel, no host copy; asynchronous, ordered on torch's
        current stream like any torch op."""
        import torch
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        n = len(idx)
        dev = torch.device("cuda", self.cfg.device)
        boards = torch.empty((n, 3, self.H, self.W), dtype=torch.float32, device=dev)
        pi = torch.empty((n, self.A), dtype=torch.float32, device=dev)
        z = torch.empty((n, 1), dtype=torch.float32, device=dev)
        # queued on torch's CURRENT stream: the tensors above come from torch's stream-ordered caching allocator, so a kernel on any
        # other stream could overwrite a recycled block while work queued on its previous owner is still pending
        with torch.cuda.device(dev):
            self._ck(self._L.dbaz_dataset_batch_on(self.h, C.c_void_p(_p(idx)), C.c_int32(n), C.c_int32(sym), C.c_void_p(boards.data_ptr()),
                                                   C.c_void_p(pi.data_ptr()), C.c_void_p(z.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return boards, pi, z

    def symmetry_apply(self, sym, boards=None, policies=None):
        """SymmetriesGenerator transform `sym` of torch CUDA float32 tensors (out of place)."""
        import torch
        n = int((boards if boards is not None else policies).shape[0])
        for t in (boards, policies):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError("symmetry_apply needs contiguous float32 CUDA tensors")
        torch.cuda.current_stream(boards.device if boards is not None else policies.device).synchronize()
        bo = torch.empty_like(boards) if boards is not None else None
        po = torch.empty_like(policies) if policies is not None else None
        dp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        self._ck(self._L.dbaz_symmetry_apply(self.h, C.c_int32(sym), dp(boards), dp(policies), C.c_int64(n), dp(bo), dp(po)))
        return bo, po


def symmetry_table(rows, cols, sym):
    """src[a'] with out[a'] = in[src[a']] over the two edge planes (host only, no GPU needed)."""
    L = _lib.load()
    lut = np.empty(2 * (rows + 1) * (cols + 1), dtype=np.int32)
    _lib.check(None, L.dbaz_symmetry_table(C.c_int32(rows), C.c_int32(cols), C.c_int32(sym), C.c_void_p(lut.ctypes.data)))
    return lut
