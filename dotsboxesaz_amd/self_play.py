"""Host-side mirror of the reference's self-play driver contract (self_play.py).

    generate_games(hdf_file_name, generation, nn_class, n_games, params, ...)   self_play.py:291-306
    SelfPlay(nn, params).play_games(...) / get_datasets(generation)             self_play.py:19-156

The games themselves run on the GPU (dotsboxesaz_amd.engine.Engine): thousands of concurrent
games, one sequential search per game (the reference's max_async_searches=1 semantics), slots
refilled as games finish.  This module only shapes configuration in and DataFrames out, shards
game indices over ranks and all-gathers the replay rows over RCCL at iteration end.
"""
import time

import numpy as np


def _get(d, k, default=None):
    if d is None:
        return default
    if isinstance(d, dict):
        return d.get(k, default)
    return getattr(d, k, default)


def shard_games(n_games, world_size, rank):
    """Contiguous game-index range of `rank` (np.array_split semantics, self_play.py:294)."""
    base, extra = divmod(int(n_games), int(world_size))
    first = rank * base + min(rank, extra)
    return first, base + (1 if rank < extra else 0)


def start_index(game_idx, n_starts, games_per_start=1):
    """Which start position of a book of n_starts game `game_idx` (the ABSOLUTE index; scalar or numpy array) begins from:
    games_per_start consecutive games share a start, and the book wraps round (dbaz_selfplay_set_start)."""
    return (np.asarray(game_idx) // int(games_per_start)) % int(n_starts)


def start_moves(game_state, rows, cols):
    """The move sequence from the empty board that dbaz_selfplay_set_start needs, of a reference-style game_state (the
    mirror BoxesState records it in `_moves`) or of a plain move sequence.  None / a state on the empty board: [].
    TypeError for a position that does not say how it was reached (a set of edges determines neither to_play nor
    boxes_to_close); ValueError for a state of another board size."""
    if game_state is None:
        return []
    moves = getattr(game_state, "_moves", None)
    if moves is not None:
        dim = getattr(game_state, "_dim", None)
        if dim is not None and tuple(dim) != (rows, cols):
            raise ValueError("game_state is a %dx%d board, the engine plays %dx%d" % (dim[0], dim[1], rows, cols))
        return [int(m) for m in moves]
    if hasattr(game_state, "board") or hasattr(game_state, "get_features"):
        if hasattr(game_state, "board"):
            played = np.asarray(game_state.board) // 255  # what get_features shows (dots_boxes_game.py:96-100)
            shape = played.shape[-2:]
        else:
            feats = np.asarray(game_state.get_features())
            played, shape = feats[:2], feats.shape[-2:]
        if tuple(shape) != (rows + 1, cols + 1):
            raise ValueError("game_state is a %dx%d board, the engine plays %dx%d" % (shape[0] - 1, shape[1] - 1, rows, cols))
        if not played.any():
            return []
        raise TypeError("game_state is not the empty board and does not record its moves (`_moves`, as dotsboxesaz_amd.game."
                        "BoxesState does): the edges alone determine neither to_play nor boxes_to_close")
    return [int(m) for m in game_state]  # a plain move sequence


def _gumbel_args(gum):
    """params.self_play.gumbel -> (m, c_visit, c_scale) with the defaults of Engine.selfplay_set_gumbel; (m, c_visit, c_scale, True)
    with "full": True (the rule below the root too)"""
    args = (int(_get(gum, "m", 16)), float(_get(gum, "c_visit", 50.0)), float(_get(gum, "c_scale", 1.0)))
    return args + (True,) if bool(_get(gum, "full", False)) else args


def match_search_spec(spec):
    """the search of one model of a match as compute_elo(search=) and solver_match(search=) take it -- None, or {"reads": n, "gumbel":
    {...params.self_play.gumbel's dict..., "g_scale": s}}, either key optional -- as Engine(match_search=) takes it"""
    if spec is None:
        return None
    out = {"reads": int(_get(spec, "reads", 0) or 0)}
    gum = _get(spec, "gumbel")
    if gum:
        args = _gumbel_args(gum)
        gs = _get(gum, "g_scale")
        out["gumbel"] = args[:3] + (len(args) > 3, 1.0 if gs is None else float(gs))
    return out


def engine_kwargs_from_params(params, async_searches=False):
    """Pull the hot-path knobs out of a reference-style params dict (configuration.py:82-100).

    async_searches: the reference runs every self-play search with `max_async_searches` simulations of the ONE tree in flight
    (self_play.py:27-30, configuration.py:99: 64), only to fill a GPU batch from a single game -- 98 % of those leaves are
    duplicates.  Here the batch comes from thousands of concurrent games, so the default is the sequential search per
    game (max_pending_evals = 1: the semantics of every parity path).  async_searches=True honours the knob instead: every search
    of every game runs in waves of self_play.mcts.max_async_searches simulations with the reference's bookkeeping
    (dbaz_config.selfplay_pending; equal to the reference's own UCT_search(..., max_pending_evals=K) under an evaluator that
    suspends once per call, tests/test_hip_pending.py).

    params.self_play.playout_cap = {"full_prob": p, "fast_reads": n} (not a knob of the reference; absent = off) becomes
    Engine(playout_cap=(p, n)): playout cap randomization, Engine.selfplay_set_playout_cap.
    params.self_play.forced_playouts = {"k": 2.0, "prune": True} (the same; absent = off) becomes Engine(forced_playouts=(k, prune)):
    forced playouts and policy target pruning, Engine.selfplay_set_forced_playouts.  It is refused together with
    async_searches=True and max_async_searches > 1 (self-play in waves).
    params.self_play.gumbel = {"m": 16, "c_visit": 50, "c_scale": 1.0} (the same; absent = off) becomes Engine(gumbel=(m, c_visit,
    c_scale)): the Gumbel root search, Engine.selfplay_set_gumbel.  It is refused together with forced_playouts and with self-play
    in waves.  "full": True in that dict makes it Engine(gumbel=(m, c_visit, c_scale, True)): the rule below the root too."""
    sp = _get(params, "self_play")
    m = _get(sp, "mcts")
    noise = _get(sp, "noise", [0.0, 0.0])
    kw = dict(mcts_num_read=int(_get(m, "mcts_num_read", 800)), cpuct=tuple(_get(m, "mcts_cpuct", (1.25, 19652))),
              noise=(float(noise[0]), float(noise[1])), temperature=dict(_get(m, "temperature", {0: 1.0})),
              reuse_tree=bool(_get(sp, "reuse_mcts_tree", True)))
    k = int(_get(m, "max_async_searches", 1) or 1)
    if async_searches and k > 1:
        kw.update(max_pending_evals=k, selfplay_pending=True, transposition_cache=False)
    cap = _get(sp, "playout_cap")
    if cap is not None:
        kw["playout_cap"] = (float(_get(cap, "full_prob")), int(_get(cap, "fast_reads")))
    forced = _get(sp, "forced_playouts")
    if forced is not None:
        kw["forced_playouts"] = (float(_get(forced, "k")), bool(_get(forced, "prune", True)))
    gum = _get(sp, "gumbel")
    if gum is not None:
        kw["gumbel"] = _gumbel_args(gum)
    return kw


def samples_to_dataframe(s, generation, rows, cols, with_features=True):
    """SelfPlay.get_datasets schema (self_play.py:95-156): index (generation, game_idx, move_idx);
    columns move i16, player i8, x_* i16, pi_* f64, z i64, max_deepness i16, tree_size i32,
    terminal_count i32, q_value f32."""
    import pandas as pd
    n = len(s["move"])
    A = s["pi"].shape[1]
    F = s["x"].shape[1]
    if isinstance(generation, (list, tuple)):
        gen = np.where(s["player"] == 0, generation[0], generation[1]).astype(np.int16)
    else:
        gen = np.full(n, generation, dtype=np.int16)
    cols_ = {"generation": gen, "game_idx": s["game_idx"].astype(np.int16), "move_idx": s["move_idx"].astype(np.int16),
             "move": s["move"].astype(np.int16), "player": s["player"].astype(np.int8)}
    df = pd.DataFrame(cols_)
    parts = [df]
    if with_features:
        parts.append(pd.DataFrame(s["x"].astype(np.int16), columns=["x_%d" % i for i in range(F)]))
    parts.append(pd.DataFrame(s["pi"].astype(np.float64), columns=["pi_%d" % i for i in range(A)]))
    parts.append(pd.DataFrame({"z": s["z"].astype(np.int64)}))
    parts.append(pd.DataFrame({"max_deepness": s["max_deepness"].astype(np.int16), "tree_size": s["tree_size"].astype(np.int32),
                               "terminal_count": s["terminal_count"].astype(np.int32),
                               "q_value": s["q_value"].astype(np.float32)}))
    df = pd.concat(parts, axis=1)
    df.set_index(["generation", "game_idx", "move_idx"], inplace=True)
    return df


class SelfPlay:
    """Reference: self_play.py:19-156.  `nn` is a dotsboxesaz_amd.nn.NeuralNetWrapper (its engine
    plays the games) or an Engine whose evaluator is already configured.  leaf_endgame, leaf_free, leaf_models, leaf_seed: an
    endgame.Endgame that is attached to that engine as the leaf solver of the listed models (Engine.attach_leaf_solver) before
    the first game; leaf_seed picks among equally good moves, as Engine(endgame_seed=) does."""

    def __init__(self, nn, params, leaf_endgame=None, leaf_free=None, leaf_models=(0,), leaf_seed=0):
        self.params = params
        self.engine = getattr(nn, "engine", nn)
        self.samples = None
        if leaf_endgame is not None:
            for model in leaf_models:
                self.engine.attach_leaf_solver(leaf_endgame, leaf_free, model, leaf_seed)
        forced = _get(_get(params, "self_play"), "forced_playouts")
        if forced is not None:  # the engine was made elsewhere: the setting of the handle follows the parameters
            self.engine.selfplay_set_forced_playouts(float(_get(forced, "k")), bool(_get(forced, "prune", True)))
        gum = _get(_get(params, "self_play"), "gumbel")
        if gum is not None:
            self.engine.selfplay_set_gumbel(*_gumbel_args(gum))

    def play_games_sync(self, games_idxs, game_state=None):
        """game_state: the position every game starts from (self_play.py:51-55; None = the empty board); move_idx and the
        temperature schedule count from it."""
        idx = np.asarray(list(games_idxs), dtype=np.int64)
        moves = start_moves(game_state, self.engine.rows, self.engine.cols)
        if len(idx) == 0:
            return
        if not np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx))):
            raise ValueError("game indices must be a contiguous range")
        self.engine.selfplay_set_start([moves] if moves else None)
        self.engine.selfplay_start(len(idx), int(idx[0]))
        self.engine.run()
        got = self.engine.fetch_samples()
        self.samples = got if self.samples is None else {k: np.concatenate([self.samples[k], got[k]]) for k in got}

    async def play_games(self, game_state, games_idxs, show_progress=False):
        self.play_games_sync(games_idxs, game_state)

    def get_datasets(self, generation, with_features=True):
        e = self.engine
        return samples_to_dataframe(self.samples, generation, e.rows, e.cols, with_features)


def write_dataset(file_name, key, df):
    """utils.write_to_hdf (utils/utils.py:94-96): append to an HDFStore table; parquet when the
    file name says so (pytables is not part of this image)."""
    if str(file_name).endswith(".parquet"):
        df.reset_index().to_parquet(file_name)
        return
    import pandas as pd
    with pd.HDFStore(file_name, mode="a") as store:
        store.append(key, df, format="table")


def generate_games(hdf_file_name, generation, nn_class, n_games, params, n_workers=None, games_per_workers=10,
                   rows=None, cols=None, n_slots=None, device=0, dist=None, nn_precision=None, async_searches=False,
                   start_states=None, games_per_start=1, endgame=None, endgame_models=(0,), endgame_tables=None, fast_rows="drop",
                   endgame_wait=False, leaf_endgame=None, leaf_free=None, leaf_models=(0,)):
    """Reference: self_play.generate_games (self_play.py:291-306) called from coach.selfplay
    (coach.py:27-29).  Plays n_games with generation-1's weights (random init for generation 0,
    self_play.py:187-190) and appends the samples (+ `training` = 0) to key "fresh".
    With torch.distributed initialised (one process per GPU) the game indices are sharded over
    the ranks (the reference's np.array_split over pool workers, :294); every rank keeps its
    finished rows on the device, the packed rows are all-gathered (RCCL; host-staged under gloo)
    and EVERY rank builds the DataFrame of all n_games games -- the reference's workers all append
    to the one HDF file (self_play.py:264-265); here rank 0 writes it.
    nn_precision: None = the engine's default for the network (ResNetZero: 1, the f16x3 mode every published number of this
    repository is measured in; 0 = exact f32 MFMA, 2.6x slower).
    async_searches: honour params.self_play.mcts.max_async_searches (see engine_kwargs_from_params; default: sequential search
    per game, batching across games).
    start_states: a book of start positions (move sequences from the empty board, or mirror BoxesStates): game g starts from
    start_states[start_index(g, len(start_states), games_per_start)], g being the absolute game index, so a game's rows stay
    a function of (seed, game index) however the games are sharded over ranks.  None: the empty board.
    endgame: an endgame.Endgame (max_free <= 16) or endgame.DeepTables (max_free <= 31) of the board and device: from a game's first search root with at most endgame.max_free free edges
    on, every leaf is answered from that root's exact table instead of the network (Engine.attach_endgame).
    endgame_tables: with a DeepTables, the slots share a pool of that many tables (Engine(endgame_tables=N)); None: one per slot.
    endgame_wait: with endgame_tables, a slot that finds the pool dry waits for a table instead of searching that move without one
    (Engine(endgame_wait=True)): the rows are those of endgame_tables=None whatever the pool's size.
    leaf_endgame, leaf_free, leaf_models: an endgame.Endgame whose solver answers every leaf with at most leaf_free free edges that no
    table serves, whatever the root (Engine(leaf_endgame=...), Engine.attach_leaf_solver); alone or next to endgame=.
    fast_rows: with params.self_play.playout_cap set, "drop" leaves the rows of the fast searches (bit 0 of "pad") out of the
    DataFrame -- they moved the games on and are no training targets -- and "keep" writes every row.  Without a cap no row is
    marked and the two are the same."""
    from .engine import Engine
    if fast_rows not in ("drop", "keep"):
        raise ValueError("fast_rows must be 'drop' or 'keep', not %r" % (fast_rows,))
    game = _get(params, "game")
    if rows is None:
        dims = _get(game, "dims") or getattr(_get(game, "clazz"), "BOARD_DIM", (3, 3))
        rows, cols = int(dims[0]), int(dims[1])
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist is not None else (0, 1)
    first, count = shard_games(n_games, world, rank)
    n_slots = n_slots or max(1, min(count, 8192))
    model = nn_class(params)
    if generation != 0:
        model.load_parameters(generation - 1)
    # Philox streams are keyed by (seed, game, ply): sharding does not change a game
    eng = Engine(rows, cols, n_slots, evaluator=model.kind, device=device, seed=generation * 1000003,
                 nn_precision=nn_precision, endgame=endgame, endgame_models=endgame_models, endgame_tables=endgame_tables,
                 endgame_wait=endgame_wait, leaf_endgame=leaf_endgame, leaf_free=leaf_free, leaf_models=leaf_models,
                 **engine_kwargs_from_params(params, async_searches))
    try:
        if model.kind in ("resnet", "simplenn"):
            eng.load_state_dict(model.state_dict(), model.kind, **model.shape)
        if start_states is not None and len(start_states) and count > 0:
            eng.selfplay_set_start([start_moves(st, rows, cols) for st in start_states], games_per_start)
        packed = collect_rows_device(eng, count, first)
        if dist is not None and world > 1:
            packed, _ = all_gather_rows(packed, dist)
        samples = unpack_rows(packed.cpu().numpy(), eng.F, eng.A)
    finally:
        eng.close()
    if fast_rows == "drop":
        samples = full_rows_only(samples)
    df = samples_to_dataframe(samples, generation, rows, cols, True)
    df["training"] = np.zeros(len(df.index), dtype=np.int8)
    if hdf_file_name is not None and rank == 0:
        write_dataset(hdf_file_name, "fresh", df)
    return df


# ---------------------------------------------------------------------------------------
# multi-GPU: replay all-gather over RCCL (replaces the HDF-append-under-lock exchange,
# self_play.py:264-265).  Fixed-stride packed rows (DESIGN.md "replay row").
# ---------------------------------------------------------------------------------------
class _DevBuf:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}


# RowMeta of csrc/common.h (28 bytes); a packed replay row is RowMeta | x int16[3HW] | visits int32[A], padded to 8 B
ROW_META = np.dtype([("game_idx", "<i4"), ("move_idx", "<i2"), ("move", "<i2"), ("played", "<i2"),
                     ("max_deepness", "<i2"), ("tree_size", "<i4"), ("terminal_count", "<i4"), ("q_value", "<f4"),
                     ("player", "i1"), ("z", "i1"), ("pad", "<i2")])
assert ROW_META.itemsize == 28


ROW_FLAGS_OFF, ROW_FLAG_FAST = 26, 1  # csrc/replay_row.h: the int16 "pad"; bit 0 = the row of a fast search of the playout cap
ROW_FLAG_PRUNED = 2  # bit 1 = policy target pruning ran on the row: its visits (and pi) are the pruned ones
ROW_FLAG_GUMBEL = 4  # bit 2 = the row of a Gumbel search: its visits are the target pi' in units of 2^-24 (pi = visits / visits.sum())
ROW_FLAG_GUMBEL_FULL = 8  # bit 3, beside bit 2 = that search ran the full mode: the rule below the root too


def full_rows_only(samples):
    """The rows of a sample dict of unpack_rows whose search was a full one ("pad" bit 0 clear); the dict itself when none is marked."""
    keep = (samples["pad"] & ROW_FLAG_FAST) == 0
    return samples if keep.all() else {k: v[keep] for k, v in samples.items()}


def row_bytes(F, A):
    return (ROW_META.itemsize + 2 * F + 4 * A + 7) // 8 * 8


def unpack_rows(packed, F, A):
    """Packed replay rows (uint8 [n, row_bytes], any rank order) -> the sample dict of
    Engine.fetch_samples(), sorted by (game_idx, move_idx); pi = visits / (sum or 1.0) in float64
    (self_play.py:114-115), plus "pad", the rows' flag word (bit 0: the row of a fast search of the playout cap; 0 without one)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    n = packed.shape[0]
    if n and packed.shape[1] != row_bytes(F, A):
        raise ValueError("row stride %d does not match a %d-feature / %d-action board" % (packed.shape[1], F, A))
    m0 = ROW_META.itemsize
    meta = np.ascontiguousarray(packed[:, :m0]).view(ROW_META).reshape(n)
    x = np.ascontiguousarray(packed[:, m0:m0 + 2 * F]).view("<i2").reshape(n, F)
    vis = np.ascontiguousarray(packed[:, m0 + 2 * F:m0 + 2 * F + 4 * A]).view("<i4").reshape(n, A)
    vs = vis.sum(axis=1, dtype=np.int64).astype(np.float64)
    pi = vis.astype(np.float64) / np.where(vs == 0, 1.0, vs)[:, None]
    out = dict(game_idx=meta["game_idx"].astype(np.int32), move_idx=meta["move_idx"].astype(np.int16),
               move=meta["move"].astype(np.int16), player=meta["player"].astype(np.int8), x=x.astype(np.int16),
               visits=vis.astype(np.int32), pi=pi, z=meta["z"].astype(np.int8),
               max_deepness=meta["max_deepness"].astype(np.int16), tree_size=meta["tree_size"].astype(np.int32),
               terminal_count=meta["terminal_count"].astype(np.int32), q_value=meta["q_value"].astype(np.float32),
               played=meta["played"].astype(np.int16), pad=meta["pad"].astype(np.int16))
    order = np.lexsort((out["move_idx"], out["game_idx"]))
    return {k: v[order] for k, v in out.items()}


def _warn_pool_resets(engine, counters):
    """The reference's search trees are unbounded; a slot's node pool is not.  When the subtree kept by tree reuse would not leave
    room for the next search, the engine starts that move from a fresh root (dbaz_counters.pool_resets) -- say so once per run."""
    n = int(counters.get("pool_resets", 0))
    if n:
        import warnings
        warnings.warn("%d moves (of %d) were searched from a fresh root because the reused subtree did not leave mcts_num_read + 2 nodes "
                      "of the slot's pool free: raise nodes_per_slot (now %d) to keep the reference's tree reuse on every move"
                      % (n, int(counters.get("moves_played", 0)), int(getattr(engine, "nodes_per_slot", 0) or engine.cfg.nodes_per_slot)))


def collect_rows_device(engine, count, first):
    """Play games first .. first+count-1 and return their packed rows as ONE uint8 CUDA tensor
    [n, row_bytes]; the rows never visit the host.  Whenever the device row buffer fills (the
    engine's backpressure: finished games wait in PH_EMIT) its content is cloned on the device and
    the buffer emptied."""
    import torch
    dev = torch.device("cuda", engine.cfg.device)
    chunks = []
    if count > 0:
        engine.selfplay_start(count, first)
        while True:
            engine._ck(engine._L.dbaz_run(engine.h, 0))
            ptr, n, rb = engine.replay_rows_dev()
            if n:
                chunks.append(torch.as_tensor(_DevBuf(ptr, n * rb), device=dev).view(n, rb).clone())
            c = engine.counters()
            engine.replay_rows_clear()
            if c["active_slots"] == 0:
                break
        _warn_pool_resets(engine, c)
        engine._warn_tables_denied()
    if chunks:
        return torch.cat(chunks, dim=0)
    return torch.zeros((0, engine.row_bytes), dtype=torch.uint8, device=dev)


def all_gather_rows(rows, dist):
    """rows: uint8 tensor [n_i, row_bytes] (any device).  Returns (uint8 [sum n_i, row_bytes], counts),
    rank order.  Under RCCL ("nccl") the exchange runs device to device; a gloo group (CPU tests,
    two ranks sharing one GPU) is staged through the host and the result returned on rows' device."""
    import torch
    world = dist.get_world_size()
    home = rows.device
    if rows.is_cuda and dist.get_backend() == "gloo":
        rows = rows.cpu()
    n = torch.tensor([rows.shape[0]], dtype=torch.int64, device=rows.device)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n)
    counts = [int(c.item()) for c in counts]
    mx = max(max(counts), 1)
    padded = torch.zeros((mx, rows.shape[1]), dtype=torch.uint8, device=rows.device)
    padded[: rows.shape[0]] = rows
    out = torch.empty((world * mx, rows.shape[1]), dtype=torch.uint8, device=rows.device)
    dist.all_gather_into_tensor(out, padded)
    keep = torch.cat([out[r * mx: r * mx + counts[r]] for r in range(world)], dim=0)
    return keep.to(home), counts


def gather_replay(engine, dist, synthetic_rows=0):
    """All-gather the finished rows that sit in HBM (dbaz_replay_rows_dev).  Returns
    (total rows, milliseconds).  synthetic_rows > 0 pads every rank's shard to that many rows
    (benchmarking the exchange before games have finished)."""
    import torch
    ptr, n, rb = engine.replay_rows_dev()
    dev = torch.device("cuda", engine.cfg.device)
    if n > 0:
        rows = torch.as_tensor(_DevBuf(ptr, n * rb), device=dev).view(n, rb)
    else:
        rows = torch.zeros((0, rb), dtype=torch.uint8, device=dev)
    if synthetic_rows > n:
        rows = torch.cat([rows, torch.zeros((synthetic_rows - n, rb), dtype=torch.uint8, device=dev)], dim=0)
    torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    allrows, counts = all_gather_rows(rows, dist)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    return int(sum(counts)), ms


# ---------------------------------------------------------------------------------------
# two-model match play + Elo (self_play.compute_elo, self_play.py:309-344)
# ---------------------------------------------------------------------------------------
def elo_rating2(elo0, elo1, n0, n1, K=30):
    """utils/utils.py:124-132."""
    import math
    p1 = 1.0 / (1 + 1.0 * math.pow(10, (elo0 - elo1) / 400))
    p0 = 1 - p1
    return elo0 + K * (n0 * p1 - n1 * p0), elo1 + K * (n1 * p0 - n0 * p1)


def match_winners(samples, generations):
    """(n0, n1): wins of generations[0] / generations[1] counted as the reference does
    (self_play.py:336-338): per game the first row (lowest move_idx) with z == 1 names the winner;
    drawn games have no such row.  Seats: model = player XOR (game_idx & 1)."""
    gen = np.where((samples["player"] ^ (samples["game_idx"] & 1)) == 0, generations[0], generations[1])
    n0 = n1 = 0
    for g in np.unique(samples["game_idx"]):
        r = np.nonzero((samples["game_idx"] == g) & (samples["z"] == 1))[0]
        if len(r) == 0:
            continue
        first = r[np.argmin(samples["move_idx"][r])]
        if gen[first] == generations[0]:
            n0 += 1
        else:
            n1 += 1
    return n0, n1


def compute_elo(elo_params, params, generations, elos, nn_classes=None, rows=None, cols=None, n_slots=None, device=0,
                nn_precision=None, openings=None, endgame=None, endgame_models=(0,), endgame_tables=None, endgame_wait=False,
                leaf_endgame=None, leaf_free=None, leaf_models=(0,), search=None):
    """Reference: self_play.compute_elo(elo_params, [params0, params1], [gen0, gen1], (elo0, elo1)).
    The two models play elo_params.n_games games against each other on the GPU: the model of the
    player to move at the root runs that move's whole search (self_play.py:59,237-239), seats are
    swapped on odd games, the `self_play_override` of elo_params applies (no tree reuse, no noise,
    1200 reads in the shipped configuration, configuration.py:107-113).
    nn_precision: as in generate_games (None = f16x3 for ResNetZero).
    openings: a book of start positions (move sequences or mirror BoxesStates) instead of n_games games from the empty board:
    games 2k and 2k+1 start from opening k % len(openings), so with the seat swap of odd games every opening is played once per
    seating.
    endgame, endgame_models: an endgame.Endgame or endgame.DeepTables that answers the late leaves of the listed models (Engine.attach_endgame); the
    same network with and without it -- params twice, endgame_models=(0,) -- is then one call.  endgame_tables: with a DeepTables, a pool
    of that many tables shared by the slots and by both models (Engine(endgame_tables=N)); endgame_wait: a slot that finds that pool dry
    waits for a table (Engine(endgame_wait=True)), so that the match does not depend on the pool's size.
    leaf_endgame, leaf_free, leaf_models: an endgame.Endgame that solves the leaves with at most leaf_free free edges of the listed
    models from scratch, whatever the root (Engine.attach_leaf_solver).
    search: (spec0, spec1), the search of each model (Engine.match_set_search): a spec is None -- PUCT at the match's reads -- or
    {"reads": n, "gumbel": {...params.self_play.gumbel's dict..., "g_scale": s}}, e.g. Gumbel at 32 reads against PUCT at 800 of the
    same network.  reads is at most the match's mcts_num_read.  Absent, the match is what it always was: the params' own gumbel
    key is dropped.
    Returns (elo0, elo1, n1 / number of decided games)."""
    from .engine import Engine
    p0, p1 = params
    over = _get(elo_params, "self_play_override", {}) or {}
    kw = engine_kwargs_from_params(p0)
    kw.pop("playout_cap", None)  # the cap belongs to self-play: a match searches every move in full
    kw.pop("forced_playouts", None)  # and so do forced playouts
    kw.pop("gumbel", None)  # and the Gumbel root search
    if "reuse_mcts_tree" in over:
        kw["reuse_tree"] = bool(_get(over, "reuse_mcts_tree"))
    if "noise" in over:
        nz = _get(over, "noise")
        kw["noise"] = (float(nz[0]), float(nz[1]))
    m = _get(over, "mcts")
    if m is not None and _get(m, "mcts_num_read") is not None:
        kw["mcts_num_read"] = int(_get(m, "mcts_num_read"))
    if rows is None:
        game = _get(p0, "game")
        dims = _get(game, "dims") or getattr(_get(game, "clazz"), "BOARD_DIM", (3, 3))
        rows, cols = int(dims[0]), int(dims[1])
    n_games = int(_get(elo_params, "n_games"))
    classes = nn_classes or [_get(_get(p, "nn"), "model_class") for p in params]
    models = [classes[0](p0), classes[1](p1)]
    for mdl, gen in zip(models, generations):
        if gen != 0:
            mdl.load_parameters(gen)  # compare_models: generation g itself (self_play.py:190)
    eng = Engine(rows, cols, n_slots or max(1, min(n_games, 4096)), evaluator=models[0].kind, evaluator2=models[1].kind,
                 match_play=True, device=device, nn_precision=nn_precision, endgame=endgame, endgame_models=endgame_models,
                 endgame_tables=endgame_tables, endgame_wait=endgame_wait, leaf_endgame=leaf_endgame, leaf_free=leaf_free,
                 leaf_models=leaf_models, match_search=None if search is None else tuple(match_search_spec(s) for s in search), **kw)
    try:
        for i, mdl in enumerate(models):
            eng.load_state_dict(mdl.state_dict(), mdl.kind, model=i, **mdl.shape)
        if openings is not None and len(openings):
            eng.selfplay_set_start([start_moves(st, rows, cols) for st in openings], 2)
        eng.selfplay_start(n_games, 0)
        eng.run()
        got = eng.fetch_samples()
    finally:
        eng.close()
    n0, n1 = match_winners(got, generations)
    e0, e1 = elo_rating2(elos[0], elos[1], n0, n1, K=30)
    decided = n0 + n1
    return e0, e1, (n1 / decided if decided else float("nan"))


def solver_match(params, generation, n_games, rows, cols, openings=None, solver=None, solver_seed=0, solver_reads=2, nn_class=None,
                 n_slots=None, device=0, nn_precision=None, search=None):
    """The network against perfect play: the absolute measure next to compute_elo's relative one, on boards the exact solver
    holds (at most 31 edges).  The network of `params` / `generation` is model 0, the solved table (dotsboxesaz_amd.solver) model
    1; seats and book as in compute_elo: the network moves first in even games, games 2k and 2k+1 start from opening
    k % len(openings).  solver: a solved Solver of the board (reuse it: a solve costs 2^E bytes); solver_seed picks among the
    table's equally good moves; the table's searches run min(rule, solver_reads) reads (one already finds its move).
    search: the spec of the network's seat, model 0, as in compute_elo (None or absent: PUCT at the params' reads); the table keeps
    solver_reads.
    Returns dict(games, wins, draws, losses -- the network's --, theory = {"win", "draw", "loss"}: games whose start is that
    result for the network's seat under perfect play, held = games in which the network got at least that result, held_rate,
    f32_fallback_evals of the engine's counters, samples = the rows of the games)."""
    from .engine import Engine
    from .solver import Solver
    own = solver is None
    if own:
        solver = Solver(rows, cols, device).solve()
    cls = nn_class or _get(_get(params, "nn"), "model_class")
    model = cls(params)
    if generation != 0:
        model.load_parameters(generation)
    n_games = int(n_games)
    kw = engine_kwargs_from_params(params)
    # the shipped match configuration (configuration.py:107-113): every move from a fresh root -- a reused subtree would carry the
    # other model's priors, and the table's one-hot prior only binds the search from a root whose expansion was counted -- no noise
    kw.update(reuse_tree=False, noise=(0.0, 0.0))
    kw.pop("playout_cap", None)  # the cap belongs to self-play
    kw.pop("forced_playouts", None)
    kw.pop("gumbel", None)
    eng = Engine(rows, cols, n_slots or max(1, min(n_games, 4096)), evaluator=model.kind, evaluator2="solver", match_play=True,
                 device=device, nn_precision=nn_precision, solver=solver, solver_seed=solver_seed, solver_reads=solver_reads,
                 match_search=None if search is None else (match_search_spec(search), None), **kw)
    try:
        eng.load_state_dict(model.state_dict(), model.kind, model=0, **model.shape)
        if openings is not None and len(openings):
            eng.selfplay_set_start([start_moves(st, rows, cols) for st in openings], 2)
        eng.selfplay_start(n_games, 0)
        eng.run()
        got = eng.fetch_samples()
        counters = eng.counters()
    finally:
        eng.close()
    out = match_vs_theory(got, solver)
    out["f32_fallback_evals"] = int(counters["f32_fallback_evals"])
    out["samples"] = got  # the match's rows (Engine.fetch_samples), e.g. for solver.score_samples
    if own:
        solver.close()
    return out


def match_vs_theory(samples, solver):
    """Rows of a match in which model 0 met a perfect model 1 (seats: model = player XOR (game_idx & 1)) -> solver_match's
    counts.  Per game: the network's result is the first row's z seen from the network's seat, the theoretical result of the
    start is Solver.score of the first row, seen from the same seat."""
    first = np.nonzero(samples["move_idx"] == 0)[0]
    g = samples["game_idx"][first]
    seat_is_mover = (samples["player"][first] ^ (g & 1)) == 0  # the network is to move in the first row
    sign = np.where(seat_is_mover, 1, -1)
    z = samples["z"][first].astype(np.int64) * sign
    theory = solver.score(np.asarray(samples["x"])[first].reshape(len(first), solver.F))["value"].astype(np.int64) * sign
    held = int((z >= theory).sum())
    n = len(first)
    return dict(games=n, wins=int((z > 0).sum()), draws=int((z == 0).sum()), losses=int((z < 0).sum()),
                theory=dict(win=int((theory > 0).sum()), draw=int((theory == 0).sum()), loss=int((theory < 0).sum())),
                held=held, held_rate=held / n if n else float("nan"))
