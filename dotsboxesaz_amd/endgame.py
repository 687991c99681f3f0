"""Exact endgame solver for any board (A <= 256): true values of positions with at most 16 free edges.

    python -m dotsboxesaz_amd.endgame --rows 6 --cols 6 --bench 4096 [--free 16]
    python -m dotsboxesaz_amd.endgame --rows 6 --cols 6 --selfplay-bench 8192 [--slots 8192] [--reads 800] [--endgame-reads 0] [--max-free 20]
    python -m dotsboxesaz_amd.endgame --rows 6 --cols 6 --targets-bench 262144
    python -m dotsboxesaz_amd.endgame --rows 6 --cols 6 --deep-bench 4096 [--free 24]
    python -m dotsboxesaz_amd.endgame --rows 6 --cols 6 --tables-bench 64 --free 20
    python -m dotsboxesaz_amd.endgame --rows 6 --cols 6 --tails-bench 1024 --reads 20 --free 24 [--tables 64]
    python -m dotsboxesaz_amd.endgame --rows 6 --cols 6 --replay-bench 1024 --reads 20 --free 20 --tables 64

The solver's D (solver.py) depends only on which edges are still free, so a position with F free edges is a game
over 2^F masks; one workgroup solves it in LDS (csrc/endgame.hip).  No table, no solve step.
DeepEndgame goes further, up to 31 free edges: one root position solved into a table in HBM by the small-board solver's kernels
(csrc/solver.hip), and the root and every position after it answered from that table; score_game_tails uses it per game.
DeepTables is the batched form: a pool of such tables, many roots solved side by side, rows of many games answered in one launch
(score_game_tails(tables=), game_tail_targets; DeepTables.replay_targets does it on packed replay rows without leaving the device:
Coach(exact_targets=DeepTables(...))).  Engine(endgame=DeepTables(rows, cols, max_free=M)) puts such tables inside the
search, one per engine slot (Engine.attach_endgame, dbaz_attach_tables).
"""
import ctypes as C

import numpy as np

from . import _lib
from .solver import ILLEGAL, _margin, edge_actions

MAX_FREE = 16  # ENDGAME_MAX_FREE
PI_MODES = {"keep": 0, "uniform": 1, "restrict": 2}  # dbaz_exact_targets' pi_mode


def target_modes(pi_mode, z_mode):
    """(pi_mode, z_mode) of dbaz_exact_targets from a name ("keep", "uniform", "restrict") or number, and a truth value"""
    if isinstance(pi_mode, str):
        if pi_mode not in PI_MODES:
            raise ValueError("pi_mode %r: one of %s" % (pi_mode, sorted(PI_MODES)))
        pi_mode = PI_MODES[pi_mode]
    return int(pi_mode), int(z_mode)


class Endgame:
    """Endgame scorer of one board size on one GPU.  A > 256 or max_free outside 1 .. 16 raises DbazError before the device is
    touched."""

    ATTACH = "dbaz_attach_endgame"  # the entry Engine.attach_endgame calls with this handle

    def __init__(self, rows, cols, device=0, max_free=MAX_FREE):
        self._L = _lib.load()
        self.rows, self.cols, self.device, self.max_free = int(rows), int(cols), int(device), int(max_free)
        self.H, self.W = self.rows + 1, self.cols + 1
        self.A, self.F = 2 * self.H * self.W, 3 * self.H * self.W
        self.h = C.c_void_p()
        rc = self._L.dbaz_endgame_create(self.rows, self.cols, self.device, self.max_free, C.byref(self.h))
        if rc != _lib.OK:
            self.h = None
            self._ck(rc)
        self.max_free = self.max_free or MAX_FREE
        self.actions = edge_actions(self.rows, self.cols)
        self.n_edges = len(self.actions)

    def _ck(self, rc):
        if rc != _lib.OK:
            msg = self._L.dbaz_endgame_last_error(self.h)
            raise _lib.DbazError(rc, msg.decode() if msg else "error %d" % rc)

    def close(self):
        if getattr(self, "h", None):
            self._L.dbaz_endgame_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def score(self, x, pi=None):
        """x: feature rows int16 [n, 3*H*W] (or [n, 3, H, W]); pi: optional float32 [n, A].  numpy arrays or torch tensors on
        the handle's device; the outputs come back as the same kind, queued on torch's current stream.  Returns dict(value int8
        [n], diff int8 [n], q int8 [n, A], policy_mass float32 [n] or None, n_free int16 [n], solved bool [n]); a row with
        n_free > max_free is not solved: value 0, diff -128, q all -128, policy_mass 0."""
        import torch
        dev = torch.device("cuda", self.device)
        as_numpy = not isinstance(x, torch.Tensor)
        xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.int16) if as_numpy else x).to(device=dev, dtype=torch.int16).reshape(-1, self.F).contiguous()
        n = int(xt.shape[0])
        pt = None
        if pi is not None:
            pt = torch.as_tensor(np.ascontiguousarray(pi, dtype=np.float32) if not isinstance(pi, torch.Tensor) else pi)
            pt = pt.to(device=dev, dtype=torch.float32).reshape(-1, self.A).contiguous()
            if int(pt.shape[0]) != n:
                raise ValueError("pi has %d rows, x has %d" % (pt.shape[0], n))
        value = torch.empty(n, dtype=torch.int8, device=dev)
        diff = torch.empty(n, dtype=torch.int8, device=dev)
        q = torch.empty((n, self.A), dtype=torch.int8, device=dev)
        mass = torch.empty(n, dtype=torch.float32, device=dev) if pt is not None else None
        n_free = torch.empty(n, dtype=torch.int16, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)  # noqa: E731
        with torch.cuda.device(dev):
            self._ck(self._L.dbaz_endgame_score(self.h, C.c_int32(n), ptr(xt), ptr(pt), ptr(value), ptr(diff), ptr(q), ptr(mass), ptr(n_free),
                                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        out = dict(value=value, diff=diff, q=q, policy_mass=mass, n_free=n_free, solved=n_free <= self.max_free)
        if as_numpy:
            out = {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}
        return out

    def targets(self, x, pi, z, pi_mode="restrict", z_mode=True):
        """Exact training targets (dbaz_exact_targets): x as for score(), pi float32 [n, A], z float32 [n] (or [n, 1]).  Rows of
        unfinished games with at most max_free free edges get z = the true result for the mover (z_mode) and pi on the moves that
        keep it -- "uniform": equal shares; "restrict": the given pi renormalised over them (uniform where it has no mass there);
        "keep": pi as it is.  Every other row comes back bit for bit.  Returns (pi', z', info) with info = dict(n_free int16 [n],
        mass float32 [n]: pi's mass on those moves before the relabel, relabelled bool [n]); numpy in, numpy out, or torch tensors
        on the handle's device in and out, queued on torch's current stream.  The caller's arrays are never modified."""
        import torch
        pm, zm = target_modes(pi_mode, z_mode)
        dev = torch.device("cuda", self.device)
        as_numpy = not isinstance(x, torch.Tensor)
        xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.int16) if as_numpy else x).to(device=dev, dtype=torch.int16).reshape(-1, self.F).contiguous()
        n = int(xt.shape[0])
        z_shape = tuple(z.shape)

        def own(t, cols):  # a contiguous float32 copy on the device that this call may write
            t = torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32) if not isinstance(t, torch.Tensor) else t)
            return t.to(device=dev, dtype=torch.float32).reshape(-1, cols).clone(memory_format=torch.contiguous_format)
        pt, zt = own(pi, self.A), own(z, 1).reshape(-1)
        if int(pt.shape[0]) != n or int(zt.shape[0]) != n:
            raise ValueError("x has %d rows, pi %d, z %d" % (n, pt.shape[0], zt.shape[0]))
        n_free = torch.empty(n, dtype=torch.int16, device=dev)
        mass = torch.empty(n, dtype=torch.float32, device=dev)
        relabelled = torch.empty(n, dtype=torch.uint8, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
        with torch.cuda.device(dev):
            self._ck(self._L.dbaz_exact_targets(self.h, C.c_int32(n), ptr(xt), C.c_int32(pm), C.c_int32(zm), ptr(pt), ptr(zt), ptr(n_free), ptr(mass),
                                                ptr(relabelled), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        info = dict(n_free=n_free, mass=mass, relabelled=relabelled != 0)
        zt = zt.reshape(z_shape)
        if as_numpy:
            return pt.cpu().numpy(), zt.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}
        return pt, zt, info

    def policy(self, x, seed=0):
        """The solver as a policy/value evaluator (dbaz_exact_policy), every row solved from scratch: x as for score().  Returns
        (p float32 [n, A] one-hot on an optimal move, v float32 [n] the true result for the mover, solved bool [n]); the pick among
        equally good moves is the first in action order for seed 0, otherwise a function of the position and the seed alone.
        A finished game gets p = 0 and v = its result; a row with more than max_free free edges p = 0, v = 0, solved False."""
        import torch
        dev = torch.device("cuda", self.device)
        as_numpy = not isinstance(x, torch.Tensor)
        xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.int16) if as_numpy else x).to(device=dev, dtype=torch.int16).reshape(-1, self.F).contiguous()
        n = int(xt.shape[0])
        p = torch.empty((n, self.A), dtype=torch.float32, device=dev)
        v = torch.empty(n, dtype=torch.float32, device=dev)
        solved = torch.empty(n, dtype=torch.uint8, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
        with torch.cuda.device(dev):
            self._ck(self._L.dbaz_exact_policy(self.h, C.c_int32(n), ptr(xt), C.c_uint64(int(seed)), ptr(p), ptr(v), ptr(solved),
                                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        out = (p, v, solved != 0)
        return tuple(t.cpu().numpy() for t in out) if as_numpy else out

    def policy_from(self, roots, x, seed=0):
        """The table path the search uses, on its own (dbaz_exact_policy_from): roots int16 [m, 3*H*W], x int16 [m, k, 3*H*W] --
        x[i] are positions that draw further edges of roots[i] (the root itself included).  Root i's subgame is solved once, its k
        rows are answered from the table.  Returns (p [m, k, A], v [m, k]), equal to policy(x, seed)'s wherever roots[i] has at
        most max_free free edges (p = 0, v = 0 elsewhere).  self.last_ms = HIP-event milliseconds of (table kernel, lookup kernel)."""
        import torch
        dev = torch.device("cuda", self.device)
        as_numpy = not isinstance(x, torch.Tensor)
        conv = lambda t: torch.as_tensor(np.ascontiguousarray(t, dtype=np.int16) if not isinstance(t, torch.Tensor) else t).to(device=dev, dtype=torch.int16)  # noqa: E731
        rt = conv(roots).reshape(-1, self.F).contiguous()
        m = int(rt.shape[0])
        xt = conv(x).reshape(m, -1, self.F).contiguous() if m else conv(x).reshape(0, 1, self.F)
        k = int(xt.shape[1])
        p = torch.empty((m, k, self.A), dtype=torch.float32, device=dev)
        v = torch.empty((m, k), dtype=torch.float32, device=dev)
        ms = (C.c_float * 2)()
        ptr = lambda t: C.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
        with torch.cuda.device(dev):
            self._ck(self._L.dbaz_exact_policy_from(self.h, C.c_int32(m), ptr(rt), C.c_int32(k), ptr(xt), C.c_uint64(int(seed)), ptr(p), ptr(v), ms,
                                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        self.last_ms = (float(ms[0]), float(ms[1]))
        return (p.cpu().numpy(), v.cpu().numpy()) if as_numpy else (p, v)


def _row_report(g, x, samples, r):
    """score_endgames' report from the scored rows r (value, q, policy_mass, n_free, solved) of x [n, 3*H*W]; g: the handle"""
    n = len(x)
    solved, n_free = r["solved"], r["n_free"].astype(np.int64)
    played = np.asarray(samples["played"]).astype(np.int64).reshape(n)
    has_move = (played >= 0) & (played < g.A)
    q_played = np.where(has_move, r["q"][np.arange(n), np.clip(played, 0, g.A - 1)], ILLEGAL).astype(np.int64)
    open_ = solved & (r["q"] != ILLEGAL).any(axis=1)  # solved and not a finished game
    played_optimal = has_move & (q_played != ILLEGAL) & (np.sign(_margin(g, x) + q_played) == r["value"])
    z_ok = np.asarray(samples["z"]).reshape(n) == r["value"]
    mass = r["policy_mass"].astype(np.float64)

    def mean(values, where):
        return float(values[where].sum() / where.sum()) if where.any() else float("nan")

    depth = [solved & (n_free == f) for f in range(g.max_free + 1)]
    by_free = dict(rows=np.array([int(d.sum()) for d in depth], np.int64),
                   played_optimal_rate=np.array([mean(played_optimal, d & open_) for d in depth]),
                   optimal_policy_mass=np.array([mean(mass, d & open_) for d in depth]),
                   z_agreement=np.array([mean(z_ok, d) for d in depth]))
    return dict(value=r["value"], policy_mass=r["policy_mass"], played_optimal=played_optimal, n_free=r["n_free"], solved=solved,
                optimal_policy_mass=mean(mass, open_), played_optimal_rate=mean(played_optimal, open_), z_agreement=mean(z_ok, solved),
                coverage=float(solved.mean()) if n else 0.0, by_free=by_free)


def score_endgames(samples, rows=None, cols=None, endgame=None, max_free=MAX_FREE, device=0):
    """Scores the rows Engine.fetch_samples() / generate_games return (x, pi, played, z) on any board: the counterpart of
    solver.score_samples for the rows with at most max_free free edges.
    Per row: value, policy_mass, played_optimal (False for rows without a move and for unsolved rows), n_free, solved.
    Means: optimal_policy_mass and played_optimal_rate over the solved rows of unfinished positions, z_agreement over the solved
    rows, coverage = the share of rows solved.  by_free: arrays of length max_free + 1 indexed by the number of free edges --
    rows (solved rows of that depth), played_optimal_rate, optimal_policy_mass, z_agreement (NaN where there is no row).
    endgame: an Endgame of the rows' board size (its max_free holds).  Without one the board size comes from rows / cols, or from
    x's shape [n, 3, H, W]; flat rows [n, 3*H*W] alone do not tell it."""
    x = np.asarray(samples["x"])
    if endgame is None:
        if rows is None or cols is None:
            if x.ndim != 4:
                raise ValueError("flat feature rows do not tell the board size: pass rows= and cols=, or endgame=Endgame(rows, cols)")
            rows, cols = x.shape[2] - 1, x.shape[3] - 1
        endgame = Endgame(rows, cols, device, max_free)
    g, n = endgame, len(x)
    x = x.reshape(n, g.F)
    r = g.score(x, np.asarray(samples["pi"], dtype=np.float32).reshape(n, g.A))
    return _row_report(g, x, samples, r)


DEEP_FREE = 24  # dbaz_deep_create's default max_free: a table of 16 MiB


class _TableHandle:
    """What DeepEndgame and DeepTables share: a handle of one family of C entries (_API + "_create", "_score", ...) on one board
    and device, its error check, its end, and the rows in / outputs out of score()."""

    _API = None  # "dbaz_deep" or "dbaz_tables"

    def _open(self, rows, cols, device, max_free, *more):
        self._L = _lib.load()
        self.rows, self.cols, self.device, self.max_free = int(rows), int(cols), int(device), int(max_free)
        self.H, self.W = self.rows + 1, self.cols + 1
        self.A, self.F = 2 * self.H * self.W, 3 * self.H * self.W
        self.h = C.c_void_p()
        rc = self._fn("create")(self.rows, self.cols, self.device, self.max_free, *more, C.byref(self.h))
        if rc != _lib.OK:
            self.h = None
            self._ck(rc)
        self.max_free = self.max_free or DEEP_FREE
        self.actions = edge_actions(self.rows, self.cols)
        self.n_edges = len(self.actions)

    def _fn(self, name):
        return getattr(self._L, "%s_%s" % (self._API, name))

    def _ck(self, rc):
        if rc != _lib.OK:
            msg = self._fn("last_error")(self.h)
            raise _lib.DbazError(rc, msg.decode() if msg else "error %d" % rc)

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, x, table_of=None):
        """(device, x is numpy, x int16 [n, 3*H*W] on the device, table_of int32 [n] there or None, n)"""
        import torch
        dev = torch.device("cuda", self.device)
        as_numpy = not isinstance(x, torch.Tensor)
        xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.int16) if as_numpy else x).to(device=dev, dtype=torch.int16).reshape(-1, self.F).contiguous()
        tt = None
        if table_of is not None:
            tt = torch.as_tensor(np.ascontiguousarray(table_of, dtype=np.int32) if not isinstance(table_of, torch.Tensor) else table_of)
            tt = tt.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            if int(tt.shape[0]) != int(xt.shape[0]):
                raise ValueError("table_of has %d entries, x has %d rows" % (tt.shape[0], xt.shape[0]))
        return dev, as_numpy, xt, tt, int(xt.shape[0])

    def _score(self, x, pi, table_of=None):
        """score() of either class: the family's _score entry takes table_of after pi where there is one"""
        import torch
        dev, as_numpy, xt, tt, n = self._rows(x, table_of)
        pt = None
        if pi is not None:
            pt = torch.as_tensor(np.ascontiguousarray(pi, dtype=np.float32) if not isinstance(pi, torch.Tensor) else pi)
            pt = pt.to(device=dev, dtype=torch.float32).reshape(-1, self.A).contiguous()
            if int(pt.shape[0]) != n:
                raise ValueError("pi has %d rows, x has %d" % (pt.shape[0], n))
        value = torch.empty(n, dtype=torch.int8, device=dev)
        diff = torch.empty(n, dtype=torch.int8, device=dev)
        q = torch.empty((n, self.A), dtype=torch.int8, device=dev)
        mass = torch.empty(n, dtype=torch.float32, device=dev) if pt is not None else None
        n_free = torch.empty(n, dtype=torch.int16, device=dev)
        served = torch.empty(n, dtype=torch.uint8, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)  # noqa: E731
        args = [xt, pt] + ([tt] if table_of is not None else []) + [value, diff, q, mass, n_free, served]
        with torch.cuda.device(dev):
            self._ck(self._fn("score")(self.h, C.c_int32(n), *[ptr(t) for t in args], C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        out = dict(value=value, diff=diff, q=q, policy_mass=mass, n_free=n_free, solved=served != 0)
        if as_numpy:
            out = {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}
        return out


class DeepEndgame(_TableHandle):
    """One solved table per position (dbaz_deep_*): solve(root_x) solves the subgame of a root position with at
    most max_free <= 31 free edges into a table of 2^F bytes in HBM; score() and policy() then answer the root and every position
    that follows it from that table.  A > 256 or max_free outside 1 .. 31 raises DbazError before the device is touched."""

    _API = "dbaz_deep"

    def __init__(self, rows, cols, device=0, max_free=DEEP_FREE):
        self._open(rows, cols, device, max_free)
        self.n_free, self.d0, self.solve_ms, self.table_bytes = -1, ILLEGAL, -1.0, 1 << self.max_free

    def _info(self):
        f, b, ms, d0 = C.c_int32(), C.c_int64(), C.c_double(), C.c_int32()
        self._ck(self._L.dbaz_deep_info(self.h, C.byref(f), C.byref(b), C.byref(ms), C.byref(d0)))
        self.n_free, self.table_bytes, self.solve_ms, self.d0 = f.value, b.value, ms.value, d0.value

    def solve(self, root_x, low_bits=0):
        """root_x: ONE feature row int16 [3*H*W] (or [3, H, W]), a numpy array or a tensor anywhere: the geometry is built on the
        host.  Replaces the previous root's table; returns self when the table is complete, with n_free, d0, solve_ms (HIP-event
        time of the solve's kernels) and table_bytes set.  More than max_free free edges raises DbazError (EINVAL) and leaves the
        handle without a table.  low_bits as for Solver.solve."""
        if hasattr(root_x, "detach"):
            root_x = root_x.detach().cpu().numpy()
        row = np.ascontiguousarray(np.asarray(root_x).reshape(-1), dtype=np.int16)
        if row.size != self.F:
            raise ValueError("the root is one feature row of %d values, got %d" % (self.F, row.size))
        rc = self._L.dbaz_deep_solve(self.h, C.c_void_p(row.ctypes.data), int(low_bits))
        if rc != _lib.OK:
            self.n_free, self.d0 = -1, ILLEGAL
            self._ck(rc)
        self._info()
        return self

    def table(self, first=0, count=None):
        """Host copy of T[first : first + count] of the root's 2^n_free entries (default: all of them) as a numpy int8 array."""
        count = (1 << max(self.n_free, 0)) - first if count is None else count
        out = np.empty(max(int(count), 0), np.int8)
        self._ck(self._L.dbaz_deep_table(self.h, C.c_void_p(out.ctypes.data), C.c_int64(first), C.c_int64(count)))
        return out

    def score(self, x, pi=None):
        """Endgame.score's dict from the table, same conventions in and out; solved [n] = the row is served: its free edges are a
        subset of the root's.  A row that is not served gets value 0, diff -128, q all -128, policy_mass 0; n_free is the row's own
        count either way.  Before a successful solve(): DbazError (ESTATE)."""
        return self._score(x, pi)

    def policy(self, x, seed=0):
        """Endgame.policy's (p, v, solved) from the table: the same pick among equally good moves for the same seed; solved [n] =
        the row is served (p = 0, v = 0 where it is not)."""
        import torch
        dev, as_numpy, xt, _, n = self._rows(x)
        p = torch.empty((n, self.A), dtype=torch.float32, device=dev)
        v = torch.empty(n, dtype=torch.float32, device=dev)
        served = torch.empty(n, dtype=torch.uint8, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
        with torch.cuda.device(dev):
            self._ck(self._L.dbaz_deep_policy(self.h, C.c_int32(n), ptr(xt), C.c_uint64(int(seed)), ptr(p), ptr(v), ptr(served),
                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        out = (p, v, served != 0)
        return tuple(t.cpu().numpy() for t in out) if as_numpy else out


DEEP_TABLES = 64  # dbaz_tables_create's default n_tables: a pool of 1 GiB at max_free 24


class DeepTables(_TableHandle):
    """A pool of solved tables (dbaz_tables_*): solve(roots_x) solves up to n_tables root positions side by side,
    root i into table i; score() and targets() then answer rows of many games in one launch, row r from table table_of[r].
    replay_targets() takes packed replay rows on the device instead: roots found, solved and rows relabelled without a host copy.
    A > 256, max_free outside 1 .. 31 or n_tables outside 1 .. 65535 raises DbazError before the device is touched."""

    _API = "dbaz_tables"
    ATTACH = "dbaz_attach_tables"  # the entry Engine.attach_endgame calls with this handle

    def __init__(self, rows, cols, device=0, max_free=DEEP_FREE, n_tables=DEEP_TABLES):
        self.n_tables = int(n_tables)
        self._open(rows, cols, device, max_free, self.n_tables)
        self.n_tables = self.n_tables or DEEP_TABLES
        self.n_solved, self.n_free, self.d0 = 0, np.zeros(0, np.int32), np.zeros(0, np.int32)
        self.solve_ms, self.table_bytes, self.pool_bytes = -1.0, 1 << self.max_free, self.n_tables << self.max_free

    def _info(self):
        n, b, p, ms = C.c_int32(), C.c_int64(), C.c_int64(), C.c_double()
        self._ck(self._L.dbaz_tables_info(self.h, C.byref(n), C.byref(b), C.byref(p), C.byref(ms)))
        self.n_solved, self.table_bytes, self.pool_bytes, self.solve_ms = n.value, b.value, p.value, ms.value
        self.n_free, self.d0 = np.zeros(self.n_solved, np.int32), np.zeros(self.n_solved, np.int32)
        self._ck(self._L.dbaz_tables_roots(self.h, C.c_void_p(self.n_free.ctypes.data), C.c_void_p(self.d0.ctypes.data)))

    def solve(self, roots_x, low_bits=0):
        """roots_x: 1 .. n_tables feature rows int16 [m, 3*H*W] (or [m, 3, H, W]), a numpy array or a tensor anywhere: the
        geometries are built on the host.  Replaces every table of the previous solve; returns self when the tables are complete,
        with n_solved, n_free[m], d0[m], solve_ms (HIP-event time of the solve's kernels, all roots together) and pool_bytes set.
        A root with more than max_free free edges, more roots than tables, or a low_bits that does not fit some root raises
        DbazError (EINVAL) and leaves the handle with n_solved = 0.  low_bits as for DeepEndgame.solve, for every root."""
        if hasattr(roots_x, "detach"):
            roots_x = roots_x.detach().cpu().numpy()
        r = np.ascontiguousarray(np.asarray(roots_x).reshape(-1, self.F), dtype=np.int16)
        rc = self._L.dbaz_tables_solve(self.h, C.c_int32(len(r)), C.c_void_p(r.ctypes.data), int(low_bits))
        if rc != _lib.OK:
            self.n_solved, self.n_free, self.d0 = 0, np.zeros(0, np.int32), np.zeros(0, np.int32)
            self._ck(rc)
        self._info()
        return self

    def table(self, i, first=0, count=None):
        """Host copy of T_i[first : first + count] of root i's 2^n_free[i] entries (default: all of them) as a numpy int8 array."""
        if count is None:
            count = (1 << int(self.n_free[i])) - first if 0 <= i < self.n_solved else 0
        out = np.empty(max(int(count), 0), np.int8)
        self._ck(self._L.dbaz_tables_table(self.h, C.c_int32(int(i)), C.c_void_p(out.ctypes.data), C.c_int64(first), C.c_int64(count)))
        return out

    def score(self, x, table_of, pi=None):
        """DeepEndgame.score's dict for rows of many games: table_of int32 [n] names each row's table, the index of its root in
        the last solve().  solved [n] = the row is served: table_of is in 0 .. n_solved - 1 and the row's free edges are a subset
        of that root's.  Every other row gets the unsolved outputs; n_free is the row's own count either way.  Before a successful
        solve(): DbazError (ESTATE)."""
        return self._score(x, pi, table_of)

    def targets(self, x, table_of, pi, z, pi_mode="restrict", z_mode=True):
        """Endgame.targets from the tables (dbaz_tables_targets), for rows of any depth a table serves: x, pi, z, the modes and
        the returned (pi', z', info) as there, table_of as for score().  A served row of an unfinished game is relabelled; every
        other row comes back bit for bit.  The caller's arrays are never modified."""
        import torch
        pm, zm = target_modes(pi_mode, z_mode)
        dev, as_numpy, xt, tt, n = self._rows(x, table_of)
        z_shape = tuple(z.shape)

        def own(t, cols):  # a contiguous float32 copy on the device that this call may write
            t = torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32) if not isinstance(t, torch.Tensor) else t)
            return t.to(device=dev, dtype=torch.float32).reshape(-1, cols).clone(memory_format=torch.contiguous_format)
        pt, zt = own(pi, self.A), own(z, 1).reshape(-1)
        if int(pt.shape[0]) != n or int(zt.shape[0]) != n:
            raise ValueError("x has %d rows, pi %d, z %d" % (n, pt.shape[0], zt.shape[0]))
        n_free = torch.empty(n, dtype=torch.int16, device=dev)
        mass = torch.empty(n, dtype=torch.float32, device=dev)
        relabelled = torch.empty(n, dtype=torch.uint8, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
        with torch.cuda.device(dev):
            self._ck(self._L.dbaz_tables_targets(self.h, C.c_int32(n), ptr(xt), ptr(tt), C.c_int32(pm), C.c_int32(zm), ptr(pt), ptr(zt), ptr(n_free),
                                                 ptr(mass), ptr(relabelled), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        info = dict(n_free=n_free, mass=mass, relabelled=relabelled != 0)
        zt = zt.reshape(z_shape)
        if as_numpy:
            return pt.cpu().numpy(), zt.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}
        return pt, zt, info


    REPLAY_STATS = ("rows", "games", "roots", "chunks", "relabelled", "finished", "unserved", "z_changed")
    REPLAY_PHASES = ("scan", "group", "geometry", "solve", "relabel")

    def replay_targets(self, rows, pi_mode="restrict", z_mode=True, return_roots=False):
        """Exact targets on packed replay rows (dbaz_replay_exact_targets): rows is a contiguous uint8 CUDA tensor [n, row_bytes]
        on the handle's device, as self_play.collect_rows_device returns it, in any order -- anything else raises ValueError
        before the C call.  It is relabelled IN PLACE: a caller who wants the played targets too clones first.  Per game the
        first row by move_idx with at most max_free free edges roots one table (built and solved on the device, the games going
        through the pool n_tables at a time); that row and every later row of an unfinished position get z = the true result
        (z_mode) and their visits restricted to the moves that keep it ("restrict": 0 elsewhere, 1 on those moves if none was
        visited; "uniform": 1 on them, 0 elsewhere; "keep": untouched).  Every other byte comes back as it was.
        Returns dict(rows, games, roots, chunks, relabelled, finished, unserved, z_changed, by_free int64 [max_free + 1]:
        relabelled rows by free edges, kernel_ms: HIP-event milliseconds of scan, group, geometry, solve, relabel); with
        return_roots also root_of, an int32 CUDA tensor [n]: per row the index of its game's root row if the row is that root or
        comes after it, else -1.  Afterwards the handle holds the last chunk's tables (n_solved, n_free, d0, table(), score())."""
        import torch
        pm, zm = target_modes(pi_mode, z_mode)
        if pm not in (0, 1, 2) or zm not in (0, 1):
            raise ValueError("pi_mode %r / z_mode %r" % (pi_mode, z_mode))
        from .self_play import row_bytes
        rb = row_bytes(self.F, self.A)
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.uint8 or rows.dim() != 2:
            raise ValueError("rows must be a uint8 tensor [n, row_bytes]")
        if not rows.is_cuda or rows.device.index != self.device:
            raise ValueError("rows must live on the handle's device cuda:%d, got %s" % (self.device, rows.device))
        if int(rows.shape[1]) != rb:
            raise ValueError("row_bytes %d: a packed replay row of a %dx%d board has %d" % (rows.shape[1], self.rows, self.cols, rb))
        if not rows.is_contiguous():
            raise ValueError("rows must be contiguous: they are relabelled in place")
        n = int(rows.shape[0])
        dev = rows.device
        root_of = torch.full((n,), -1, dtype=torch.int32, device=dev) if return_roots else None
        st = np.zeros(len(self.REPLAY_STATS) + 32 + len(self.REPLAY_PHASES), np.int64)
        with torch.cuda.device(dev):
            rc = self._L.dbaz_replay_exact_targets(self.h, C.c_void_p(rows.data_ptr() if n else None), C.c_int64(n), C.c_int32(rb), C.c_int32(pm),
                                                   C.c_int32(zm), C.c_void_p(root_of.data_ptr() if return_roots and n else None),
                                                   C.c_void_p(st.ctypes.data), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != _lib.OK:
            self.n_solved, self.n_free, self.d0 = 0, np.zeros(0, np.int32), np.zeros(0, np.int32)
            self._ck(rc)
        if n:
            self._info()
        k = len(self.REPLAY_STATS)
        out = {name: int(st[i]) for i, name in enumerate(self.REPLAY_STATS)}
        out["by_free"] = st[k:k + self.max_free + 1].copy()
        out["kernel_ms"] = {name: float(st[k + 32 + i]) * 1e-6 for i, name in enumerate(self.REPLAY_PHASES)}
        if return_roots:
            out["root_of"] = root_of
        return out


def _game_roots(game, move, n_free, max_free):
    """Game-ordered rows in any order -> (root [g]: per game that has one, the index of its first row by move_idx with at most
    max_free free edges; table_of [n]: per row the position of its game's root in `root` if the row is that root or comes after
    it, else -1; tails: per root the indices of those rows, the root first)."""
    n = len(game)
    order = np.lexsort((move, game))
    by_game = game[order]
    bounds = [0] + (np.nonzero(by_game[1:] != by_game[:-1])[0] + 1).tolist() + [n]  # where a new game starts
    root, table_of, tails = [], np.full(n, -1, np.int32), []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        idx = order[lo:hi]
        late = np.nonzero(n_free[idx] <= max_free)[0]
        if len(late):
            tails.append(idx[late[0]:])
            table_of[tails[-1]] = len(root)
            root.append(tails[-1][0])
    return np.asarray(root, np.int64), table_of, tails


def _tables_handle(tables, x, rows, cols, max_free, device, what):
    if isinstance(tables, DeepTables):
        return tables
    if rows is None or cols is None:
        if x.ndim != 4:
            raise ValueError("flat feature rows do not tell the board size: pass rows= and cols=, or %s" % what)
        rows, cols = x.shape[2] - 1, x.shape[3] - 1
    return DeepTables(rows, cols, device, max_free, int(tables))


def _tail_rows(g, samples):
    """score_game_tails' rows for the handle g: (x int16 [n, 3*H*W], pi float32 [n, A], r: the report's per-row arrays with every
    row unsolved, then root, table_of and tails as _game_roots gives them)"""
    x = np.asarray(samples["x"])
    n = len(x)
    x = np.ascontiguousarray(x.reshape(n, g.F), dtype=np.int16)
    pi = np.ascontiguousarray(np.asarray(samples["pi"], dtype=np.float32).reshape(n, g.A))
    game = np.asarray(samples["game_idx"]).astype(np.int64).reshape(n)
    move = np.asarray(samples["move_idx"]).astype(np.int64).reshape(n)
    n_free = (x[:, g.actions] == 0).sum(axis=1).astype(np.int16)
    r = dict(value=np.zeros(n, np.int8), q=np.full((n, g.A), ILLEGAL, np.int8), policy_mass=np.zeros(n, np.float32), n_free=n_free,
             solved=np.zeros(n, bool))
    return (x, pi, r) + _game_roots(game, move, n_free, g.max_free)


def _score_game_tails_batched(samples, rows, cols, max_free, device, tables):
    """score_game_tails' batched path: the games in chunks of n_tables, one solve and one score per chunk"""
    g = _tables_handle(tables, np.asarray(samples["x"]), rows, cols, max_free, device, "tables=DeepTables(rows, cols)")
    x, pi, r, root, table_of, _ = _tail_rows(g, samples)
    solve_ms = 0.0
    for lo in range(0, len(root), g.n_tables):
        hi = min(lo + g.n_tables, len(root))
        idx = np.nonzero((table_of >= lo) & (table_of < hi))[0]
        got = g.solve(x[root[lo:hi]]).score(x[idx], table_of[idx] - lo, pi[idx])
        solve_ms += g.solve_ms
        for k in ("value", "q", "policy_mass", "solved"):
            r[k][idx] = got[k]
    return dict(_row_report(g, x, samples, r), tables=len(root), solve_ms=solve_ms)


def game_tail_targets(samples, rows=None, cols=None, max_free=DEEP_FREE, tables=DEEP_TABLES, pi_mode="restrict", z_mode=True, device=0):
    """Exact training targets for game-ordered rows, as Engine.fetch_samples() returns them (x, pi, z, game_idx, move_idx), in
    any order: per game the first row, by move_idx, with at most max_free free edges roots one table, and that row and every
    later row of an unfinished position of the game are relabelled from it as Endgame.targets relabels the rows it solves
    (DeepTables.targets); the rows before a game's root come back bit for bit.  The games go through the pool in chunks of its
    n_tables.  tables: the pool's size, or a DeepTables of the rows' board size (its max_free holds).  Returns (pi', z', info)
    as numpy arrays in the caller's row order, z' in z's shape; info = dict(n_free int16 [n], mass float32 [n], relabelled bool
    [n], tables = roots solved)."""
    x = np.asarray(samples["x"])
    g = _tables_handle(tables, x, rows, cols, max_free, device, "tables=DeepTables(rows, cols)")
    n = len(x)
    x = np.ascontiguousarray(x.reshape(n, g.F), dtype=np.int16)
    pi = np.array(np.asarray(samples["pi"], dtype=np.float32).reshape(n, g.A), copy=True)
    z_in = np.asarray(samples["z"], dtype=np.float32)
    z = np.array(z_in.reshape(n), copy=True)
    game = np.asarray(samples["game_idx"]).astype(np.int64).reshape(n)
    move = np.asarray(samples["move_idx"]).astype(np.int64).reshape(n)
    n_free = (x[:, g.actions] == 0).sum(axis=1).astype(np.int16)
    info = dict(n_free=n_free, mass=np.zeros(n, np.float32), relabelled=np.zeros(n, bool))
    root, table_of, _ = _game_roots(game, move, n_free, g.max_free)
    for lo in range(0, len(root), g.n_tables):
        hi = min(lo + g.n_tables, len(root))
        idx = np.nonzero((table_of >= lo) & (table_of < hi))[0]
        p, zz, got = g.solve(x[root[lo:hi]]).targets(x[idx], table_of[idx] - lo, pi[idx], z[idx], pi_mode, z_mode)
        pi[idx], z[idx] = p, zz
        info["mass"][idx], info["relabelled"][idx] = got["mass"], got["relabelled"]
    return pi, z.reshape(z_in.shape), dict(info, tables=len(root))


def score_game_tails(samples, rows=None, cols=None, max_free=DEEP_FREE, device=0, deep=None, tables=None):
    """score_endgames for game-ordered rows, as Engine.fetch_samples() returns them (x, pi, played, z, game_idx, move_idx): per
    game the first row, by move_idx, with at most max_free free edges roots ONE solve (DeepEndgame), and that row and every later
    row of the game are scored from its table; the rows before it are unsolved.  The same keys with the same definitions as
    score_endgames, by_free of length max_free + 1, plus tables = solves done and solve_ms = the sum of their kernel times.
    deep: a DeepEndgame of the rows' board size (its max_free holds); without one the board size comes from rows / cols or from
    x's shape [n, 3, H, W].
    tables: None walks the games one by one as described; a number, or a DeepTables of the rows' board size (its max_free
    holds), takes the games in chunks of that many through a pool of tables -- one solve and one score per chunk, the same
    result; tables = the roots solved, solve_ms = the sum over the chunks."""
    if tables is not None:
        return _score_game_tails_batched(samples, rows, cols, max_free, device, tables)
    x = np.asarray(samples["x"])
    if deep is None:
        if rows is None or cols is None:
            if x.ndim != 4:
                raise ValueError("flat feature rows do not tell the board size: pass rows= and cols=, or deep=DeepEndgame(rows, cols)")
            rows, cols = x.shape[2] - 1, x.shape[3] - 1
        deep = DeepEndgame(rows, cols, device, max_free)
    g = deep
    x, pi, r, _, _, tails = _tail_rows(g, samples)
    solve_ms = 0.0
    for idx in tails:
        got = g.solve(x[idx[0]]).score(x[idx], pi[idx])
        solve_ms += g.solve_ms
        for k in ("value", "q", "policy_mass", "solved"):
            r[k][idx] = got[k]
    return dict(_row_report(g, x, samples, r), tables=len(tails), solve_ms=solve_ms)


def random_rows(rows, cols, n, free, seed=0):
    """n feature rows int16 [n, 3*H*W] with free[i] (or free, a number) free edges in row i: all other edges drawn, at random;
    the closed boxes shared out so that the row is a position of an unfinished game wherever one exists with those edges."""
    rs = np.random.RandomState(seed)
    H, W = rows + 1, cols + 1
    HW, acts = H * W, edge_actions(rows, cols)
    free = np.broadcast_to(np.asarray(free, np.int64), (n,))
    x = np.ones((n, 3 * HW), np.int16)  # sentinel slots are 1, as get_features has them
    x[:, acts] = np.argsort(rs.rand(n, len(acts)), axis=1) >= free[:, None]  # a random permutation's first `free` edges stay free
    e = x[:, :2 * HW] != 0
    closed = np.zeros(n, np.int64)
    for l in range(rows):
        for c in range(cols):
            closed += e[:, l * W + c] & e[:, (l + 1) * W + c] & e[:, HW + l * W + c] & e[:, HW + l * W + c + 1]
    x[:, 2 * HW:] = (rows * cols - 2 * (closed // 2))[:, None]
    return x


def random_descendants(rows, cols, root, n, seed=0):
    """n feature rows int16 [n, 3*H*W] that draw further edges of the feature row `root`: row i keeps a random subset of the
    root's free edges, of a size uniform in 0 .. F; plane 2 as random_rows sets it."""
    rs = np.random.RandomState(seed)
    H, W = rows + 1, cols + 1
    HW, acts = H * W, edge_actions(rows, cols)
    root = np.asarray(root, np.int16).reshape(3 * HW)
    free = acts[root[acts] == 0]
    x = np.repeat(root[None], n, axis=0)
    keep = rs.randint(0, len(free) + 1, n)
    x[:, free] = np.argsort(rs.rand(n, len(free)), axis=1) >= keep[:, None]
    e = x[:, :2 * HW] != 0
    closed = np.zeros(n, np.int64)
    for l in range(rows):
        for c in range(cols):
            closed += e[:, l * W + c] & e[:, (l + 1) * W + c] & e[:, HW + l * W + c] & e[:, HW + l * W + c + 1]
    x[:, 2 * HW:] = (rows * cols - 2 * (closed // 2))[:, None]
    return x


def _deep_bench(a):
    """One root with a.free free edges: HIP-event milliseconds of dbaz_deep_solve (median of 5 after a warm-up), rows/s of one
    dbaz_deep_score call on a.deep_bench descendants of the root, and rows/s of one dbaz_endgame_score call on those among them
    with at most 16 free edges -- the two scorers alternating in the same run, outputs preallocated, median of 5 after a warm-up.
    Stops if the two disagree on a row both answer."""
    import torch
    n, free = a.deep_bench, a.free
    d = DeepEndgame(a.rows, a.cols, a.device, max(free, 1))
    free = min(free, d.n_edges)
    g = Endgame(a.rows, a.cols, a.device)
    dev = torch.device("cuda", d.device)
    root = random_rows(a.rows, a.cols, 1, free, seed=5)[0]
    solve_ms = [d.solve(root, a.low_bits).solve_ms for _ in range(6)][1:]
    x = random_descendants(a.rows, a.cols, root, n, seed=6)
    left = (x[:, d.actions] == 0).sum(axis=1)
    xs = {"deep": torch.as_tensor(x).to(dev), "endgame": torch.as_tensor(x[left <= MAX_FREE]).to(dev)}
    value, diff = torch.empty(n, dtype=torch.int8, device=dev), torch.empty(n, dtype=torch.int8, device=dev)
    q = torch.empty((n, d.A), dtype=torch.int8, device=dev)
    n_free = torch.empty(n, dtype=torch.int16, device=dev)
    served = torch.empty(n, dtype=torch.uint8, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ms = dict(deep=[], endgame=[])
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for i in range(6):
            for which in ("deep", "endgame"):
                xt = xs[which]
                m = C.c_int32(int(xt.shape[0]))
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                if which == "deep":
                    d._ck(d._L.dbaz_deep_score(d.h, m, ptr(xt), None, ptr(value), ptr(diff), ptr(q), None, ptr(n_free), ptr(served), stream))
                else:
                    g._ck(g._L.dbaz_endgame_score(g.h, m, ptr(xt), None, ptr(value), ptr(diff), ptr(q), None, ptr(n_free), stream))
                t1.record()
                t1.synchronize()
                if i:  # the first run warms up
                    ms[which].append(t0.elapsed_time(t1))
            if i == 0:
                assert bool(served.all().item())  # after the deep call of this round
    n_late = int(xs["endgame"].shape[0])
    if n_late:  # a table of any size checks itself against the per-row solver on the rows both answer
        a_, b_ = d.score(xs["endgame"]), g.score(xs["endgame"])
        assert all(torch.equal(a_[k], b_[k]) for k in ("value", "diff", "q", "n_free")), "the table and the per-row solver disagree"
    deep_ms, endgame_ms = float(np.median(ms["deep"])), float(np.median(ms["endgame"]))
    out = dict(rows=a.rows, cols=a.cols, E=d.n_edges, free=int(free), table_bytes=1 << free, d0=d.d0, solve_ms=round(float(np.median(solve_ms)), 4),
               deep_rows=int(n), deep_score_ms=round(deep_ms, 4), deep_rows_per_s=round(n / (deep_ms * 1e-3)),
               endgame_rows=n_late, endgame_score_ms=round(endgame_ms, 4), endgame_rows_per_s=round(n_late / (endgame_ms * 1e-3)) if n_late else 0)
    d.close()
    g.close()
    return out


def _tables_bench(a):
    """a.tables_bench generated roots with a.free free edges each (random_rows, one seed per root), solved two ways that alternate
    in the same process: one dbaz_deep_solve call per root on a DeepEndgame, and ONE dbaz_tables_solve call for all of them on a
    DeepTables.  Per way the HIP-event milliseconds of the solves' kernels and the host wall clock around the calls plus a
    synchronise, each as the median of 5 rounds after a warm-up round, and per root.  Then every batched table is compared with
    the sequential one."""
    import time
    import torch
    n, free = a.tables_bench, a.free
    d = DeepEndgame(a.rows, a.cols, a.device, max(free, 1))
    free = min(free, d.n_edges)
    t = DeepTables(a.rows, a.cols, a.device, max(free, 1), n)
    dev = torch.device("cuda", d.device)
    roots = np.ascontiguousarray(np.concatenate([random_rows(a.rows, a.cols, 1, free, seed=1000 + i) for i in range(n)]))
    ms_out = C.c_double()
    ev, wall = dict(sequential=[], batched=[]), dict(sequential=[], batched=[])
    for i in range(6):
        for which in ("sequential", "batched"):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if which == "sequential":
                ms = 0.0
                for r in roots:
                    d._ck(d._L.dbaz_deep_solve(d.h, C.c_void_p(r.ctypes.data), int(a.low_bits)))
                    d._ck(d._L.dbaz_deep_info(d.h, None, None, C.byref(ms_out), None))
                    ms += ms_out.value
            else:
                t._ck(t._L.dbaz_tables_solve(t.h, C.c_int32(n), C.c_void_p(roots.ctypes.data), int(a.low_bits)))
                t._ck(t._L.dbaz_tables_info(t.h, None, None, None, C.byref(ms_out)))
                ms = ms_out.value
            torch.cuda.synchronize(dev)
            dt = (time.perf_counter() - t0) * 1e3
            if i:  # the first round warms up
                ev[which].append(ms)
                wall[which].append(dt)
    t._info()
    for i in range(n):  # the command checks itself
        assert np.array_equal(t.table(i), d.solve(roots[i], a.low_bits).table()), "table %d: the batched and the sequential solve disagree" % i
        assert t.d0[i] == d.d0 and t.n_free[i] == d.n_free
    out = dict(rows=a.rows, cols=a.cols, roots=int(n), free=int(free), table_bytes=1 << free, pool_bytes=t.pool_bytes, tables_equal=True)
    for which in ("sequential", "batched"):
        e_, w_ = float(np.median(ev[which])), float(np.median(wall[which]))
        out[which] = dict(event_ms=round(e_, 4), wall_ms=round(w_, 4), event_ms_per_root=round(e_ / n, 5), wall_ms_per_root=round(w_ / n, 5))
    out["event_speedup"] = round(out["sequential"]["event_ms"] / out["batched"]["event_ms"], 3)
    out["wall_speedup"] = round(out["sequential"]["wall_ms"] / out["batched"]["wall_ms"], 3)
    d.close()
    t.close()
    return out


def _tails_bench(a):
    """a.tails_bench complete self-play games (formula evaluator, a.reads reads per move), their game-ordered rows scored by
    score_game_tails' game-by-game path and by its batched path (tables=a.tables), alternating: host wall clock of each call,
    the median of 5 rounds after a warm-up round.  Stops if the two reports differ."""
    import time
    from .engine import Engine
    e = Engine(a.rows, a.cols, min(a.tails_bench, 8192), mcts_num_read=a.reads, evaluator="formula", device=a.device)
    e.selfplay_start(a.tails_bench, 0)
    e.run()
    rows = e.fetch_samples()
    e.close()
    max_free = DEEP_FREE if a.free is None else a.free
    deep = DeepEndgame(a.rows, a.cols, a.device, max_free)
    pool = DeepTables(a.rows, a.cols, a.device, max_free, a.tables)
    sec, got = dict(sequential=[], batched=[]), {}
    for i in range(6):
        for which in ("sequential", "batched"):
            t0 = time.perf_counter()
            kw = dict(deep=deep) if which == "sequential" else dict(tables=pool)
            got[which] = score_game_tails(rows, **kw)
            if i:  # the first round warms up
                sec[which].append(time.perf_counter() - t0)
    for k in ("value", "policy_mass", "played_optimal", "n_free", "solved"):
        assert np.array_equal(got["sequential"][k], got["batched"][k]), k
    assert got["sequential"]["tables"] == got["batched"]["tables"]
    s, b = float(np.median(sec["sequential"])), float(np.median(sec["batched"]))
    out = dict(rows=a.rows, cols=a.cols, games=int(a.tails_bench), sample_rows=len(rows["z"]), reads=a.reads, max_free=max_free, pool_tables=a.tables,
               tables=int(got["batched"]["tables"]), coverage=round(got["batched"]["coverage"], 4), sequential_s=round(s, 4), batched_s=round(b, 4),
               sequential_solve_ms=round(got["sequential"]["solve_ms"], 3), batched_solve_ms=round(got["batched"]["solve_ms"], 3),
               speedup=round(s / b, 3))
    deep.close()
    pool.close()
    return out


def _replay_bench(a):
    """a.replay_bench complete self-play games (formula evaluator, a.reads reads per move), their packed rows left on the device
    (self_play.collect_rows_device): DeepTables.replay_targets on them next to game_tail_targets(tables=) on the same rows
    unpacked on the host, alternating in one process, a.repeats (at least 5) timed rounds after a warm-up round, the packed rows
    restored before every round.  Per route the host wall clock around the call (median, min, max); for the device route also
    the HIP-event time of its kernels, phase by phase.  Stops if the two routes relabel different rows or disagree on a z."""
    import time
    import torch
    from . import self_play as sp
    from .engine import Engine
    e = Engine(a.rows, a.cols, min(a.replay_bench, 8192), mcts_num_read=a.reads, evaluator="formula", device=a.device)
    packed0 = sp.collect_rows_device(e, a.replay_bench, 0)
    F, A = e.F, e.A
    e.close()
    host0 = packed0.cpu().numpy()
    samples = sp.unpack_rows(host0, F, A)
    max_free = DEEP_FREE if a.free is None else a.free
    pool = DeepTables(a.rows, a.cols, a.device, max_free, a.tables)
    dev = packed0.device
    packed = packed0.clone()
    wall, phases, stats, got = dict(device=[], host=[]), [], None, None
    for i in range(max(a.repeats, 5) + 1):
        packed.copy_(packed0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        stats = pool.replay_targets(packed)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        got = game_tail_targets(samples, tables=pool)
        t2 = time.perf_counter()
        if i:  # the first round warms up
            wall["device"].append(t1 - t0)
            wall["host"].append(t2 - t1)
            phases.append(stats["kernel_ms"])
    after = sp.unpack_rows(packed.cpu().numpy(), F, A)
    before = sp.unpack_rows(host0, F, A)
    changed = (after["z"] != before["z"]) | (after["visits"] != before["visits"]).any(axis=1)
    assert stats["relabelled"] == int(got[2]["relabelled"].sum()) and not (changed & ~got[2]["relabelled"]).any(), "the two routes relabel different rows"
    assert np.array_equal(after["z"][got[2]["relabelled"]].astype(np.float32), np.asarray(got[1]).reshape(-1)[got[2]["relabelled"]]), "z differs"
    out = dict(rows=a.rows, cols=a.cols, games=int(a.replay_bench), reads=a.reads, max_free=pool.max_free, pool_tables=pool.n_tables, runs=len(wall["device"]),
               sample_rows=stats["rows"], **{k: stats[k] for k in DeepTables.REPLAY_STATS[2:]})
    for which in ("device", "host"):
        w = np.asarray(wall[which]) * 1e3
        out[which] = dict(wall_ms=round(float(np.median(w)), 3), wall_ms_min=round(float(w.min()), 3), wall_ms_max=round(float(w.max()), 3),
                          rows_per_s=round(stats["rows"] / (float(np.median(w)) * 1e-3)))
    out["device"]["kernel_ms"] = {k: round(float(np.median([p[k] for p in phases])), 4) for k in DeepTables.REPLAY_PHASES}
    out["device"]["kernel_ms_total"] = round(float(np.median([sum(p.values()) for p in phases])), 4)
    spread = max(out[w]["wall_ms_max"] - out[w]["wall_ms_min"] for w in ("device", "host"))
    out["speedup"] = round(out["host"]["wall_ms"] / out["device"]["wall_ms"], 3)
    out["device_faster"] = bool(out["host"]["wall_ms"] - out["device"]["wall_ms"] > spread)  # by more than the larger spread
    pool.close()
    return out


def _bench(g, n, free):
    """HIP-event milliseconds of one dbaz_endgame_score call on n rows that all have `free` free edges, and on n rows with n_free
    uniform in 0 .. 16: outputs preallocated, median of 5 after a warm-up"""
    import torch
    dev = torch.device("cuda", g.device)
    value, diff = torch.empty(n, dtype=torch.int8, device=dev), torch.empty(n, dtype=torch.int8, device=dev)
    q = torch.empty((n, g.A), dtype=torch.int8, device=dev)
    n_free = torch.empty(n, dtype=torch.int16, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    p, v = torch.empty((n, g.A), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    solved = torch.empty(n, dtype=torch.uint8, device=dev)

    def timed(x, policy=False):
        ms = []
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for i in range(6):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                if policy:
                    g._ck(g._L.dbaz_exact_policy(g.h, C.c_int32(n), ptr(x), C.c_uint64(7), ptr(p), ptr(v), ptr(solved), stream))
                else:
                    g._ck(g._L.dbaz_endgame_score(g.h, C.c_int32(n), ptr(x), None, ptr(value), ptr(diff), ptr(q), None, ptr(n_free), stream))
                t1.record()
                t1.synchronize()
                if i:  # the first run warms up
                    ms.append(t0.elapsed_time(t1))
        return float(np.median(ms))

    out = dict(bench_rows=int(n), free=int(free))
    mixed = np.random.RandomState(1).randint(0, MAX_FREE + 1, n)
    for name, f in (("deep", free), ("mixed", np.minimum(mixed, g.n_edges))):
        x = torch.as_tensor(random_rows(g.rows, g.cols, n, np.minimum(f, g.n_edges))).to(dev)
        ms = timed(x)
        assert np.array_equal(n_free.cpu().numpy(), np.broadcast_to(np.minimum(f, g.n_edges), (n,)))
        out[name + "_ms"] = round(ms, 4)
        out[name + "_rows_per_s"] = round(n / (ms * 1e-3))
        out[name + "_policy_ms"] = round(timed(x, policy=True), 4)  # dbaz_exact_policy: the same solve, the evaluator's epilogue
        # the search's two kernels on the same rows: k_endgame_table (n tables), k_endgame_eval (n leaves, each its own root)
        both = []
        for i in range(6):
            g.policy_from(x, x.reshape(n, 1, -1), 7)
            if i:
                both.append(g.last_ms)
        out[name + "_table_ms"] = round(float(np.median([b[0] for b in both])), 4)
        out[name + "_eval_ms"] = round(float(np.median([b[1] for b in both])), 4)
    return out


def _targets_bench(g, n):
    """HIP-event milliseconds of one dbaz_exact_targets call ("restrict", solved z) next to one dbaz_endgame_score call on the same
    n rows, alternating in the same run: outputs preallocated, median of 5 after a warm-up.  Two batches of random_rows: n_free
    uniform in 0 .. 16, and a self-play-like mix with 70 % of the rows at n_free in 17 .. 40 (which neither call solves)."""
    import torch
    dev = torch.device("cuda", g.device)
    value, diff = torch.empty(n, dtype=torch.int8, device=dev), torch.empty(n, dtype=torch.int8, device=dev)
    q = torch.empty((n, g.A), dtype=torch.int8, device=dev)
    n_free = torch.empty(n, dtype=torch.int16, device=dev)
    mass = torch.empty(n, dtype=torch.float32, device=dev)
    relabelled = torch.empty(n, dtype=torch.uint8, device=dev)
    rs = np.random.RandomState(1)
    pi0 = torch.as_tensor(rs.rand(n, g.A).astype(np.float32)).to(dev)
    z0 = torch.as_tensor((np.arange(n) % 3 - 1).astype(np.float32)).to(dev)
    pi, z = pi0.clone(), z0.clone()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    uniform = rs.randint(0, MAX_FREE + 1, n)
    mix = np.where(rs.rand(n) < 0.7, rs.randint(MAX_FREE + 1, 41, n), rs.randint(0, MAX_FREE + 1, n))
    out = dict(targets_bench_rows=int(n))
    for name, f in (("uniform", uniform), ("mix", mix)):
        f = np.minimum(f, g.n_edges)
        x = torch.as_tensor(random_rows(g.rows, g.cols, n, f)).to(dev)
        ms = dict(targets=[], score=[])
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for i in range(6):
                pi.copy_(pi0)  # the call relabels in place: every run starts from the same rows
                z.copy_(z0)
                for which in ("targets", "score"):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    if which == "targets":
                        g._ck(g._L.dbaz_exact_targets(g.h, C.c_int32(n), ptr(x), C.c_int32(2), C.c_int32(1), ptr(pi), ptr(z), ptr(n_free), ptr(mass),
                                                      ptr(relabelled), stream))
                    else:
                        g._ck(g._L.dbaz_endgame_score(g.h, C.c_int32(n), ptr(x), None, ptr(value), ptr(diff), ptr(q), None, ptr(n_free), stream))
                    t1.record()
                    t1.synchronize()
                    if i:  # the first run warms up
                        ms[which].append(t0.elapsed_time(t1))
        assert np.array_equal(n_free.cpu().numpy(), f)
        out[name + "_solvable"] = int((f <= g.max_free).sum())
        out[name + "_relabelled"] = int(relabelled.sum().item())
        out[name + "_targets_ms"] = round(float(np.median(ms["targets"])), 4)
        out[name + "_score_ms"] = round(float(np.median(ms["score"])), 4)
        out[name + "_targets_rows_per_s"] = round(n / (out[name + "_targets_ms"] * 1e-3))
    return out


def _selfplay_bench(a):
    """n complete self-play games with a random-init ResNetZero (noise, tree reuse: bench.py --full-games' engine), once without
    and once with the endgame tables attached: games/s, network evaluations per game, tables solved.  Each figure is the median
    of a.repeats runs after one warm-up run.  --max-free M > 16: three engines -- plain, Endgame(16) and DeepTables(max_free=M)
    attached -- each with the table_bytes of its slot tables.  --pool N adds a fourth, DeepTables(max_free=M) with a pool of N tables
    shared by the slots (Engine(endgame_tables=N)): its high_water, denied and the pool's table_bytes.  deep=0 with --pool leaves
    the per-slot deep engine out (its n_slots << M bytes may not fit where the pool does).  --wait adds the pool in wait mode
    (Engine(endgame_wait=True)), with --endgame-reads if given -- the deny-mode pool takes no read cap and runs without one: its
    waited slot-passes, the peak of the slots waiting at once (looked at every 256 steps), evaluations per game and games/s.
    --leaf-free L[,L...] adds, per L, an engine with the leaf solver alone (Engine(leaf_endgame=Endgame(16), leaf_free=L)) and one
    with the leaf solver next to the table attach asked for (the pool if --pool, else the per-slot tables): leaves solved per game
    by F next to the other figures.  And "leaf_idle": the per-step time of the attach where no leaf qualifies -- the first steps of
    fresh games, the same engine with and without the attach, alternating."""
    import sys
    import time
    import torch
    from . import nn as dnn
    from .engine import Engine

    def play(g, pool=None, wait=False, leaf=None):
        peak_waiting = 0
        eng = Engine(a.rows, a.cols, a.slots, mcts_num_read=a.reads, noise=(0.8, 0.25), reuse_tree=True, evaluator="resnet", seed=1000,
                     device=a.device, endgame=g, endgame_reads=0 if pool and not wait else a.endgame_reads, endgame_tables=pool, endgame_wait=wait,
                     leaf_endgame=leaf_g if leaf else None, leaf_free=leaf, endgame_seed=0)
        torch.manual_seed(0)
        model = dnn.ResNetZero(dnn.resnet_params(a.rows, a.cols, a.channels, a.blocks))
        eng.load_state_dict(model.state_dict(), "resnet", **model.shape)
        runs = []
        for i in range(a.repeats + 1):
            solved0 = eng.endgame_stats()[0]
            leaves0 = eng.leaf_solves()["by_free"]
            eng.sync()
            t0 = time.perf_counter()
            eng.selfplay_start(a.selfplay_bench, 0)
            if wait:  # in pieces, to see how many slots wait at once
                while eng.counters()["active_slots"]:
                    eng.run(max_steps=256)
                    if eng.counters()["blocked_slots"]:
                        eng._drained.append(eng._fetch_once())
                    peak_waiting = max(peak_waiting, eng.table_pool_waits()["waiting"])
            else:
                eng.run()
            n_rows = len(eng.fetch_samples()["z"])
            dt = time.perf_counter() - t0
            c = eng.counters()
            print("selfplay-bench: %s%s%s%s run %d of %d, %.1f s" % (type(g).__name__, " pool %d" % pool if pool else "", " wait" if wait else "",
                                                                   " leaf %d" % leaf if leaf else "", i, a.repeats, dt),
                  file=sys.stderr, flush=True)
            if i:  # the first run warms up
                runs.append(dict(games_per_s=c["games_finished"] / dt, nn_evals_per_game=c["nn_evals"] / max(1, c["games_finished"]),
                                 rows_per_game=n_rows / max(1, c["games_finished"]), tables_solved=eng.endgame_stats()[0] - solved0,
                                 seconds=dt))
                if leaf:
                    games = max(1, c["games_finished"])
                    by = [(n1 - n0) / games for n0, n1 in zip(leaves0, eng.leaf_solves()["by_free"])]
                    runs[-1].update(leaves_solved_per_game=sum(by), **{"leaves_F%d" % f: by[f] for f in range(1, leaf + 1)})
        tp, tw = eng.table_pool(), eng.table_pool_waits()
        eng.close()
        out = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
        if leaf:
            out["leaves_solved_per_game_by_free"] = {f: out.pop("leaves_F%d" % f) for f in range(1, leaf + 1)}
        if pool:  # counted over the warm-up and the timed runs together
            out.update(high_water=tp["high_water"], denied=tp["denied"], in_use_at_end=tp["in_use"])
        if wait:
            out.update(waited=tw["waited"], peak_waiting=peak_waiting, waiting_at_end=tw["waiting"], endgame_reads=a.endgame_reads)
        return out

    def idle_cost(leaf, steps=200, rounds=5):
        """ms per step over the first `steps` steps of fresh games (no leaf anywhere near `leaf` free edges), plain and attached in turn"""
        engs = {}
        for name, lf in (("plain", None), ("attached", leaf)):
            engs[name] = Engine(a.rows, a.cols, a.slots, mcts_num_read=a.reads, noise=(0.8, 0.25), reuse_tree=True, evaluator="resnet", seed=1000,
                                device=a.device, leaf_endgame=leaf_g if lf else None, leaf_free=lf)
            torch.manual_seed(0)
            model = dnn.ResNetZero(dnn.resnet_params(a.rows, a.cols, a.channels, a.blocks))
            engs[name].load_state_dict(model.state_dict(), "resnet", **model.shape)
        ms = {k: [] for k in engs}
        for i in range(rounds + 1):
            for name, eng in engs.items():
                eng.selfplay_start(a.slots, 0)
                eng.step(8)
                eng.sync()
                t0 = time.perf_counter()
                eng.step(steps)
                eng.sync()
                if i:  # the first round warms up
                    ms[name].append(1e3 * (time.perf_counter() - t0) / steps)
        solved = engs["attached"].leaf_solves()["total"]
        for eng in engs.values():
            eng.close()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        return dict(leaf_free=leaf, steps=steps, rounds=rounds, ms_per_step=med, ms_per_step_all={k: [round(x, 4) for x in v] for k, v in ms.items()},
                    attach_cost_ms=med["attached"] - med["plain"], spread_ms=max(max(v) - min(v) for v in ms.values()), leaves_solved=solved)

    leaves = [int(x) for x in str(a.leaf_free).split(",") if x] if a.leaf_free else []
    leaf_g = Endgame(a.rows, a.cols, a.device, MAX_FREE) if leaves else None

    def leaf_runs(out, g, pool):
        for lf in leaves:
            out["leaf%d" % lf] = play(None, leaf=lf)
            out["leaf%d_with_tables" % lf] = play(g, pool or None, leaf=lf)
        if leaves:
            out["leaf_idle"] = idle_cost(max(leaves))
            leaf_g.close()

    if a.max_free > MAX_FREE:
        # past 16 free edges the slot tables are a DeepTables' (dbaz_attach_tables): plain, Endgame(16) and deep side by side
        g, d = Endgame(a.rows, a.cols, a.device, MAX_FREE), DeepTables(a.rows, a.cols, a.device, max_free=a.max_free)
        out = dict(rows=a.rows, cols=a.cols, games=a.selfplay_bench, slots=a.slots, reads=a.reads, max_free=d.max_free, endgame_reads=a.endgame_reads,
                   plain=dict(play(None), table_bytes=0), endgame16=dict(play(g), table_bytes=a.slots << MAX_FREE))
        if a.pool > 0:
            out["pooled"] = dict(play(d, a.pool), n_tables=a.pool, table_bytes=a.pool << d.max_free)
            if a.wait:  # no search is denied: the games of the per-slot deep engine, at the price of idle slot-passes
                out["pooled_wait"] = dict(play(d, a.pool, True), n_tables=a.pool, table_bytes=a.pool << d.max_free)
        if a.pool <= 0 or a.per_slot_deep:
            out["deep"] = dict(play(d), table_bytes=a.slots << d.max_free)
        best = out["deep"] if "deep" in out else out["pooled"]
        out["speedup"] = best["games_per_s"] / out["plain"]["games_per_s"]
        out["speedup_over_16"] = best["games_per_s"] / out["endgame16"]["games_per_s"]
        if "deep" in out and "pooled" in out:  # with denied == 0 the same games: the difference is the cost of the pool's two launches
            out["pooled_over_deep"] = out["pooled"]["games_per_s"] / out["deep"]["games_per_s"]
        # the one relation that must hold on the same games: the deeper tables take more leaves away from the network.  A pool
        # that ran dry does not play the same games (its denied searches go to the network), so nothing is asserted of it
        out["deep_saves_nn_evals"] = best["nn_evals_per_game"] < out["endgame16"]["nn_evals_per_game"]
        assert out["deep_saves_nn_evals"] or ("deep" not in out and out["pooled"]["denied"] > 0), out
        leaf_runs(out, d, a.pool if a.pool > 0 else 0)
        g.close()
        d.close()
        return out
    g = Endgame(a.rows, a.cols, a.device, a.max_free)
    out = dict(rows=a.rows, cols=a.cols, games=a.selfplay_bench, slots=a.slots, reads=a.reads, max_free=g.max_free,
               endgame_reads=a.endgame_reads, table_bytes=a.slots * max(16, 1 << g.max_free), plain=play(None), endgame=play(g))
    out["speedup"] = out["endgame"]["games_per_s"] / out["plain"]["games_per_s"]
    leaf_runs(out, g, 0)
    g.close()
    return out


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(description="time the endgame solver on generated rows and print one JSON line")
    ap.add_argument("--rows", type=int, default=6)
    ap.add_argument("--cols", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--max-free", type=int, default=MAX_FREE)
    ap.add_argument("--bench", type=int, default=4096, metavar="N", help="rows per timed call (median of 5 after a warm-up)")
    ap.add_argument("--free", type=int, default=None,
                    help="free edges of every row of the first batch (default 16); --deep-bench: of the root (default 24)")
    ap.add_argument("--deep-bench", type=int, default=0, metavar="N",
                    help="solve one root with --free free edges into an HBM table (DeepEndgame), then time dbaz_deep_score on N descendants "
                         "next to dbaz_endgame_score on those of them with at most 16 free edges")
    ap.add_argument("--low-bits", type=int, default=0, help="--deep-bench, --tables-bench: 0 = default, L = LDS subcube of 2^L masks, -1 = plain kernel")
    ap.add_argument("--tables-bench", type=int, default=0, metavar="N",
                    help="solve N generated roots with --free free edges (default 20) by N dbaz_deep_solve calls and by one dbaz_tables_solve call, "
                         "alternating; then compare the tables")
    ap.add_argument("--tails-bench", type=int, default=0, metavar="N",
                    help="play N self-play games (formula evaluator, --reads) and time score_game_tails on their rows game by game and with "
                         "--tables tables, max_free = --free (default 24)")
    ap.add_argument("--tables", type=int, default=DEEP_TABLES, help="--tails-bench, --replay-bench: tables of the pool")
    ap.add_argument("--replay-bench", type=int, default=0, metavar="N",
                    help="play N self-play games (formula evaluator, --reads) and time DeepTables.replay_targets on their packed rows on the "
                         "device next to game_tail_targets on the same rows on the host, max_free = --free (default 24), --tables tables")
    ap.add_argument("--selfplay-bench", type=int, default=0, metavar="N",
                    help="play N complete self-play games with a random-init ResNetZero, with and without the endgame tables attached")
    ap.add_argument("--targets-bench", type=int, default=0, metavar="N",
                    help="time dbaz_exact_targets next to dbaz_endgame_score on N generated rows: n_free uniform in 0 .. 16, and a self-play-like mix")
    ap.add_argument("--slots", type=int, default=0, help="--selfplay-bench: engine slots (default min(N, 8192))")
    ap.add_argument("--pool", type=int, default=0, metavar="N",
                    help="--selfplay-bench with --max-free > 16: a fourth engine whose slots share a pool of N deep tables")
    ap.add_argument("--wait", action="store_true",
                    help="--selfplay-bench with --pool: a further engine whose pool is in wait mode (a slot that finds it dry waits for a table)")
    ap.add_argument("--per-slot-deep", type=int, default=1,
                    help="--selfplay-bench with --pool: 0 leaves out the engine with one deep table per slot (slots << max_free bytes)")
    ap.add_argument("--leaf-free", default="", metavar="L[,L...]",
                    help="--selfplay-bench: per L two further engines, the leaf solver (leaves with at most L free edges solved from scratch) alone "
                         "and next to the table attach asked for; and the per-step cost of the attach where no leaf qualifies")
    ap.add_argument("--reads", type=int, default=800, help="--selfplay-bench: mcts_num_read")
    ap.add_argument("--endgame-reads", type=int, default=0, help="--selfplay-bench: read cap of the searches the tables serve (0: none)")
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5, help="--selfplay-bench: timed runs per configuration (median)")
    a = ap.parse_args(argv)
    if a.tables_bench > 0:
        a.free = 20 if a.free is None else a.free
        print(json.dumps(_tables_bench(a)))
        return
    if a.tails_bench > 0:
        print(json.dumps(_tails_bench(a)))
        return
    if a.replay_bench > 0:
        print(json.dumps(_replay_bench(a)))
        return
    if a.deep_bench > 0:
        a.free = DEEP_FREE if a.free is None else a.free
        print(json.dumps(_deep_bench(a)))
        return
    a.free = MAX_FREE if a.free is None else a.free
    if a.selfplay_bench > 0:
        a.slots = a.slots or min(a.selfplay_bench, 8192)
        print(json.dumps(_selfplay_bench(a)))
        return
    g = Endgame(a.rows, a.cols, a.device, a.max_free)
    out = dict(rows=a.rows, cols=a.cols, E=g.n_edges, max_free=g.max_free)
    out.update(_targets_bench(g, a.targets_bench) if a.targets_bench > 0 else _bench(g, a.bench, a.free))
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
