"""Exact solver for small boards (E <= 31 edges): true values and optimal moves from a table solved on the GPU.

    python -m dotsboxesaz_amd.solver --rows 3 --cols 3

The table int8 D[2^E] lives in HBM (csrc/solver.hip): D[mask] is the best achievable score difference over
the boxes still open for the player to move.  Bit i of a mask is the i-th real edge in ascending order of its action index.
"""
import ctypes as C

import numpy as np

from . import _lib

ILLEGAL = -128  # q of a drawn edge or a sentinel slot


def edge_actions(rows, cols):
    """Action index of every real edge, ascending: position i is compact edge i (bit i of a mask)."""
    H, W = rows + 1, cols + 1
    return np.array(sorted([l * W + c for l in range(H) for c in range(cols)] + [H * W + l * W + c for l in range(rows) for c in range(W)]),
                    dtype=np.int64)


class Solver:
    """Solved table of one board size on one GPU.  E > 31 raises DbazError before the device is touched."""

    def __init__(self, rows, cols, device=0):
        self._L = _lib.load()
        self.rows, self.cols, self.device = int(rows), int(cols), int(device)
        self.H, self.W = self.rows + 1, self.cols + 1
        self.A, self.F = 2 * self.H * self.W, 3 * self.H * self.W
        self.h = C.c_void_p()
        rc = self._L.dbaz_solver_create(self.rows, self.cols, self.device, C.byref(self.h))
        if rc != _lib.OK:
            self.h = None
            self._raise(rc)
        self.n_edges = self.info()["n_edges"]
        self.actions = edge_actions(self.rows, self.cols)
        self._bit = np.full(self.A, -1, np.int64)  # action -> compact edge
        self._bit[self.actions] = np.arange(self.n_edges)

    def _raise(self, rc):
        msg = self._L.dbaz_solver_last_error(self.h)
        raise _lib.DbazError(rc, msg.decode() if msg else "error %d" % rc)

    def _ck(self, rc):
        if rc != _lib.OK:
            self._raise(rc)

    def close(self):
        if getattr(self, "h", None):
            self._L.dbaz_solver_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, low_bits=0):
        """Runs the retrograde analysis and returns when the table is complete.  low_bits: 0 = default, L = size of the LDS
        subcube, -1 = the plain one-launch-per-layer kernel (same bytes either way)."""
        self._ck(self._L.dbaz_solver_solve(self.h, int(low_bits)))
        return self

    def info(self):
        e, b, ms, d0 = C.c_int32(), C.c_int64(), C.c_double(), C.c_int32()
        self._ck(self._L.dbaz_solver_info(self.h, C.byref(e), C.byref(b), C.byref(ms), C.byref(d0)))
        return dict(n_edges=e.value, table_bytes=b.value, solve_ms=ms.value, d0=d0.value)

    def table(self, first=0, count=None):
        """Host copy of D[first : first + count] (default: the whole table) as a numpy int8 array."""
        count = (1 << self.n_edges) - first if count is None else count
        out = np.empty(max(int(count), 0), np.int8)
        self._ck(self._L.dbaz_solver_table(self.h, C.c_void_p(out.ctypes.data), C.c_int64(first), C.c_int64(count)))
        return out

    def mask_of(self, moves_or_state):
        """Mask of a position given as a sequence of action indices, as a feature array ([3, H, W] or flat), or as a state
        object with a `board` of the A action slots (nonzero = drawn; sentinel slots are ignored)."""
        board = getattr(moves_or_state, "board", None)
        if board is not None:
            drawn = np.frombuffer(bytes(board), np.uint8)[:self.A] if isinstance(board, (bytes, bytearray, C.Array)) else np.asarray(board).ravel()[:self.A]
            return int(sum(1 << i for i, a in enumerate(self.actions) if drawn[a] != 0))
        arr = np.asarray(moves_or_state)
        if arr.size == self.F and arr.ndim in (1, 3):  # a move list has at most E < 3*H*W entries
            flat = arr.ravel()
            return int(sum(1 << i for i, a in enumerate(self.actions) if flat[a] != 0))
        mask = 0
        for a in arr.ravel().tolist():
            if not 0 <= a < self.A or self._bit[a] < 0:
                raise ValueError("action %d is not an edge of a %dx%d board" % (a, self.rows, self.cols))
            mask |= 1 << int(self._bit[a])
        return mask

    def score(self, x, pi=None):
        """x: feature rows int16 [n, 3*H*W] (or [n, 3, H, W]); pi: optional float32 [n, A].  numpy arrays or torch tensors on
        the solver's device; the outputs come back as the same kind.  Returns dict(value int8 [n], diff int8 [n],
        q int8 [n, A], policy_mass float32 [n] or None)."""
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
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)  # noqa: E731
        with torch.cuda.device(dev):  # queued on torch's current stream, like Engine.dataset_batch
            self._ck(self._L.dbaz_solver_score(self.h, C.c_int32(n), ptr(xt), ptr(pt), ptr(value), ptr(diff), ptr(q), ptr(mass),
                                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        out = dict(value=value, diff=diff, q=q, policy_mass=mass)
        if as_numpy:
            out = {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}
        return out


    def policy(self, x, seed=0):
        """The table as an evaluator: x as in score() -> (p float32 [n, A], v float32 [n]).  p is one-hot on an optimal move (all
        zero for a finished game), v the true result for the mover.  seed = 0 picks the optimal move with the lowest action
        index, any other seed one that is a fixed function of position and seed (include/dbaz.h, dbaz_perfect_policy)."""
        import torch
        dev = torch.device("cuda", self.device)
        as_numpy = not isinstance(x, torch.Tensor)
        xt = torch.as_tensor(np.ascontiguousarray(x, dtype=np.int16) if as_numpy else x).to(device=dev, dtype=torch.int16).reshape(-1, self.F).contiguous()
        n = int(xt.shape[0])
        p = torch.empty((n, self.A), dtype=torch.float32, device=dev)
        v = torch.empty(n, dtype=torch.float32, device=dev)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t.numel() else None)  # noqa: E731
        with torch.cuda.device(dev):
            self._ck(self._L.dbaz_perfect_policy(self.h, C.c_int32(n), ptr(xt), C.c_uint64(int(seed)), ptr(p), ptr(v),
                                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return (p.cpu().numpy(), v.cpu().numpy()) if as_numpy else (p, v)


def score_samples(samples, solver=None, rows=None, cols=None, device=0):
    """Scores the rows Engine.fetch_samples() / generate_games return (x, pi, played, z) against the solved table.
    Per row: value (true result for the mover), policy_mass (search policy on result-preserving moves), played_optimal (the
    move played keeps the result; False for rows without one).  Means: optimal_policy_mass, played_optimal_rate (both over the
    rows of unfinished positions), z_agreement (share of rows whose game outcome z equals the true value).
    solver: a solved Solver of the rows' board size (reuse it: a solve costs a table of 2^E bytes).  Without one the board
    size comes from rows / cols, or from x's shape [n, 3, H, W]; flat rows [n, 3*H*W] alone do not tell it."""
    x = np.asarray(samples["x"])
    if solver is None:
        if rows is None or cols is None:
            if x.ndim != 4:
                raise ValueError("flat feature rows do not tell the board size: pass rows= and cols=, or solver=Solver(rows, cols).solve()")
            rows, cols = x.shape[2] - 1, x.shape[3] - 1
        solver = Solver(rows, cols, device).solve()
    n = len(x)
    pi = np.asarray(samples["pi"], dtype=np.float32).reshape(n, solver.A)
    r = solver.score(x.reshape(n, solver.F), pi)
    played = np.asarray(samples["played"]).astype(np.int64).reshape(n)
    has_move = (played >= 0) & (played < solver.A)
    q_played = np.where(has_move, r["q"][np.arange(n), np.clip(played, 0, solver.A - 1)], ILLEGAL).astype(np.int64)
    open_ = (r["q"] != ILLEGAL).any(axis=1)  # not a finished game
    margin = _margin(solver, x.reshape(n, solver.F))
    played_optimal = has_move & (q_played != ILLEGAL) & (np.sign(margin + q_played) == r["value"])
    z = np.asarray(samples["z"]).reshape(n)
    k = max(int(open_.sum()), 1)
    return dict(value=r["value"], policy_mass=r["policy_mass"], played_optimal=played_optimal,
                optimal_policy_mass=float(r["policy_mass"][open_].astype(np.float64).sum() / k),
                played_optimal_rate=float(played_optimal[open_].sum() / k),
                z_agreement=float((z == r["value"]).mean()) if n else 0.0)


def _margin(solver, x):
    """(mover's boxes) - (opponent's boxes) of feature rows [n, 3*H*W], as the scoring kernel derives it."""
    H, W, HW = solver.H, solver.W, solver.H * solver.W
    e = x[:, :2 * HW] != 0
    closed = np.zeros(len(x), np.int64)
    for l in range(solver.rows):
        for c in range(solver.cols):
            closed += e[:, l * W + c] & e[:, (l + 1) * W + c] & e[:, HW + l * W + c] & e[:, HW + l * W + c + 1]
    mine = (solver.rows * solver.cols - x[:, 2 * HW].astype(np.int64)) // 2
    return 2 * mine - closed


def _random_rows(solver, n, seed=0):
    """n feature rows int16 [n, 3*H*W]: every edge drawn with a per-row probability, boxes shared out so that the row is a
    position of an unfinished game wherever one exists with those edges."""
    rs = np.random.RandomState(seed)
    H, W, HW = solver.H, solver.W, solver.H * solver.W
    x = np.zeros((n, solver.F), np.int16)
    drawn = rs.rand(n, solver.n_edges) < rs.rand(n, 1)
    x[:, solver.actions] = drawn
    x[:, [a for a in range(solver.A) if a not in set(solver.actions.tolist())]] = 1  # sentinel slots, as get_features has them
    e = x[:, :2 * HW] != 0
    closed = np.zeros(n, np.int64)
    for l in range(solver.rows):
        for c in range(solver.cols):
            closed += e[:, l * W + c] & e[:, (l + 1) * W + c] & e[:, HW + l * W + c] & e[:, HW + l * W + c + 1]
    mine = closed // 2
    x[:, 2 * HW:] = (solver.rows * solver.cols - 2 * mine)[:, None]
    return x


def _policy_bench(solver, n):
    """HIP-event milliseconds of one dbaz_perfect_policy and one dbaz_solver_score call on the same n rows: median of 5 after a warm-up"""
    import torch
    dev = torch.device("cuda", solver.device)
    x = torch.as_tensor(_random_rows(solver, n)).to(dev)
    p = torch.empty((n, solver.A), dtype=torch.float32, device=dev)
    v = torch.empty(n, dtype=torch.float32, device=dev)
    value, diff = torch.empty(n, dtype=torch.int8, device=dev), torch.empty(n, dtype=torch.int8, device=dev)
    q = torch.empty((n, solver.A), dtype=torch.int8, device=dev)
    L, ptr = solver._L, lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def timed(call):  # the output buffers exist: the events enclose the kernel alone
        ms = []
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for i in range(6):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                solver._ck(call(stream))
                t1.record()
                t1.synchronize()
                if i:  # the first run warms up
                    ms.append(t0.elapsed_time(t1))
        return round(float(np.median(ms)), 4)

    policy_ms = timed(lambda st: L.dbaz_perfect_policy(solver.h, C.c_int32(n), ptr(x), C.c_uint64(0), ptr(p), ptr(v), st))
    score_ms = timed(lambda st: L.dbaz_solver_score(solver.h, C.c_int32(n), ptr(x), None, ptr(value), ptr(diff), ptr(q), None, st))
    return dict(policy_bench_rows=int(n), policy_ms=policy_ms, score_ms=score_ms)


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(description="solve a small board on the GPU and print one JSON line")
    ap.add_argument("--rows", type=int, default=3)
    ap.add_argument("--cols", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--low-bits", type=int, default=0, help="0 = default, L = LDS subcube of 2^L masks, -1 = plain kernel")
    ap.add_argument("--policy-bench", type=int, default=0, metavar="N",
                    help="HIP-event time of dbaz_perfect_policy and dbaz_solver_score on the same N random positions (median of 5)")
    a = ap.parse_args(argv)
    s = Solver(a.rows, a.cols, a.device).solve(a.low_bits)
    x0 = np.zeros((1, 3, s.H, s.W), np.int16)
    x0[:, 2] = a.rows * a.cols
    q = s.score(x0)["q"][0]
    i = s.info()
    out = dict(rows=a.rows, cols=a.cols, E=i["n_edges"], table_bytes=i["table_bytes"], solve_ms=round(i["solve_ms"], 3),
               d0=i["d0"], first_move_q={int(act): int(q[act]) for act in s.actions})
    if a.policy_bench > 0:
        out.update(_policy_bench(s, a.policy_bench))
    print(json.dumps(out))
    s.close()


if __name__ == "__main__":
    main()
