"""Gumbel root search (Danihelka et al., ICLR 2022, "Policy improvement by planning with Gumbel") at the root of the self-play
driver's searches.

With Engine(gumbel=(m, c_visit, c_scale)) -- params.self_play.gumbel = {"m": 16, "c_visit": 50, "c_scale": 1.0} -- every search
the driver starts samples its candidates by the Gumbel-top-m trick, spends its reads by sequential halving, plays the rule's own
move and records softmax(logits + sigma(completed Q)) as the row's target (visits = round(pi' * 2^24), bit 2 of a row's "pad";
fetch_samples()["gumbel"]).  That target is a policy improvement at any budget, which is what the searches of 16 to 100 reads
need.  The rule is stated in full in include/dbaz.h; its host mirrors (no device):

    considered_visits(m_eff, R)                       the sequence of considered visits (dbaz_gumbel_considered)
    target(c_visit, c_scale, P, W, n, same, valid)    the row's visits of a root (dbaz_gumbel_target)

Engine(gumbel=(m, c_visit, c_scale, True)) -- "full": True in the params -- is the paper's "Full Gumbel": every level below the root
takes argmax pi'(a) - n(a) / (1 + sum n) instead of the UCB's pick, and unvisited children are completed with the full v_mix around
the node's own value v (bit 3 of "pad" beside bit 2; fetch_samples()["gumbel_full"]).  Its host mirrors:

    improved_policy(c_visit, c_scale, v, P, W, n, same, valid)    pi' of a node, float64 [A] (dbaz_gumbel_improved_policy)
    nonroot_pick(c_visit, c_scale, v, P, W, n, same, valid)       the child a simulation takes below the root (dbaz_gumbel_nonroot_pick)
    target(..., v=v)                                              the row's visits with the full v_mix (dbaz_gumbel_target_full)

What the rule does to playing strength per GPU-hour has not been measured here.

    python -m dotsboxesaz_amd.gumbel --rows 6 --cols 6 --bench 8192 --slots 8192 --reads 32,64,100 [--full-prob 0.25 --fast-reads 100]

plays the same game indices with a random-init ResNetZero with PUCT at --puct-reads and with the Gumbel root at each read count,
in one process, and prints one JSON line: per mode games/s, recorded rows/s, network evaluations per game, the mean entropy
(nats) of the recorded pi and the mean max_deepness of the searches.  --full adds the full mode at each read count.

In match play each of the two models has its own search (Engine.match_set_search, dbaz_match_set_search: read budget, PUCT or Gumbel,
the Gumbel constants, root-only or full, and a scale on the Gumbel noise -- 0 is the paper's deterministic evaluation search):

    python -m dotsboxesaz_amd.gumbel --rows 6 --cols 6 --match 8192 --seat0 gumbel:32[:full][:g0] --seat1 puct:800 [--openings 64 --opening-plies 4]

plays N games of one random-init network against itself, seats swapped on odd games, from K random openings of P plies (two
deterministic seats need a book), and prints one JSON line: games/s, evaluations per game, wins / draws / losses of seat 0 and the
Elo difference they imply.  With --rows 3 --cols 3 --vs-solver seat 1 is the solved table and the line carries held_rate.
"""
import ctypes as C

import numpy as np

from . import _lib

DEFAULT = (16, 50.0, 1.0)  # m, c_visit, c_scale


def considered_visits(m_eff, R):
    """int32 [R]: considered(m_eff, R, t) for t = 0 .. R - 1.  ValueError for what dbaz_gumbel_considered refuses."""
    L = _lib.load()
    out = np.zeros(max(int(R), 0), dtype=np.int32)
    if L.dbaz_gumbel_considered(int(m_eff), int(R), out.ctypes.data) != 0:
        raise ValueError("dbaz_gumbel_considered refused its arguments (m_eff = %r, R = %r)" % (m_eff, R))
    return out


def _node_arrays(P, W, n, same, valid):
    P = np.ascontiguousarray(P, dtype=np.float64)
    W = np.ascontiguousarray(W, dtype=np.float32)
    n = np.ascontiguousarray(n, dtype=np.int64)
    A = P.shape[0]
    if not (P.shape == W.shape == n.shape == (A,) == np.shape(same) == np.shape(valid)) or (n < 0).any() or (n > 0x3FFFFFFF).any():
        raise ValueError("P, W, n, same and valid are [A] arrays, n in 0 .. 2^30 - 1")
    ns = (n.astype(np.uint32) | np.where(np.asarray(same, dtype=bool), np.uint32(0x40000000), np.uint32(0))).astype(np.uint32)
    return A, P, W, ns, np.ascontiguousarray(np.asarray(valid, dtype=bool), dtype=np.uint8)


def _node_call(fn, out, c_visit, c_scale, v, P, W, n, same, valid):
    A, P, W, ns, va = _node_arrays(P, W, n, same, valid)
    rc = fn(A, C.c_double(float(c_visit)), C.c_double(float(c_scale)), C.c_double(float(v)), P.ctypes.data, W.ctypes.data, ns.ctypes.data,
            va.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise ValueError("%s refused its arguments (A = %d, c_visit = %r, c_scale = %r, v = %r)" % (fn.__name__, A, c_visit, c_scale, v))
    return out


def improved_policy(c_visit, c_scale, v, P, W, n, same, valid):
    """float64 [A]: pi' = softmax(logit + sigma(completed Q)) over the candidates of a node in the full mode (0.0 elsewhere), the
    completed Q of an unvisited child being the full v_mix around v, the float32 value the node got at its expansion.  The other
    arguments are those of target().  ValueError for what dbaz_gumbel_improved_policy refuses."""
    return _node_call(_lib.load().dbaz_gumbel_improved_policy, np.zeros(len(P), dtype=np.float64), c_visit, c_scale, v, P, W, n, same, valid)


def nonroot_pick(c_visit, c_scale, v, P, W, n, same, valid):
    """int: the child a simulation of the full mode takes at a node below the root, the first maximum over the candidates of
    pi'(a) - n(a) / (1 + sum n); -1 if no child is valid.  ValueError for what dbaz_gumbel_nonroot_pick refuses."""
    return int(_node_call(_lib.load().dbaz_gumbel_nonroot_pick, np.zeros(1, dtype=np.int32), c_visit, c_scale, v, P, W, n, same, valid)[0])


def target(c_visit, c_scale, P, W, n, same, valid, v=None):
    """int32 [A]: the visits a Gumbel row records for a root with float64 priors P, float32 child_total_value W, visit counts n,
    same[i] = child i's player to move is the root's (sgn = +1), valid[i] = child i is a legal move: floor(pi' * 2^24 + 0.5) with
    pi' = softmax(logit + sigma(completed Q)) over the candidates.  v given: the full mode's row (dbaz_gumbel_target_full), with the
    full v_mix around the root's own value v.  ValueError for what dbaz_gumbel_target refuses."""
    L = _lib.load()
    if v is not None:
        return _node_call(L.dbaz_gumbel_target_full, np.zeros(len(P), dtype=np.int32), c_visit, c_scale, v, P, W, n, same, valid)
    P = np.ascontiguousarray(P, dtype=np.float64)
    W = np.ascontiguousarray(W, dtype=np.float32)
    n = np.ascontiguousarray(n, dtype=np.int64)
    A = P.shape[0]
    if not (P.shape == W.shape == n.shape == (A,) == np.shape(same) == np.shape(valid)) or (n < 0).any() or (n > 0x3FFFFFFF).any():
        raise ValueError("P, W, n, same and valid are [A] arrays, n in 0 .. 2^30 - 1")
    ns = (n.astype(np.uint32) | np.where(np.asarray(same, dtype=bool), np.uint32(0x40000000), np.uint32(0))).astype(np.uint32)
    v = np.ascontiguousarray(np.asarray(valid, dtype=bool), dtype=np.uint8)
    out = np.zeros(A, dtype=np.int32)
    rc = L.dbaz_gumbel_target(A, C.c_double(float(c_visit)), C.c_double(float(c_scale)), P.ctypes.data, W.ctypes.data, ns.ctypes.data,
                              v.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise ValueError("dbaz_gumbel_target refused its arguments (A = %d, c_visit = %r, c_scale = %r)" % (A, c_visit, c_scale))
    return out


def _entropy(pi):
    """mean over the rows of -sum pi log pi (nats)"""
    p = np.asarray(pi, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log(p), 0.0)
    return float(-t.sum(axis=1).mean()) if len(p) else 0.0


def _bench(a):
    import sys
    import time
    import torch
    from . import nn as dnn
    from .engine import Engine

    cap = (a.full_prob, a.fast_reads) if a.full_prob < 1.0 else None

    def play(name, reads, gumbel):
        eng = Engine(a.rows, a.cols, a.slots, mcts_num_read=reads, noise=(0.8, 0.25), reuse_tree=True, evaluator="resnet", seed=1000,
                     device=a.device, playout_cap=cap, gumbel=gumbel)
        torch.manual_seed(0)
        model = dnn.ResNetZero(dnn.resnet_params(a.rows, a.cols, a.channels, a.blocks))
        eng.load_state_dict(model.state_dict(), "resnet", **model.shape)
        runs = []
        for i in range(a.repeats + 1):
            n_games = a.bench if i else min(a.bench, a.warmup_games)  # the first run warms up, on few games
            eng.sync()
            t0 = time.perf_counter()
            eng.selfplay_start(n_games, 0)
            eng.run()
            dt = time.perf_counter() - t0  # the games; the rows are fetched outside (a generation keeps them on the device)
            got = eng.fetch_samples()
            c, gm = eng.counters(), eng.gumbel()
            full = got["full"] if "full" in got else np.ones(len(got["z"]), bool)
            print("gumbel bench: %s run %d of %d, %d games, %.1f s" % (name, i, a.repeats, n_games, dt), file=sys.stderr, flush=True)
            if i:
                games = max(1, c["games_finished"])
                runs.append(dict(games_per_s=c["games_finished"] / dt, recorded_rows_per_s=int(full.sum()) / dt,
                                 nn_evals_per_game=c["nn_evals"] / games, gumbel_rows=gm["rows"], steps=c["steps"],
                                 pi_entropy=_entropy(got["pi"][full]), mean_max_deepness=float(np.mean(got["max_deepness"])),
                                 pool_resets=c["pool_resets"], seconds=dt))
        eng.close()
        return {k: float(np.median([r[k] for r in runs])) for k in runs[0]}

    out = dict(rows=a.rows, cols=a.cols, games=a.bench, slots=a.slots, m=a.m, c_visit=a.c_visit, c_scale=a.c_scale, full_prob=a.full_prob,
               fast_reads=a.fast_reads, puct_reads=a.puct_reads)
    if a.puct_reads > 0:
        out["puct"] = play("puct %d" % a.puct_reads, a.puct_reads, None)
    for r in a.reads:
        out["gumbel_%d" % r] = play("gumbel %d" % r, r, (a.m, a.c_visit, a.c_scale))
        if a.full:
            out["gumbel_full_%d" % r] = play("gumbel full %d" % r, r, (a.m, a.c_visit, a.c_scale, True))
    return out


def parse_seat(text, m=DEFAULT[0], c_visit=DEFAULT[1], c_scale=DEFAULT[2]):
    """"puct:800", "gumbel:32", "gumbel:32:full", "gumbel:32:g0", "gumbel:32:full:g0" -> a spec of Engine(match_search=)"""
    parts = str(text).split(":")
    if len(parts) < 2 or parts[0] not in ("puct", "gumbel") or not parts[1].isdigit() or int(parts[1]) < 1:
        raise ValueError("seat %r: puct:READS or gumbel:READS[:full][:g0]" % (text,))
    opts = parts[2:]
    if parts[0] == "puct":
        if opts:
            raise ValueError("seat %r: a PUCT seat takes no option" % (text,))
        return dict(reads=int(parts[1]))
    if any(o not in ("full", "g0") for o in opts):
        raise ValueError("seat %r: the options of a Gumbel seat are full and g0" % (text,))
    return dict(reads=int(parts[1]), gumbel=(int(m), float(c_visit), float(c_scale), "full" in opts, 0.0 if "g0" in opts else 1.0))


def random_openings(rows, cols, n, plies, seed=0):
    """n legal unfinished openings of `plies` random moves each (move sequences), by the rules of dotsboxesaz_amd.game"""
    from .game import BoxesState
    saved = BoxesState.BOARD_DIM
    BoxesState.init_static_fields(((rows, cols),))
    try:
        rs = np.random.RandomState(seed)
        book = []
        while len(book) < n:
            st, moves = BoxesState(), []
            for _ in range(plies):
                valid = np.asarray(st.get_valid_moves(as_indices=True))
                if st.get_result() is not None or len(valid) == 0:
                    break
                mv = int(valid[rs.randint(len(valid))])
                st.play_(mv)
                moves.append(mv)
            if len(moves) == plies and st.get_result() is None:
                book.append(moves)
    finally:
        BoxesState.init_static_fields((saved,))
    return book


def elo_difference(wins, draws, losses):
    """the Elo difference a score implies: -400 log10(1 / s - 1) with s = (wins + draws / 2) / games (+-inf at s = 1, 0)"""
    n = wins + draws + losses
    s = (wins + 0.5 * draws) / n if n else 0.5
    if s <= 0.0 or s >= 1.0:
        return float("inf") if s >= 1.0 else float("-inf")
    return float(-400.0 * np.log10(1.0 / s - 1.0))


def _match(a):
    import time
    import torch
    from . import nn as dnn
    from . import self_play as sp
    from .engine import Engine

    seats = (parse_seat(a.seat0, a.m, a.c_visit, a.c_scale), None if a.vs_solver else parse_seat(a.seat1, a.m, a.c_visit, a.c_scale))
    reads = max(s["reads"] for s in seats if s)
    solver = eng = None
    try:
        if a.vs_solver:
            from .solver import Solver
            solver = Solver(a.rows, a.cols, a.device).solve()
            kw = dict(evaluator2="solver", solver=solver, solver_reads=a.solver_reads)
        else:
            kw = dict(evaluator2=a.evaluator)
        eng = Engine(a.rows, a.cols, a.slots, mcts_num_read=reads, noise=(0.0, 0.0), reuse_tree=False, evaluator=a.evaluator, seed=1000,
                     device=a.device, match_play=True, match_search=seats, **kw)
        if a.evaluator == "resnet":
            torch.manual_seed(0)
            model = dnn.ResNetZero(dnn.resnet_params(a.rows, a.cols, a.channels, a.blocks))
            for i in range(1 if a.vs_solver else 2):
                eng.load_state_dict(model.state_dict(), "resnet", model=i, **model.shape)
        if a.openings > 0:
            eng.selfplay_set_start(random_openings(a.rows, a.cols, a.openings, a.opening_plies), 2)
        eng.sync()
        t0 = time.perf_counter()
        eng.selfplay_start(a.match, 0)
        eng.run()
        dt = time.perf_counter() - t0
        got = eng.fetch_samples()
        c, gm = eng.counters(), eng.gumbel()
        first = np.nonzero(got["move_idx"] == 0)[0]
        z0 = got["z"][first].astype(np.int64) * np.where((got["player"][first] ^ (got["game_idx"][first] & 1)) == 0, 1, -1)  # seat 0's result
        w, dr, l = int((z0 > 0).sum()), int((z0 == 0).sum()), int((z0 < 0).sum())
        games = max(1, c["games_finished"])
        out = dict(rows=a.rows, cols=a.cols, games=int(c["games_finished"]), slots=a.slots, evaluator=a.evaluator, seat0=a.seat0,
                   seat1="solver" if a.vs_solver else a.seat1, openings=a.openings, opening_plies=a.opening_plies, games_per_s=c["games_finished"] / dt,
                   evals_per_game=(c["nn_evals"] if a.evaluator == "resnet" else c["expansions"]) / games, gumbel_rows=gm["rows"],
                   wins=w, draws=dr, losses=l, elo_diff=elo_difference(w, dr, l), seconds=dt)
        if solver is not None:
            out["held_rate"] = sp.match_vs_theory(got, solver)["held_rate"]
        return out
    finally:
        if eng is not None:
            eng.close()
        if solver is not None:
            solver.close()


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(description="self-play with PUCT and with the Gumbel root search at several read counts; prints one JSON line")
    ap.add_argument("--rows", type=int, default=6)
    ap.add_argument("--cols", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bench", type=int, default=8192, metavar="N", help="games per timed run (game indices 0 .. N-1, in every mode)")
    ap.add_argument("--slots", type=int, default=0, help="engine slots (default min(N, 8192))")
    ap.add_argument("--reads", type=lambda s: [int(x) for x in s.split(",") if x], default=[32, 64, 100], help="mcts_num_read of the Gumbel runs")
    ap.add_argument("--puct-reads", type=int, default=800, help="mcts_num_read of the PUCT run (0: none)")
    ap.add_argument("--m", type=int, default=DEFAULT[0], help="candidates sampled without replacement")
    ap.add_argument("--c-visit", type=float, default=DEFAULT[1])
    ap.add_argument("--c-scale", type=float, default=DEFAULT[2])
    ap.add_argument("--full", action="store_true", help="also play the full mode (the rule below the root too) at each read count")
    ap.add_argument("--full-prob", type=float, default=1.0, help="playout cap: share of full searches (1 = no cap)")
    ap.add_argument("--fast-reads", type=int, default=100)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=1, help="timed runs per mode (median)")
    ap.add_argument("--warmup-games", type=int, default=64, help="games of the one untimed run in front of them")
    ap.add_argument("--match", type=int, default=0, metavar="N", help="match play instead of the bench: N games of one network against itself")
    ap.add_argument("--seat0", default="gumbel:32", help="model 0's search: puct:READS or gumbel:READS[:full][:g0]")
    ap.add_argument("--seat1", default="puct:800", help="model 1's search")
    ap.add_argument("--openings", type=int, default=0, metavar="K", help="a book of K random openings, two games each per round (0: the empty board)")
    ap.add_argument("--opening-plies", type=int, default=4, metavar="P")
    ap.add_argument("--vs-solver", action="store_true", help="seat 1 is the solved table of the board (small boards); adds held_rate")
    ap.add_argument("--solver-reads", type=int, default=2)
    ap.add_argument("--evaluator", default="resnet", choices=("resnet", "formula", "uniform"), help="the network (random-init) or a formula evaluator")
    a = ap.parse_args(argv)
    if a.match > 0:
        a.slots = a.slots or max(1, min(a.match, 8192))
        print(json.dumps(_match(a)))
        return
    a.slots = a.slots or max(1, min(a.bench, 8192))
    print(json.dumps(_bench(a)))


if __name__ == "__main__":
    main()
