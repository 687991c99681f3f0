"""Forced playouts and policy target pruning (Wu 2019, "Accelerating Self-Play Learning in Go", section 3.2) at the root of the
self-play driver's full searches.

With Engine(forced_playouts=(k, prune)) -- params.self_play.forced_playouts = {"k": 2.0, "prune": True} -- every visited root
child of a full search gets at least sqrt(k P N) playouts, and with prune the recorded visits lose those again wherever PUCT on
its own would not have spent them (bit 1 of a row's "pad"; fetch_samples()["pruned"]).  Exploration stays in the tree and out of
the target; the game, q_value and TreeStats are untouched by the pruning.  The rule is stated in full in include/dbaz.h:

    prune_visits(k, pbc, sq, root_N, P, W, n, same, valid)      its second half on the host (dbaz_prune_visits: no device)

What the pair does to playing strength per GPU-hour has not been measured here.

    python -m dotsboxesaz_amd.forced_playouts --rows 6 --cols 6 --bench 8192 --slots 8192 [--full-prob 0.25 --fast-reads 100] --k 2

plays the same game indices with a random-init ResNetZero with the rule off, forcing only, and forcing plus pruning, in one
process, and prints one JSON line: per mode games/s, recorded rows/s, network evaluations per game, rows pruned, mean visits
pruned per row and the mean entropy (nats) of the recorded pi.
"""
import ctypes as C

import numpy as np

from . import _lib


def prune_visits(k, pbc, sq, root_N, P, W, n, same, valid):
    """int32 [A]: the visits a row records for a root with float64 priors P, float32 child_total_value W, visit counts n,
    same[i] = child i's player to move is the root's (sgn = +1), valid[i] = child i is a legal move; pbc = log((N + base + 1) /
    base) + cpuct and sq = sqrt(N) at the root's visit count N = root_N.  k = 0 gives n back.  ValueError for what
    dbaz_prune_visits refuses."""
    L = _lib.load()
    P = np.ascontiguousarray(P, dtype=np.float64)
    W = np.ascontiguousarray(W, dtype=np.float32)
    n = np.ascontiguousarray(n, dtype=np.int64)
    A = P.shape[0]
    if not (P.shape == W.shape == n.shape == (A,) == np.shape(same) == np.shape(valid)) or (n < 0).any() or (n > 0x3FFFFFFF).any():
        raise ValueError("P, W, n, same and valid are [A] arrays, n in 0 .. 2^30 - 1")
    ns = (n.astype(np.uint32) | np.where(np.asarray(same, dtype=bool), np.uint32(0x40000000), np.uint32(0))).astype(np.uint32)
    v = np.ascontiguousarray(np.asarray(valid, dtype=bool), dtype=np.uint8)
    out = np.zeros(A, dtype=np.int32)
    rc = L.dbaz_prune_visits(A, C.c_double(float(k)), C.c_double(float(pbc)), C.c_double(float(sq)), int(root_N), P.ctypes.data,
                             W.ctypes.data, ns.ctypes.data, v.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise ValueError("dbaz_prune_visits refused its arguments (A = %d, k = %r, root_N = %r)" % (A, k, root_N))
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

    def play(name, forced):
        eng = Engine(a.rows, a.cols, a.slots, mcts_num_read=a.reads, noise=(0.8, 0.25), reuse_tree=True, evaluator="resnet", seed=1000,
                     device=a.device, playout_cap=cap, forced_playouts=forced)
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
            c, fp = eng.counters(), eng.forced_playouts()
            full = got["full"] if "full" in got else np.ones(len(got["z"]), bool)
            print("forced-playouts bench: %s run %d of %d, %d games, %.1f s" % (name, i, a.repeats, n_games, dt), file=sys.stderr, flush=True)
            if i:
                games = max(1, c["games_finished"])
                runs.append(dict(games_per_s=c["games_finished"] / dt, recorded_rows_per_s=int(full.sum()) / dt,
                                 nn_evals_per_game=c["nn_evals"] / games, rows_pruned=fp["rows_pruned"],
                                 visits_pruned_per_row=fp["visits_pruned"] / max(1, fp["rows_pruned"]),
                                 pi_entropy=_entropy(got["pi"][full]), pool_resets=c["pool_resets"], seconds=dt))
        eng.close()
        return {k: float(np.median([r[k] for r in runs])) for k in runs[0]}

    out = dict(rows=a.rows, cols=a.cols, games=a.bench, slots=a.slots, reads=a.reads, k=a.k, full_prob=a.full_prob, fast_reads=a.fast_reads,
               off=play("off", None), forced=play("forced", (a.k, False)), pruned=play("pruned", (a.k, True)))
    for m in ("forced", "pruned"):
        out[m + "_games_ratio"] = out[m]["games_per_s"] / out["off"]["games_per_s"]
    return out


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(description="self-play with forced playouts off, on, and on with policy target pruning; prints one JSON line")
    ap.add_argument("--rows", type=int, default=6)
    ap.add_argument("--cols", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bench", type=int, default=8192, metavar="N", help="games per timed run (game indices 0 .. N-1, in every mode)")
    ap.add_argument("--slots", type=int, default=0, help="engine slots (default min(N, 8192))")
    ap.add_argument("--k", type=float, default=2.0, help="a visited root child gets at least sqrt(k P N) playouts")
    ap.add_argument("--full-prob", type=float, default=1.0, help="playout cap: share of full searches (1 = no cap)")
    ap.add_argument("--fast-reads", type=int, default=100)
    ap.add_argument("--reads", type=int, default=800, help="mcts_num_read")
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=1, help="timed runs per mode (median)")
    ap.add_argument("--warmup-games", type=int, default=64, help="games of the one untimed run in front of them")
    a = ap.parse_args(argv)
    a.slots = a.slots or max(1, min(a.bench, 8192))
    print(json.dumps(_bench(a)))


if __name__ == "__main__":
    main()
