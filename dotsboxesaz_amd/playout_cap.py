"""Playout cap randomization (Wu 2019, "Accelerating Self-Play Learning in Go", section 3.1): which self-play searches are full.

With Engine(playout_cap=(full_prob, fast_reads)) -- params.self_play.playout_cap = {"full_prob": p, "fast_reads": n} -- a random
share full_prob of the searches the self-play driver starts are the ordinary ones (the driver rule's reads, root noise, a row
that trains); every other one runs min(driver rule, fast_reads) reads without noise, only moves its game on, and marks its row
(bit 0 of "pad").  The decision is a pure function of (seed, absolute game index, ply), stated in full in include/dbaz.h:

    is_full(seed, game_idx, ply, full_prob)      the rule on the host (dbaz_playout_cap_is_full: no device), numpy-vectorised

What the trade buys in playing strength per GPU-hour has not been measured here.

    python -m dotsboxesaz_amd.playout_cap --rows 6 --cols 6 --bench 8192 --slots 8192 --full-prob 0.25 --fast-reads 100

plays the same game indices with a random-init ResNetZero once without and once with the cap and prints one JSON line: games/s,
recorded (full) rows/s, network evaluations per game, full and fast searches, pool_resets.
"""
import ctypes as C

import numpy as np

from . import _lib


def is_full(seed, game_idx, ply, full_prob):
    """bool array (the broadcast shape of game_idx and ply; a bool for scalars): the search of game `game_idx` at ply `ply` under
    `seed` is a full one.  full_prob >= 1 (no cap): all True.  ValueError for full_prob NaN or outside [0, 1]."""
    L = _lib.load()
    full_prob = float(full_prob)
    if not 0.0 <= full_prob <= 1.0:
        raise ValueError("full_prob = %r is outside [0, 1]" % (full_prob,))
    g, p = np.broadcast_arrays(np.asarray(game_idx, dtype=np.int64), np.asarray(ply, dtype=np.int64))
    out = np.empty(g.shape, dtype=bool)
    fn, s, fp = L.dbaz_playout_cap_is_full, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_double(full_prob)
    flat = out.reshape(-1)
    for i, (gi, pi) in enumerate(zip(g.reshape(-1).tolist(), p.reshape(-1).tolist())):
        flat[i] = fn(s, gi, pi, fp) == 1
    return out if out.ndim else bool(out)


def _bench(a):
    import sys
    import time
    import torch
    from . import nn as dnn
    from .engine import Engine

    def play(cap):
        eng = Engine(a.rows, a.cols, a.slots, mcts_num_read=a.reads, noise=(0.8, 0.25), reuse_tree=True, evaluator="resnet", seed=1000,
                     device=a.device, playout_cap=cap)
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
            c, pc = eng.counters(), eng.playout_cap()
            n_full = int(got["full"].sum()) if "full" in got else len(got["z"])
            print("playout-cap bench: cap %s run %d of %d, %d games, %.1f s" % (cap, i, a.repeats, n_games, dt), file=sys.stderr, flush=True)
            if i:
                games = max(1, c["games_finished"])
                runs.append(dict(games_per_s=c["games_finished"] / dt, recorded_rows_per_s=n_full / dt, rows_per_s=len(got["z"]) / dt,
                                 nn_evals_per_game=c["nn_evals"] / games, reads_per_move=c["expansions"] / max(1, c["moves_played"]),
                                 full_searches=pc["full_searches"], fast_searches=pc["fast_searches"], pool_resets=c["pool_resets"],
                                 seconds=dt))
        eng.close()
        return {k: float(np.median([r[k] for r in runs])) for k in runs[0]}

    out = dict(rows=a.rows, cols=a.cols, games=a.bench, slots=a.slots, reads=a.reads, full_prob=a.full_prob, fast_reads=a.fast_reads,
               off=play(None), on=play((a.full_prob, a.fast_reads)))
    out["games_speedup"] = out["on"]["games_per_s"] / out["off"]["games_per_s"]
    out["recorded_rows_ratio"] = out["on"]["recorded_rows_per_s"] / out["off"]["recorded_rows_per_s"]
    # what the mean read budget alone would give if every move ran mcts_num_read reads (the driver rule and the endgame make it less)
    out["derived_speedup"] = a.reads / (a.full_prob * a.reads + (1.0 - a.full_prob) * min(a.reads, a.fast_reads))
    return out


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(description="self-play throughput with and without playout cap randomization; prints one JSON line")
    ap.add_argument("--rows", type=int, default=6)
    ap.add_argument("--cols", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bench", type=int, default=8192, metavar="N", help="games per timed run (game indices 0 .. N-1, both ways)")
    ap.add_argument("--slots", type=int, default=0, help="engine slots (default min(N, 8192))")
    ap.add_argument("--full-prob", type=float, default=0.25)
    ap.add_argument("--fast-reads", type=int, default=100)
    ap.add_argument("--reads", type=int, default=800, help="mcts_num_read")
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=1, help="timed runs per configuration (median)")
    ap.add_argument("--warmup-games", type=int, default=64, help="games of the one untimed run in front of them")
    a = ap.parse_args(argv)
    a.slots = a.slots or max(1, min(a.bench, 8192))
    print(json.dumps(_bench(a)))


if __name__ == "__main__":
    main()
