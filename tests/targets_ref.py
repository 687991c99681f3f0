"""Exact training targets restated in numpy float32 (helper of test_exact_targets_cpu.py / test_hip_exact_targets.py), written from
the rule in include/dbaz.h (dbaz_exact_targets) on top of endgame_ref.py, not from the kernel.

A row with more than max_free free edges, or of a finished game, stays as it is.  Otherwise v = sign(margin + D[0]),
O = the free edges a with sign(margin + q[a]) == v, z <- v, and pi <- uniform on O, or pi / S on O with S = the float32 sum of pi
over O in ascending a (uniform where S is not > 0); every other slot of pi <- 0."""
import numpy as np

import endgame_ref as ER

PI_MODES = {"keep": 0, "uniform": 1, "restrict": 2}


def margin_of(R, C, x_row):
    """(mover's boxes) - (opponent's boxes) of a feature row, as solver_facts (csrc/solver.h) has it"""
    _, boxes = ER.board(R, C)
    HW, B = (R + 1) * (C + 1), R * C
    x = np.asarray(x_row).ravel()
    closed = sum(all(x[a] != 0 for a in b) for b in boxes)
    mine = (B - int(x[2 * HW])) // 2
    return mine - (closed - mine)


def solve_rows(R, C, x, max_free=16):
    """per row dict(n_free, touched, v, O): touched = the rule applies (unfinished, n_free <= max_free); v and O only then"""
    acts, _ = ER.board(R, C)
    out = []
    for row in np.asarray(x).reshape(len(x), -1):
        F = int(sum(row[a] == 0 for a in acts))
        fact = dict(n_free=F, touched=False, finished=False, v=None, O=[])
        if F <= max_free:
            r = ER.endgame_ref(R, C, row)
            fact["finished"] = r["finished"]
            if not r["finished"]:
                m = margin_of(R, C, row)
                v = int(np.sign(m + r["diff"]))
                assert v == r["value"]
                O = [a for a in acts if r["q"][a] != -128 and int(np.sign(m + int(r["q"][a]))) == v]
                assert O and all(row[a] == 0 for a in O)
                fact.update(touched=True, v=v, O=O)
        out.append(fact)
    return out


def apply_targets(facts, pi, z, pi_mode, z_mode):
    """dict(pi, z, n_free int16, mass float32, relabelled uint8, z_changed) of dbaz_exact_targets on rows whose facts are solve_rows'"""
    pm = PI_MODES[pi_mode] if isinstance(pi_mode, str) else int(pi_mode)
    pi = np.array(pi, dtype=np.float32, copy=True)
    z = np.array(z, dtype=np.float32, copy=True)
    n = len(facts)
    mass, relabelled, z_changed = np.zeros(n, np.float32), np.zeros(n, np.uint8), 0
    for i, f in enumerate(facts):
        if not f["touched"]:
            continue
        relabelled[i] = 1
        S = np.float32(0)
        for a in f["O"]:  # ascending a
            S = np.float32(S + pi[i, a])
        mass[i] = S
        z_changed += int(z[i] != np.float32(f["v"]))
        if z_mode:
            z[i] = np.float32(f["v"])
        if pm:
            new = np.zeros(pi.shape[1], np.float32)
            if pm == 2 and S > 0:
                new[f["O"]] = pi[i, f["O"]] / S  # float32 / float32
            else:
                new[f["O"]] = np.float32(1.0) / np.float32(len(f["O"]))
            pi[i] = new
    return dict(pi=pi, z=z, n_free=np.array([f["n_free"] for f in facts], np.int16), mass=mass, relabelled=relabelled, z_changed=z_changed)


def targets_ref(R, C, x, pi, z, pi_mode="restrict", z_mode=True, max_free=16):
    return apply_targets(solve_rows(R, C, x, max_free), pi, z, pi_mode, z_mode)


def stats_ref(facts, out, max_free=16):
    """the counts dbaz_dataset_exact_targets reports for these rows"""
    by_free = np.zeros(17, np.int64)
    for f in facts:
        if f["touched"]:
            by_free[f["n_free"]] += 1
    return dict(rows=len(facts), relabelled=int(by_free.sum()), finished=sum(f["finished"] and f["n_free"] <= max_free for f in facts),
                z_changed=int(out["z_changed"]), by_free=by_free)


def late_positions(R, C, seed, count=60, max_left=9):
    """the late positions test_endgame_cpu.py builds from uniformly random oracle play: (feature rows int16 [n, 3*H*W], the
    oracle states they were taken from); games are played until at least `count` positions are there, the last one to its end"""
    from oracle import oracle as O
    d = O.dims(R, C)
    E = 2 * R * C + R + C
    rs = np.random.RandomState(seed)
    xs, states = [], []
    while len(xs) < count:
        s = O.new_state(d)
        left = E
        while O.get_result(s) is None:
            if left <= max_left:
                xs.append(np.asarray(O.features(d, s)).ravel().astype(np.int16))
                states.append(s.copy())
            valid = np.nonzero(O.valid_moves(d, s))[0]
            O.play_(d, s, int(valid[rs.randint(len(valid))]))
            left -= 1
    return np.array(xs, np.int16), states
