"""Exact targets on packed replay rows restated in numpy (helper of test_replay_targets_cpu.py / test_hip_replay_targets.py), written
from the rule in include/dbaz.h (dbaz_replay_exact_targets), not from the kernels.  Integers only.

A game is the rows of one game_idx; its root is its first row by move_idx with at most max_free free real edges.  The root and the
rows after it are candidates.  A candidate whose free edges are no subset of the root's is `unserved`, one whose game is over is
`finished`; every other candidate is relabelled: z <- v, and the visits outside O <- 0 ("restrict"; 1 on O where the visits on O
sum to 0) or 1 on O and 0 elsewhere ("uniform").  v, O and finished are the facts of endgame_ref.py / targets_ref.py
(targets_ref.solve_rows' dicts); where they come from is the caller's business: `facts_for(root_x, rows_x)` returns them for the
rows a root serves."""
import numpy as np

import endgame_ref as ER
from dotsboxesaz_amd.self_play import ROW_META, row_bytes

PI_MODES = {"keep": 0, "uniform": 1, "restrict": 2}
STATS = ("rows", "games", "roots", "chunks", "relabelled", "finished", "unserved", "z_changed")


def fields(R, C, packed):
    """(meta view, x int16 [n, 3HW] view, visits int32 [n, A] copy) of packed rows uint8 [n, row_bytes]"""
    HW = (R + 1) * (C + 1)
    F, A = 3 * HW, 2 * HW
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    n = len(packed)
    assert packed.shape == (n, row_bytes(F, A))
    m0 = ROW_META.itemsize
    meta = np.ascontiguousarray(packed[:, :m0]).view(ROW_META).reshape(n)
    x = np.ascontiguousarray(packed[:, m0:m0 + 2 * F]).view("<i2").reshape(n, F)
    vis = np.ascontiguousarray(packed[:, m0 + 2 * F:m0 + 2 * F + 4 * A]).view("<i4").reshape(n, A)
    return meta, x, vis


def pack(R, C, game_idx, move_idx, x, visits, z, seed=0):
    """packed rows from their fields; every other meta field and the padding get arbitrary bytes, which must survive the call"""
    HW = (R + 1) * (C + 1)
    F, A = 3 * HW, 2 * HW
    n = len(x)
    rs = np.random.RandomState(seed)
    out = rs.randint(0, 256, (n, row_bytes(F, A))).astype(np.uint8)
    meta = np.zeros(n, ROW_META)
    for k in ("move", "played", "max_deepness", "tree_size", "terminal_count", "player", "pad"):
        meta[k] = rs.randint(0, 100, n)
    meta["q_value"] = rs.rand(n).astype(np.float32)
    meta["game_idx"], meta["move_idx"], meta["z"] = game_idx, move_idx, z
    m0 = ROW_META.itemsize
    out[:, :m0] = meta.view(np.uint8).reshape(n, m0)
    out[:, m0:m0 + 2 * F] = np.ascontiguousarray(x, dtype="<i2").view(np.uint8).reshape(n, 2 * F)
    out[:, m0 + 2 * F:m0 + 2 * F + 4 * A] = np.ascontiguousarray(visits, dtype="<i4").view(np.uint8).reshape(n, 4 * A)
    return out


def plan(R, C, packed, max_free, facts_for):
    """What does not depend on the modes: dict(root_of int32 [n]: per row the row index of its game's root if the row is a candidate,
    else -1; roots: the root rows in the order they are solved (F descending, game_idx ascending); status [n]: None, "unserved",
    "finished" or "relabel"; v [n], O [n]: of the rows to relabel; n_free [n]; games).  Two rows with one (game_idx, move_idx):
    ValueError."""
    acts, _ = ER.board(R, C)
    meta, x, _ = fields(R, C, packed)
    n = len(x)
    game, move = meta["game_idx"].astype(np.int64), meta["move_idx"].astype(np.int64)
    if len(set(zip(game.tolist(), move.tolist()))) != n:
        raise ValueError("two rows with the same (game_idx, move_idx)")
    free = x[:, acts] == 0
    n_free = free.sum(axis=1)
    root_of = np.full(n, -1, np.int32)
    status, v, O = [None] * n, [None] * n, [None] * n
    roots = []
    for g in sorted(set(game.tolist())):
        rows = np.nonzero(game == g)[0]
        rows = rows[np.argsort(move[rows], kind="stable")]
        late = np.nonzero(n_free[rows] <= max_free)[0]
        if not len(late):
            continue
        cand = rows[late[0]:]
        root = int(cand[0])
        roots.append(root)
        root_of[cand] = root
        served = [int(r) for r in cand if not (free[r] & ~free[root]).any()]
        facts = facts_for(x[root], x[served]) if served else []
        assert len(facts) == len(served)
        for r in cand:
            status[r] = "unserved"
        for r, f in zip(served, facts):
            status[r] = "finished" if f["finished"] else "relabel"
            if not f["finished"]:
                assert f["O"] and all(x[r][a] == 0 for a in f["O"]) and f["v"] in (-1, 0, 1)
                v[r], O[r] = int(f["v"]), list(f["O"])
    roots.sort(key=lambda r: (-int(n_free[r]), int(game[r])))
    return dict(root_of=root_of, roots=np.asarray(roots, np.int64), status=status, v=v, O=O, n_free=n_free, games=len(set(game.tolist())))


def apply(R, C, packed, p, pi_mode="restrict", z_mode=True, n_tables=None, max_free=31):
    """(the packed rows after the call, its stats) for plan() p of the same rows"""
    pm = PI_MODES[pi_mode] if isinstance(pi_mode, str) else int(pi_mode)
    HW = (R + 1) * (C + 1)
    F, A = 3 * HW, 2 * HW
    out = np.array(packed, dtype=np.uint8, copy=True)
    meta, _, vis = fields(R, C, packed)
    n = len(out)
    m0 = ROW_META.itemsize
    z_at = m0 - 3  # RowMeta: ... int8 player, int8 z, int16 pad
    assert ROW_META.fields["z"][1] == z_at
    st = dict.fromkeys(STATS, 0)
    by_free = np.zeros(max_free + 1, np.int64)
    for r in range(n):
        s = p["status"][r]
        if s in ("unserved", "finished"):
            st[s] += 1
        if s != "relabel":
            continue
        st["relabelled"] += 1
        by_free[p["n_free"][r]] += 1
        v, O = p["v"][r], p["O"][r]
        st["z_changed"] += int(int(meta["z"][r]) != v)
        if z_mode:
            out[r, z_at] = np.int8(v).view(np.uint8)
        if pm:
            new = np.zeros(A, np.int64)
            if pm == 2 and int(vis[r][O].astype(np.int64).sum()) != 0:
                new[O] = vis[r][O]
            else:
                new[O] = 1
            out[r, m0 + 2 * F:m0 + 2 * F + 4 * A] = new.astype("<i4").view(np.uint8)
    n_roots = len(p["roots"])
    st.update(rows=n, games=p["games"] if n else 0, roots=n_roots, chunks=-(-n_roots // n_tables) if n_tables else 0)
    st["by_free"] = by_free
    return out, st
