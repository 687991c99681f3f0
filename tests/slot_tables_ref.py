"""The table evaluator of the search restated in numpy (helper of test_slot_tables_ref_cpu.py / test_hip_slot_tables.py), written
from the definitions in include/dbaz.h (dbaz_attach_endgame, dbaz_attach_tables, dbaz_exact_policy) on top of
endgame_policy_ref.py.

Per start position ONE table is solved (endgame_policy_ref.subgame over the start's free edges, compact edge j = the j-th free
real edge in ascending action order, bit j of an index = that edge has been drawn since).  Any row whose free edges are a subset
of some start's is answered by lookup: p is one-hot by endgame_pick's rule (pick_key, mix), v = sign(margin + D[mask]); a
finished game gets p = 0 and v = get_result, as in endgame_policy_ref.policy.  Which superset start answers a row cannot matter:
D depends on the free edges only.  A row no start serves gets p = 0, v = 0, solved = False."""
import numpy as np

import endgame_ref as ER
import endgame_policy_ref as PR
from solver_ref import mix

_tables = {}  # (R, C, free edges) -> the solved table: shared by every instance, whatever its seed


class SlotTablesRef:
    def __init__(self, R, C, starts_x, seed=0, max_free=31):
        self.R, self.C, self.seed, self.max_free = R, C, seed, max_free
        self.acts, self.boxes = ER.board(R, C)
        self.HW, self.A, self.B = (R + 1) * (C + 1), 2 * (R + 1) * (C + 1), R * C
        self.roots, self._rows = [], {}
        solved = set()
        for x in np.asarray(starts_x).reshape(-1, 3 * self.HW):
            free = [int(a) for a in self.acts if x[a] == 0]
            if len(free) > max_free:
                continue
            key = (R, C, tuple(free))
            if key in solved:  # one table per distinct free-edge set
                continue
            solved.add(key)
            if key not in _tables:
                idx = {a: j for j, a in enumerate(free)}
                masks = [sum(1 << idx[a] for a in b if a in idx) for b in self.boxes]
                masks = [bm for bm in masks if bm]
                _tables[key] = dict(free=free, idx=idx, set=frozenset(free), masks=masks, D=PR.subgame(len(free), masks))
            self.roots.append(_tables[key])

    def table(self, i):
        """root i's table as int8 [2^F]"""
        return self.roots[i]["D"].astype(np.int8)

    def one(self, x):
        """(picked action or -1, v, served) of one feature row"""
        x = np.asarray(x).ravel().astype(np.int16)
        key = x.tobytes()
        if key not in self._rows:
            self._rows[key] = self._one(x)
        return self._rows[key]

    def _one(self, x):
        free = [int(a) for a in self.acts if x[a] == 0]
        root = next((r for r in self.roots if r["set"].issuperset(free)), None)
        if root is None:
            return -1, 0.0, False
        m = sum(1 << j for a, j in root["idx"].items() if x[a] != 0)
        D, masks = root["D"], root["masks"]
        closed = sum(1 for b in self.boxes if all(x[a] != 0 for a in b))
        own = int(x[2 * self.HW])
        mine = (self.B - own) // 2
        theirs = closed - mine
        opp = self.B - 2 * theirs
        res = 0 if (own == 0 and opp == 0) else 1 if own < 0 else -1 if opp < 0 else None
        if res is not None:
            return -1, float(res), True
        v = float(np.sign(mine - theirs + int(D[m])))
        q = {}
        for a in free:
            t = m | 1 << root["idx"][a]
            c = sum(1 for bm in masks if t & bm == bm and m & bm != bm)
            d = int(D[t])
            q[a] = c + d if c > 0 else -d
        best = max(q.values())
        opt = [a for a in free if q[a] == best]  # ascending action order
        k = mix(PR.pick_key(self.R, self.C, x), self.seed) % len(opt) if self.seed else 0
        return opt[k], v, True

    def policy(self, x):
        """x [n, 3*H*W] -> (p float32 [n, A], v float32 [n], served bool [n])"""
        x = np.asarray(x).reshape(-1, 3 * self.HW)
        p = np.zeros((len(x), self.A), np.float32)
        v = np.zeros(len(x), np.float32)
        served = np.zeros(len(x), bool)
        for r in range(len(x)):
            a, v[r], served[r] = self.one(x[r])
            if a >= 0:
                p[r, a] = 1.0
        return p, v, served

    def evaluator(self, strict=True):
        """an evaluate(x) -> (p, v) for Engine.search_external; strict: every leaf of a search from the starts must be served"""
        def evaluate(x):
            p, v, served = self.policy(x)
            assert served.all() or not strict, "a leaf that no start's table serves"
            return p, v
        return evaluate
