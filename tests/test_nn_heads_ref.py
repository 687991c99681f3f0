"""oracle/nn_heads.py and the case table of tests/test_hip_nn_heads.py on the CPU: the criterion in logit space has teeth at the
largest K allowed, the GPU cases run every launch body their head shapes make reachable and every head edge csrc/nn.hip has, and
their inputs keep the float64 reference inside the masks."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from oracle import nn_heads, nn_plan, nn_probe

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_MAX = 16      # the largest K the GPU tests may use (nn_probe.K_MAX)


@functools.lru_cache(maxsize=None)
def _gpu_file():
    spec = importlib.util.spec_from_file_location("_heads_cases", os.path.join(REPO, "tests", "test_hip_nn_heads.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    return T


# ---------------------------------------------------------------- teeth
# (rows, cols, channels, blocks, head_channels, value_fc): the shipped shape, then odd ones
TEETH = [(6, 6, 64, 2, 16, 8), (6, 6, 64, 1, 5, 17), (3, 3, 64, 1, 20, 64), (1, 1, 64, 1, 2, 1), (6, 5, 64, 1, 32, 33), (2, 3, 64, 1, 64, 16)]


@pytest.mark.parametrize("shape", TEETH, ids=lambda s: "%dx%d-%dch-%db-hc%d-vf%d" % s)
def test_criterion_has_teeth(shape):
    """E <= K * E_32 + allow at K = K_MAX = 16, on 96 positions.  Untouched torch float32, returned as float32 (p, v), passes at
    K = 1 by construction.  Every mutant of oracle/nn_heads.py fails by a factor of 4 or more beyond K = 16, in the head it
    damages and only there.  The factors E / (16 E_32 + allow) over the six shapes (printed per shape):
        (a) lo half of the policy head-conv weights lost in one tile     10.6 ... 43.6   (log p)
        (b) the same for the value rows                                  13.0 ... 52.3   (atanh v)
        (c) last live K element of the last policy output dropped         559 ... 48 736
        (d) value FC0 outputs 16.. dropped (value_fc > 16)             34 927 ... 158 818
        (e) FC bias of the last policy tile lost                        1 011 ... 23 272
        (f) sample ns - 1 gets the head activations of sample ns - 2   28 237 ... 147 569 in both heads
    The head a mutant leaves alone stays at 0.1 (the float32 rounding of the output alone)."""
    r, c, ch, nb, hc, vf = shape
    m = nn_heads.trained_like_model(r, c, ch, nb, hc, vf, r * 131 + c * 17 + ch + nb + 7 * hc + vf)
    X = nn_probe.positions(r, c, 96, 3)
    R = nn_heads.Reference(m, X)
    assert R.mask_p.mean() >= 0.9 and R.mask_v.mean() >= 0.9
    assert 1e-7 < R.e32_p < 2e-5 and 2e-8 < R.e32_v < 2e-5
    xp, xv = R.excess(*nn_heads.as_f32_outputs(R.f32["lp"], R.f32["u"]), 1)
    print("%s untouched torch float32 at K = 1: log p %.2f, atanh v %.2f of the bound" % (shape, xp, xv))
    assert xp <= 1 and xv <= 1
    A = 2 * (r + 1) * (c + 1)
    S = nn_plan.Plan(r, c, ch, hc, vf, 1, 256).S_main
    assert (R.f64["ap"][:, nn_heads.live_k(R)] != 0).mean() >= 0.5
    muts = [("a", "p", nn_heads.mutant_policy_lo_lost(hc, 0)), ("b", "v", nn_heads.mutant_value_lo_lost(hc)),
            ("c", "p", nn_heads.mutant_last_k_dropped(R)), ("e", "p", nn_heads.mutant_last_tile_bias_lost(A)),
            ("f", "pv", nn_heads.mutant_clamp_off_by_one(S))]
    if vf > 16:
        assert (R.f64["h"][:, 16:] > 0).any()       # (trained_like_model: the last FC0 tile is alive)
        muts.append(("d", "v", nn_heads.mutant_fc0_tail_dropped()))
    for name, where, mut in muts:
        xp, xv = R.excess(*R.mutant(**mut), K_MAX)
        print("%s mutant (%s): log p %.1f, atanh v %.1f times the bound at K = 16" % (shape, name, xp, xv))
        assert (xp >= 4) == ("p" in where) and (xv >= 4) == ("v" in where), (name, xp, xv)
        assert "p" in where or xp <= 1
        assert "v" in where or xv <= 1


# ---------------------------------------------------------------- the case table
def _strip(b):
    return b.split("/table")[0].split("/natural")[0]


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_the_gpu_cases_run_every_reachable_body(cus, monkeypatch):
    """tests/test_hip_nn_heads.py without a GPU: every case's batch gives exactly the launches the case names, whatever the number
    of compute units, and between them the cases run every instantiation some board reaches with the head shapes of that file
    (every head_channels x value_fc of them; k_tower<64,2,0,1,true>, dead with the shipped heads, is among them)"""
    T = _gpu_file()
    monkeypatch.setattr(T, "_cus", lambda: cus)
    assert 40 <= len(T.CASES) <= 60 and len(set(T._id(gc) for gc in T.CASES)) == len(T.CASES)
    run = set()
    for geo, case in T.CASES:
        plan = T._plan(geo)
        n = T._n(plan, case)
        launches = plan.launches(n)
        assert tuple(l.body for l in launches) == case[3], (T._id((geo, case)), n)
        if case[2] == "p":
            assert len(launches) == 1 and launches[0].count % launches[0].S != 0
        assert len(T._compare_idx(plan, n, n)) <= T.MAX_COMPARED
        assert n <= plan.round + max([plan.round] + [lim for lim, _ in plan.tail_limits() if lim])     # one round plus a tail
        assert geo[3] <= 2                                                                             # blocks
        run.update(_strip(b) for b in case[3])
    hcs = tuple(sorted(set(g[5] for g, _ in T.CASES)))
    vfs = tuple(sorted(set(g[6] for g, _ in T.CASES)))
    reach = nn_plan.reachable(head_channels=hcs, value_fc=vfs)
    assert "tower_dispatch_c2 k_tower<64,2,0,1,true>" in reach
    assert set(nm.split(" ", 1)[1] for nm in reach) <= run, sorted(set(nm.split(" ", 1)[1] for nm in reach) - run)


def _facts(T, geo, case, cus=256):
    """what the head code of csrc/nn.hip does in this case, in plain integers"""
    r, c, ch, nb, prec, hc, vf = geo
    plan = nn_plan.Plan(r, c, ch, hc, vf, prec, cus)
    n = T._n(plan, case)
    ls = plan.launches(n)
    HW = plan.HW
    n_ct = (2 * hc + 15) // 16
    f = dict(r=r, c=c, ch=ch, C=plan.C, prec=prec, hc=hc, vf=vf, HW=HW, A=2 * HW, K=hc * HW, n_ct=n_ct,
             mfma=prec == 1 and plan.C >= 32 and n_ct in (1, 2, 4, 8), ntp=(2 * HW + 15) // 16, ntv=(vf + 15) // 16,
             S=[l.S for l in ls], partial=any(l.count % l.S for l in ls), c2=bool(plan.c2), nt_c2=plan.NT_c2 if plan.c2 else 0,
             shape=(hc, vf), board=(r, c))
    f["valu"] = not f["mfma"]
    img, need0, need1 = plan.lds_parts(plan.S)
    f["heads_set_lds"] = need1 > max(img, need0)
    return f


# every head edge of nn.hip (the list of the issue this file answers), one predicate each
EDGES = {
    "MFMA conv, n_ct 1, full tile (2 hc = 16)": lambda f: f["mfma"] and f["hc"] == 8,
    "MFMA conv, n_ct 1, masked output rows (2 hc < 16)": lambda f: f["mfma"] and 2 * f["hc"] < 16,
    "MFMA conv, n_ct 1, masked, odd hc": lambda f: f["mfma"] and f["hc"] == 5,
    "MFMA conv, n_ct 2": lambda f: f["mfma"] and f["n_ct"] == 2,
    "MFMA conv, n_ct 4": lambda f: f["mfma"] and f["n_ct"] == 4,
    "MFMA conv, n_ct 8 (ngrp 1)": lambda f: f["mfma"] and f["n_ct"] == 8,
    "MFMA conv, n_ct 8 in the two-cout-tile body": lambda f: f["mfma"] and f["n_ct"] == 8 and f["c2"],
    "VALU conv inside f16x3, hc 17..24": lambda f: f["prec"] == 1 and f["valu"] and f["n_ct"] == 3,
    "VALU conv inside f16x3, hc 33..56": lambda f: f["prec"] == 1 and f["valu"] and 5 <= f["n_ct"] <= 7,
    "VALU conv inside the two-cout-tile body": lambda f: f["prec"] == 1 and f["valu"] and f["c2"],
    "VALU conv inside f16x3 at 32 channels": lambda f: f["prec"] == 1 and f["valu"] and f["C"] == 32,
    "the same VALU head shape in exact f32 on the same board": lambda f: f["prec"] == 0 and f["shape"] == (20, 64) and f["board"] == (6, 6),
    "... and in f16x3": lambda f: f["prec"] == 1 and f["shape"] == (20, 64) and f["board"] == (6, 6),
    "K % 16 != 0, MFMA conv": lambda f: f["K"] % 16 and f["mfma"],
    "K % 16 != 0, VALU conv": lambda f: f["K"] % 16 and f["valu"],
    "K % 16 != 0 in a partial workgroup, MFMA conv": lambda f: f["K"] % 16 and f["mfma"] and f["partial"],
    "K % 16 != 0 in a partial workgroup, VALU conv": lambda f: f["K"] % 16 and f["valu"] and f["partial"],
    "K < 16: one K-chunk": lambda f: f["K"] < 16,
    "partial workgroup (columns beyond ns read min(jrow, ns - 1))": lambda f: f["partial"],
    "16 samples per workgroup (no column beyond ns)": lambda f: 16 in f["S"],
    "one sample per workgroup": lambda f: f["S"] == [1],
    "two samples per workgroup (9x9)": lambda f: f["board"] == (9, 9) and 2 in f["S"],
    "12 positions, S capped at 16 (2x3)": lambda f: f["board"] == (2, 3) and 16 in f["S"],
    "A < 16 (1x1)": lambda f: f["A"] < 16,
    "A % 16 = 0 (3x3)": lambda f: f["A"] == 32,
    "A % 16 != 0 beyond one tile": lambda f: f["A"] > 16 and f["A"] % 16,
    "ntp 16 (10x10)": lambda f: f["ntp"] == 16 and f["A"] < 256,
    "A 256 (15x7)": lambda f: f["A"] == 256,
    "H != W": lambda f: f["r"] != f["c"],
    "ntv 1": lambda f: f["ntv"] == 1,
    "ntv 2": lambda f: f["ntv"] == 2,
    "ntv 3": lambda f: f["ntv"] == 3,
    "ntv 4, value_fc at its maximum": lambda f: f["ntv"] == 4 and f["vf"] == 64,
    "last value tile with a single valid output": lambda f: f["vf"] > 16 and f["vf"] % 16 == 1,
    "value_fc 1": lambda f: f["vf"] == 1,
    "exact f32 (VALU conv) at 16 channels": lambda f: f["prec"] == 0 and f["C"] == 16,
    "exact f32 at 32 channels": lambda f: f["prec"] == 0 and f["C"] == 32,
    "exact f32 at 64 channels": lambda f: f["prec"] == 0 and f["C"] == 64,
    "exact f32 at 128 channels": lambda f: f["prec"] == 0 and f["C"] == 128,
    "f16x3, 16 channels padded to 32": lambda f: f["prec"] == 1 and f["ch"] == 16 and f["C"] == 32 and f["mfma"],
    "f16x3 MFMA conv at 32 channels (KS 1)": lambda f: f["mfma"] and f["ch"] == 32,
    "f16x3 MFMA conv at 128 channels (KS 4)": lambda f: f["mfma"] and f["C"] == 128,
    "f16x3 at 128 channels, n_ct 4": lambda f: f["mfma"] and f["C"] == 128 and f["n_ct"] == 4,
    "lg behind the weights and the stage (VALU conv)": lambda f: f["valu"],
    "lg behind the stage alone (MFMA conv)": lambda f: f["mfma"],
    "the head phase sets the LDS size, f16x3": lambda f: f["heads_set_lds"] and f["prec"] == 1,
    "the head phase sets the LDS size, exact f32": lambda f: f["heads_set_lds"] and f["prec"] == 0,
    "the tower sets the LDS size": lambda f: not f["heads_set_lds"],
    "two-cout-tile body of 2 tiles": lambda f: f["nt_c2"] == 2,
    "two-cout-tile body of 3 tiles": lambda f: f["nt_c2"] == 3,
    "two-cout-tile body of 4 tiles": lambda f: f["nt_c2"] == 4,
}
SHAPES = {(16, 8), (8, 8), (2, 1), (5, 17), (20, 64), (32, 33), (64, 16), (40, 8)}
BOARDS = {(1, 1), (2, 3), (3, 3), (6, 6), (6, 5), (9, 9), (10, 10), (15, 7)}


def test_the_gpu_cases_reach_every_head_edge():
    T = _gpu_file()
    facts = [_facts(T, geo, case) for geo, case in T.CASES]
    for name, pred in EDGES.items():
        assert any(pred(f) for f in facts), name
    assert SHAPES == set(f["shape"] for f in facts)
    assert BOARDS <= set(f["board"] for f in facts)
    # 64 channels on every board; 16, 32 and 128 on 6x6 and 3x3 with two head shapes each
    assert BOARDS == set(f["board"] for f in facts if f["ch"] == 64)
    for ch in (16, 32, 128):
        for board in ((6, 6), (3, 3)):
            assert len(set(f["shape"] for f in facts if f["ch"] == ch and f["board"] == board)) >= 2, (ch, board)
    # both precisions for a VALU and for an MFMA head shape on the same board
    for shape in ((20, 64), (16, 8)):
        assert {0, 1} == set(f["prec"] for f in facts if f["shape"] == shape and f["board"] == (6, 6) and f["ch"] == 64)


def test_the_gpu_cases_keep_the_reference_inside_the_masks():
    """a condition on the inputs: in every case the float64 reference alone keeps >= 90 % of the logits (p64 >= 1e-30) and >= 90 %
    of the values (|v64| <= 0.99) of the compared samples, torch float32 differs from it in both heads (E_32 > 0: the heads are
    alive) and the logits span more than half a unit"""
    T = _gpu_file()
    T._cus = lambda: 256
    for geo, case in T.CASES:
        plan = T._plan(geo)
        n = T._n(plan, case)
        idx = T._compare_idx(plan, n, n)
        R = nn_heads.Reference(T._model(geo), T._inputs(geo, n)[idx])
        name = T._id((geo, case))
        assert R.mask_p.mean() >= 0.9 and R.mask_v.mean() >= 0.9, (name, R.mask_p.mean(), R.mask_v.mean())
        assert R.e32_p > 0 and R.e32_v > 0 and np.ptp(R.z, axis=1).mean() > 0.5 and R.u.std() > 1e-3, (name, R.e32_p, R.e32_v)
