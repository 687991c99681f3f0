"""Both heads of csrc/nn.hip in logit space -- head conv (MFMA f16x3 or VALU), head_fc_fused, softmax, tanh -- against float64, at every
head shape and in every launch body.

oracle/nn_heads.py holds the criterion.  Per case, over the first and last workgroup of every launch, both sides of every
boundary and 32 random samples (at most 192; the float64 reference is evaluated on those alone):

    E_p = max |log p - log p64|                <=  K_HEAD[mode] * E32_p + 2^-23                       over p64 >= 1e-30
    |atanh v - u64|  (per element)             <=  K_HEAD[mode] * E32_v + 2^-23 / (1 - v64^2)         over |v64| <= 0.99

E32: torch float32's own distance from float64 in z / u.  K_HEAD: twice the largest ratio this file prints on the MI355X per
arithmetic mode, rounded up to a power of two (EXPERIMENTS.md, section 1, holds the table); tests/test_nn_heads_ref.py shows on
the CPU what fails the criterion at K = 16, that the cases below run every body and every head edge, and that their inputs keep
>= 90 % of the logits and values inside the masks.

Each case names the bodies oracle/nn_plan.py must list for its batch and says in its id what it is there for.  The samples on
either side of every launch boundary (and the first and last of the batch) are predicted again as a batch of their own and must
come back with the same bits: DESIGN.md's "a sample's (p, v) is bitwise independent of its batch and of which tower body
evaluated it", here across bodies, head shapes and both arithmetic modes.

SimpleNN's heads run in k_dense and k_head_fc: the same criterion on 3x3 around the 16 samples a k_head_fc workgroup holds."""
import functools

import numpy as np
import pytest
import torch

from oracle import nn_heads, nn_plan, nn_probe, nn_ref

pytestmark = pytest.mark.gpu

K_HEAD = nn_heads.K_HEAD
MAX_COMPARED = 192
HEAD_MT = 1     # csrc/nn.hip: sample tiles of 16 per k_head_fc workgroup


def C2(nt, order):
    return "k_tower<64,%d,0,1,true>/%s" % (nt, order)


def RR(t):
    return "k_tower_rem<64,RR>/<%s>" % t


def REM(c, t):
    return "k_tower_rem<%d>/<%s>" % (c, t)


def KT(c, t, prec):
    return "k_tower<%d,%s,%d>" % (c, t, prec)


# (rows, cols, channels, blocks, precision, head_channels, value_fc):
#     [(full rounds, tail in compute units, tail + samples, bodies the plan must name, what the case is there for)]
# "p" as the + part: the smallest +1, +2, ... that leaves the main launch a partial last workgroup
GEOMETRIES = [
    ((6, 6, 64, 2, 1, 16, 8), [(1, 0, 1, (C2(4, "table"), RR("2,2"),), "shipped"),
                              (1, 4, "p", (C2(4, "table"),), "shipped, partial workgroup")]),
    ((6, 6, 64, 1, 1, 8, 8), [(1, 1, 1, (C2(4, "table"), RR("4,4"),), "one full cout tile")]),
    ((6, 6, 64, 1, 1, 2, 1), [(1, 2, 1, (C2(4, "table"), RR("5,5"),), "masked tile, vf 1")]),
    ((6, 6, 64, 2, 1, 5, 17), [(1, 3, 1, (C2(4, "table"), RR("7,6"),), "odd hc, K % 16 = 5, ntv 2 with one valid output")]),
    ((6, 6, 64, 2, 1, 20, 64), [(1, 0, 1, (C2(4, "table"), RR("2,2"),), "n_ct 3: VALU conv in the two-cout-tile body, ntv 4"),
                               (1, 4, "p", (C2(4, "table"),), "VALU conv, partial workgroup")]),
    ((6, 6, 64, 1, 1, 32, 33), [(1, 0, 1, (KT(64, "7,6", 1), REM(64, "2,2"),), "n_ct 4, ntv 3 with one valid output")]),
    ((6, 6, 64, 1, 1, 64, 16), [(1, 0, 1, (KT(64, "7,6", 1), REM(64, "4,4"),), "n_ct 8, heads set the LDS size")]),
    ((6, 6, 64, 1, 1, 40, 8), [(1, 0, 1, (KT(64, "7,6", 1), REM(64, "2,2"),), "n_ct 5: VALU conv in f16x3")]),
    ((6, 6, 64, 2, 0, 16, 8), [(1, 0, 1, (KT(64, "7,6", 0), KT(64, "2,2", 0),), "shipped, exact f32")]),
    ((6, 6, 64, 1, 0, 20, 64), [(1, 1, 1, (KT(64, "7,6", 0), KT(64, "4,4", 0),), "VALU conv in both precisions")]),
    ((6, 6, 64, 1, 0, 5, 17), [(1, 2, 1, (KT(64, "7,6", 0), KT(64, "5,5", 0),), "odd hc, exact f32")]),
    ((6, 6, 64, 1, 0, 64, 16), [(1, 0, 1, (KT(64, "7,6", 0), KT(64, "4,4", 0),), "heads set the LDS size, exact f32")]),
    ((6, 6, 64, 1, 0, 2, 1), [(1, 3, "p", (KT(64, "7,6", 0),), "vf 1, partial workgroup, exact f32")]),
    ((1, 1, 64, 1, 1, 2, 1), [(1, 0, 1, (KT(64, "2,2", 1),), "A 8, K 8: one K-chunk, masked tile")]),
    ((1, 1, 32, 1, 1, 5, 17), [(1, 0, 1, (KT(32, "2,2", 1),), "A 8, K 20, 32 channels on the 2-tile kernel")]),
    ((1, 1, 64, 1, 1, 64, 16), [(1, 0, 1, (KT(64, "2,2", 1),), "n_ct 8 on 4 position tiles")]),
    ((1, 1, 64, 1, 1, 20, 64), [(1, 0, 1, (KT(64, "2,2", 1),), "VALU conv, 16 samples")]),
    ((1, 1, 64, 1, 0, 2, 1), [(1, 0, 1, (KT(64, "2,2", 0),), "A 8, K 8, exact f32")]),
    ((2, 3, 64, 1, 1, 16, 8), [(1, 0, 1, (C2(3, "natural"), RR("2,2"),), "12 positions, S capped at 16")]),
    ((2, 3, 64, 1, 1, 5, 17), [(1, 13, 1, (C2(3, "natural"), RR("7,6"),), "K 60")]),
    ((2, 3, 64, 1, 1, 64, 16), [(1, 0, 1, (KT(64, "7,6", 1), REM(64, "2,2"),), "n_ct 8, S 12")]),
    ((3, 3, 64, 1, 1, 16, 8), [(1, 0, 1, (C2(4, "table"), RR("2,2"),), "A % 16 = 0")]),
    ((3, 3, 64, 1, 1, 64, 16), [(1, 0, 1, (C2(2, "natural"), RR("2,2"),), "n_ct 8 in the two-cout-tile body of 2 tiles"),
                               (1, 7, 1, (C2(2, "natural"), RR("5,5"),), "n_ct 8")]),
    ((3, 3, 64, 1, 1, 32, 33), [(1, 10, "p", (KT(64, "7,6", 1),), "n_ct 4, partial workgroup")]),
    ((3, 3, 64, 1, 1, 40, 8), [(1, 0, 1, (C2(3, "natural"), RR("2,2"),), "n_ct 5: VALU conv in the two-cout-tile body of 3 tiles")]),
    ((3, 3, 64, 1, 0, 8, 8), [(1, 0, 1, (KT(64, "7,6", 0), KT(64, "2,2", 0),), "A % 16 = 0, exact f32")]),
    ((10, 10, 32, 1, 1, 16, 8), [(1, 0, 3, (KT(32, "4,4", 1),), "S 1, ntp 16, 32 channels on the 4-tile kernel")]),
    ((10, 10, 64, 1, 1, 20, 64), [(1, 0, 3, (KT(64, "4,4", 1),), "S 1, VALU conv, 20 FC jobs")]),
    ((10, 10, 64, 1, 1, 64, 16), [(1, 0, 3, (KT(64, "4,4", 1),), "S 1, n_ct 8")]),
    ((10, 10, 64, 1, 0, 64, 16), [(1, 0, 3, (KT(64, "4,4", 0),), "S 1, heads set the LDS size, exact f32")]),
    ((15, 7, 64, 1, 1, 32, 33), [(1, 0, 3, (KT(64, "4,4", 1),), "A 256")]),
    ((15, 7, 64, 1, 1, 40, 8), [(1, 0, 3, (KT(64, "4,4", 1),), "A 256, VALU conv")]),
    ((15, 7, 64, 1, 0, 5, 17), [(1, 0, 3, (KT(64, "4,4", 0),), "A 256, exact f32")]),
    ((9, 9, 64, 1, 1, 16, 8), [(1, 0, 1, (KT(64, "7,6", 1), REM(64, "5,5"),), "S 2")]),
    ((9, 9, 64, 1, 1, 5, 17), [(1, 1, 1, (KT(64, "7,6", 1),), "S 2, partial workgroup")]),
    ((9, 9, 64, 1, 1, 64, 16), [(1, 0, 3, (KT(64, "4,4", 1),), "S 1 by the heads")]),
    ((6, 5, 64, 1, 1, 16, 8), [(1, 0, 1, (KT(64, "7,6", 1), REM(64, "2,2"),), "H != W")]),
    ((6, 5, 64, 1, 1, 40, 8), [(1, 3, 1, (C2(3, "natural"), RR("7,6"),), "H != W, the heads move 6x5 to the two-cout-tile body")]),
    ((6, 5, 64, 1, 1, 64, 16), [(1, 0, 1, (KT(64, "4,4", 1), KT(64, "2,2", 1),), "H != W, n_ct 8, 4-tile kernels")]),
    ((6, 6, 16, 1, 1, 16, 8), [(1, 0, 1, (KT(32, "7,6", 1), REM(32, "2,2"),), "16 channels padded to 32")]),
    ((6, 6, 16, 1, 0, 5, 17), [(1, 0, 1, (KT(16, "7,6", 0), KT(16, "2,2", 0),), "16 channels, exact f32: VALU conv at C 16")]),
    ((6, 6, 32, 1, 1, 2, 1), [(1, 1, 1, (KT(32, "7,6", 1), REM(32, "4,4"),), "32 channels: KS 1")]),
    ((6, 6, 32, 1, 1, 20, 64), [(1, 2, 1, (KT(32, "7,6", 1), REM(32, "5,5"),), "32 channels, VALU conv")]),
    ((6, 6, 32, 1, 0, 8, 8), [(1, 0, 1, (KT(32, "7,6", 0), KT(32, "2,2", 0),), "32 channels, exact f32")]),
    ((6, 6, 128, 1, 1, 16, 8), [(1, 0, 1, (KT(128, "4,4", 1), KT(128, "2,2", 1),), "128 channels: KS 4")]),
    ((6, 6, 128, 1, 0, 5, 17), [(1, 0, 1, (KT(128, "4,4", 0), KT(128, "2,2", 0),), "128 channels, exact f32")]),
    ((3, 3, 16, 1, 1, 8, 8), [(1, 0, 1, (KT(32, "7,6", 1), REM(32, "2,2"),), "16 channels")]),
    ((3, 3, 16, 1, 0, 32, 33), [(1, 4, 1, (KT(16, "7,6", 0), KT(16, "4,4", 0),), "16 channels, exact f32"),
                               (1, 8, 1, (KT(16, "7,6", 0), KT(16, "5,5", 0),), "16 channels, exact f32")]),
    ((3, 3, 32, 1, 1, 5, 17), [(1, 4, 1, (KT(32, "7,6", 1), REM(32, "4,4"),), "32 channels")]),
    ((3, 3, 32, 1, 0, 16, 8), [(1, 4, 1, (KT(32, "7,6", 0), KT(32, "4,4", 0),), "32 channels, exact f32"),
                              (1, 8, 1, (KT(32, "7,6", 0), KT(32, "5,5", 0),), "32 channels, exact f32")]),
    ((3, 3, 128, 1, 1, 32, 33), [(1, 0, 1, (KT(128, "4,4", 1), KT(128, "2,2", 1),), "128 channels, n_ct 4")]),
    ((3, 3, 128, 1, 0, 20, 64), [(1, 7, 1, (KT(128, "7,6", 0), KT(128, "5,5", 0),), "128 channels, exact f32")]),
    ((2, 2, 128, 1, 1, 2, 1), [(1, 0, 1, (KT(128, "7,6", 1), REM(128, "2,2"),), "128 channels on the 7-tile kernel")]),
    ((2, 2, 128, 1, 1, 5, 17), [(1, 7, 1, (KT(128, "7,6", 1), REM(128, "4,4"),), "128 channels, K 45")]),
    ((2, 2, 128, 1, 1, 16, 8), [(1, 13, 1, (KT(128, "7,6", 1), REM(128, "5,5"),), "128 channels, 15 samples")]),
]
CASES = [(g, c) for g, cs in GEOMETRIES for c in cs]


def _id(gc):
    (r, c, ch, nb, prec, hc, vf), (rounds, tcu, plus, bodies, why) = gc
    return "%dx%d-%dch-prec%d-hc%d-vf%d-%dr+%dcu+%s-%s" % (r, c, ch, prec, hc, vf, rounds, tcu, plus, why.replace(" ", "_"))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(geo):
    r, c, ch, nb, prec, hc, vf = geo
    return nn_plan.Plan(r, c, ch, hc, vf, prec, _cus())


def _n(plan, case):
    rounds, tcu, plus = case[:3]
    base = rounds * plan.round + tcu * plan.cus
    if plus != "p":
        return base + plus
    n = base + 1
    while n % plan.S_main == 0:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def _model(geo):
    """1 - 2 blocks with the statistics of a trained network: logits that span a few units, head-conv weights that need their lo half"""
    r, c, ch, nb, prec, hc, vf = geo
    return nn_heads.trained_like_model(r, c, ch, nb, hc, vf, r * 131 + c * 17 + ch + nb + 7 * hc + vf)


def _inputs(geo, n):
    return nn_probe.positions(geo[0], geo[1], n, geo[0] * 7 + geo[1] + geo[5])


def _n_slots(geo):
    """the largest batch of any case on this board in this mode: the engine's size does not depend on the order of the tests"""
    return max(_n(_plan(g), c) for g, c in CASES if (g[0], g[1], g[4]) == (geo[0], geo[1], geo[4]))


_engine = {}


def _engine_for(geo):
    """one engine per (board, precision) at a time; load_state_dict configures and commits the case's network on it"""
    from dotsboxesaz_amd.engine import Engine
    key = (geo[0], geo[1], geo[4])
    if _engine.get("key") != key:
        _close_engine()
        _engine.update(key=key, e=Engine(geo[0], geo[1], _n_slots(geo), mcts_num_read=8, evaluator="resnet", nn_precision=geo[4]))
    return _engine["e"]


def _close_engine():
    if _engine.get("e") is not None:
        _engine["e"].close()
    _engine.clear()


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    _close_engine()


def _compare_idx(plan, n, seed):
    idx = set(plan.workgroup_edges(n))
    idx.update(np.random.RandomState(seed).choice(n, min(32, n), replace=False).tolist())
    idx = sorted(idx)
    assert len(idx) <= MAX_COMPARED
    return idx


def _boundary_idx(plan, n):
    """the samples on either side of every launch boundary, and the first and last of the batch"""
    idx = {0, n - 1}
    for l in plan.launches(n):
        idx.update(i for i in (l.first - 1, l.first) if 0 <= i < n)
    return sorted(idx)


def _check(ref, p, v, prec, what):
    """the assertions on the compared samples; returns the ratios K_HEAD is set from"""
    p, v = np.asarray(p), np.asarray(v).reshape(-1)
    assert np.isfinite(p[ref.mask_p]).all() and (p[ref.mask_p] > 0).all() and np.isfinite(v).all() and (np.abs(v) < 1).all()
    e_p, e_v, ip, iv = ref.errors(p, v)
    r_p, r_v = ref.ratios(p, v)
    print("RATIO %s E_p %.2e E32_p %.2e ratio_p %5.2f (sample %d, action %d) E_v %.2e E32_v %.2e ratio_v %5.2f (sample %d); %d samples, "
          "%.0f %% of the logits, %.0f %% of the values" % (what, e_p, ref.e32_p, r_p, ip[0], ip[1], e_v, ref.e32_v, r_v, iv, len(v),
                                                          100 * ref.mask_p.mean(), 100 * ref.mask_v.mean()))
    k = K_HEAD[prec]
    assert k <= nn_heads.K_MAX
    dp, dv = ref.deltas(p, v)
    assert e_p <= k * ref.e32_p + ref.allow_p, (e_p, ref.e32_p, ip)
    assert (dv <= k * ref.e32_v + ref.allow_v).all(), (e_v, ref.e32_v, iv)
    return r_p, r_v


@pytest.mark.parametrize("gc", CASES, ids=_id)
def test_heads_in_logit_space(gc):
    geo, case = gc
    bodies = case[3]
    plan = _plan(geo)
    n = _n(plan, case)
    launches = plan.launches(n)
    assert tuple(l.body for l in launches) == bodies, (n, launches)
    if case[2] == "p":
        assert len(launches) == 1 and launches[0].count % launches[0].S != 0
    m, X = _model(geo), _inputs(geo, n)
    idx = _compare_idx(plan, n, n)
    ref = nn_heads.Reference(m, X[idx])
    assert ref.mask_p.mean() >= 0.9 and ref.mask_v.mean() >= 0.9
    e = _engine_for(geo)
    c = m.cfg
    e.load_state_dict(m.state_dict(), "resnet", c["channels"], c["blocks"], c["head_channels"], c["value_fc"])
    p, v = e.predict(X)
    assert e.counters()["f32_fallback_evals"] == 0
    assert p.shape == (n, 2 * plan.HW) and np.isfinite(p).all() and np.isfinite(v).all()
    _check(ref, p[idx], v[idx], geo[4], "%-100s n %5d bodies %-50s" % (_id(gc), n, "+".join(bodies)))
    # the bitwise contract: the boundary samples as a batch of their own (another body, other neighbours, another workgroup size)
    b = _boundary_idx(plan, n)
    pb, vb = e.predict(X[b])
    assert e.counters()["f32_fallback_evals"] == 0
    assert np.array_equal(pb, p[b]) and np.array_equal(vb, v[b]), (b, np.abs(pb - p[b]).max(), np.abs(vb - v[b]).max())


# ---------------------------------------------------------------- SimpleNN: k_dense and k_head_fc
@functools.lru_cache(maxsize=None)
def _simple():
    torch.manual_seed(11)
    m = nn_ref.SimpleNNRef()
    nn_ref.randomize_bn(m, 3)
    return m


SIMPLE_N = [1, 16, 16 * HEAD_MT + 1, 33]    # one sample, a full workgroup of k_head_fc, one more than it holds, two and one


@pytest.mark.parametrize("precision", [0, 1])
def test_simplenn_heads_in_logit_space(precision):
    """SimpleNNRef on 3x3: log p and atanh v = value_fc(x) against float64 at n = 1, 16, 17 (= 16 HEAD_MT + 1) and 33, one engine;
    the first and last sample of the largest batch again as a batch of their own: same bits"""
    from dotsboxesaz_amd.engine import Engine
    m = _simple()
    X = nn_probe.positions(3, 3, max(SIMPLE_N), 5)
    ref = nn_heads.Reference(m, X)
    assert ref.mask_p.mean() >= 0.9 and ref.mask_v.mean() >= 0.9
    e = Engine(3, 3, 64, mcts_num_read=8, evaluator="simplenn", nn_precision=precision)
    try:
        e.load_state_dict(m.state_dict(), "simplenn")
        for n in SIMPLE_N:
            p, v = e.predict(X[:n])
            assert p.shape == (n, 32) and v.shape == (n, 1)
            _check(nn_heads.Reference(m, X[:n]) if n < len(X) else ref, p, v, precision, "SimpleNN 3x3 prec%d n %2d" % (precision, n))
        b = [0, len(X) - 1]
        pb, vb = e.predict(X[b])
        assert np.array_equal(pb, p[b]) and np.array_equal(vb, v[b])
    finally:
        e.close()
