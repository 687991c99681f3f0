"""The tower of csrc/nn.hip, element by element and launch body by launch body, against float64.

Every case names the launch bodies it runs (oracle/nn_plan.py restates which body takes which samples of a batch, from the
device's compute-unit count), asserts that the plan of its batch size holds exactly those, and reads the tower output through
the probe head of oracle/nn_probe.py: log p = log_softmax(s' t[c0:c0+2]).  Compared are the first and last workgroup of every
launch, the samples on either side of every boundary and 32 random ones (at most 192), in every probe the case asks for:

    E_hip = max |log p_hip - log p_f64|   <=   K[mode] * E_32,     E_32 = the same for torch's own float32 tower

K: twice the largest E_hip / E_32 observed per arithmetic mode, rounded up to a power of two (EXPERIMENTS.md, section 1, holds
the table); the CPU tests of tests/test_nn_probe_ref.py show what fails it at K = 16."""
import functools

import numpy as np
import pytest
import torch

from oracle import nn_plan, nn_probe, nn_ref

pytestmark = pytest.mark.gpu

K = nn_probe.K     # per nn_precision; measured, see EXPERIMENTS.md (the criterion allows at most 16)
MAX_COMPARED = 192

C2T, C2N = "k_tower<64,4,0,1,true>/table", "k_tower<64,4,0,1,true>/natural"


def RR(t):
    return "k_tower_rem<64,RR>/<%s>" % t


def REM(c, t):
    return "k_tower_rem<%d>/<%s>" % (c, t)


def KT(c, t, prec):
    return "k_tower<%d,%s,%d>" % (c, t, prec)


ALL, TILE = "all", "tile"   # probes: every C/2 of them, or one per cout tile of 16 channels
# (rows, cols, channels, blocks, precision): [(full rounds, tail in compute units, tail + samples, bodies the plan must name, probes)]
# "p" as the + part: the smallest +1, +2, ... that leaves the main launch a partial last workgroup
GEOMETRIES = [
    ((6, 6, 64, 2, 1), [(1, 0, 1, (C2T, RR("2,2")), ALL), (1, 1, 0, (C2T, RR("2,2")), TILE),
                        (1, 1, 1, (C2T, RR("4,4")), ALL), (1, 2, 0, (C2T, RR("4,4")), TILE),
                        (1, 2, 1, (C2T, RR("5,5")), ALL), (1, 3, 0, (C2T, RR("5,5")), TILE),
                        (1, 3, 1, (C2T, RR("7,6")), ALL), (1, 4, 0, (C2T, RR("7,6")), TILE),
                        (1, 4, 1, (C2T,), TILE), (1, 4, "p", (C2T,), ALL), (0, 0, 3, (RR("2,2"),), TILE)]),
    ((3, 3, 64, 2, 1), [(1, 0, 1, (C2T, RR("2,2")), ALL), (1, 4, 1, (C2T, RR("4,4")), ALL), (1, 8, 1, (C2T, RR("5,5")), ALL),
                        (1, 10, 1, (C2T, RR("7,6")), ALL), (1, 13, "p", (C2T,), TILE)]),
    # 6x5 (H != W): 5 x 42 rows fill the two-cout-tile body too badly, its main launch is the 7-tile kernel (not RR)
    ((6, 5, 64, 2, 1), [(1, 0, 1, (KT(64, "7,6", 1), REM(64, "2,2")), ALL), (1, 2, 1, (KT(64, "7,6", 1), REM(64, "5,5")), ALL),
                        (1, 1, 1, (KT(64, "7,6", 1), REM(64, "4,4")), TILE)]),
    ((5, 5, 64, 2, 1), [(1, 1, 1, (C2T, RR("4,4")), ALL), (1, 4, 1, (C2T, RR("7,6")), TILE)]),
    ((6, 7, 64, 1, 1), [(1, 0, 1, (C2T, RR("4,4")), ALL)]),                                    # H != W through the row table
    # the two-cout-tile body in natural row order: 4 tiles per wave pair without a table (8x8), and 3 tiles (7x7)
    ((8, 8, 64, 1, 1), [(1, 1, 1, (C2N, RR("7,6")), ALL), (1, 0, 1, (C2N, RR("5,5")), TILE)]),
    ((7, 7, 64, 1, 1), [(1, 0, 1, ("k_tower<64,3,0,1,true>/natural", RR("4,4")), ALL)]),
    # boards of at most 12 positions: 208 rows would be 17 ... 52 samples, and a workgroup holds 16 (the columns of the head FC's
    # MFMA; nn_commit did not cap it, and samples 16.. of a full workgroup of the one-cout-tile bodies came back without logits).
    # 16 samples: 1x1 is 4 tiles, the 2-tile kernel as the only launch; 1x3 8 tiles; 2x2 9 tiles, the 7-tile kernel
    ((1, 3, 64, 1, 1), [(1, 0, 1, (KT(64, "4,4", 1), KT(64, "2,2", 1)), ALL)]),
    ((1, 1, 64, 1, 1), [(1, 0, 1, (KT(64, "2,2", 1),), ALL)]),
    ((1, 1, 32, 1, 1), [(1, 0, 1, (KT(32, "2,2", 1),), TILE)]),
    ((2, 2, 64, 1, 1), [(1, 0, 1, (KT(64, "7,6", 1), REM(64, "2,2")), ALL), (1, 14, 1, (KT(64, "7,6", 1), REM(64, "5,5")), TILE)]),
    ((2, 2, 64, 1, 0), [(1, 0, 1, (KT(64, "7,6", 0), KT(64, "2,2", 0)), ALL), (1, 14, 1, (KT(64, "7,6", 0), KT(64, "5,5", 0)), TILE)]),
    ((1, 1, 64, 1, 0), [(1, 0, 1, (KT(64, "2,2", 0),), TILE)]),
    # 9x9: the 7-tile kernel that is not RR as the main launch, with and without its <5,5> remainder
    ((9, 9, 64, 1, 1), [(1, 0, 1, (KT(64, "7,6", 1), REM(64, "5,5")), ALL), (1, 1, 1, (KT(64, "7,6", 1),), TILE),
                        (1, 1, 0, (KT(64, "7,6", 1), REM(64, "5,5")), TILE)]),
    ((6, 6, 32, 2, 1), [(1, 0, 1, (KT(32, "7,6", 1), REM(32, "2,2")), ALL), (1, 1, 1, (KT(32, "7,6", 1), REM(32, "4,4")), ALL),
                        (1, 2, 1, (KT(32, "7,6", 1), REM(32, "5,5")), ALL), (1, 3, "p", (KT(32, "7,6", 1),), TILE)]),
    ((6, 6, 128, 1, 1), [(1, 0, 1, (KT(128, "4,4", 1), KT(128, "2,2", 1)), ALL), (1, 1, 1, (KT(128, "4,4", 1),), TILE)]),
    # one sample in 8 tiles: the 4-tile f16x3 kernel as the only launch (no remainder kernel, no two-cout-tile body)
    ((10, 10, 64, 1, 1), [(1, 0, 3, (KT(64, "4,4", 1),), ALL)]),
    ((10, 10, 32, 1, 1), [(1, 0, 3, (KT(32, "4,4", 1),), TILE)]),
    # 128 channels with 144 rows per workgroup (3x3: 9 samples): the images and the static LDS of k_tower_rem<128> do not fit
    # into 160 KiB together and nn_commit failed; it now takes 8 samples, which the 4-tile kernel holds without a remainder kernel
    ((3, 3, 128, 1, 1), [(1, 0, 1, (KT(128, "4,4", 1), KT(128, "2,2", 1)), ALL), (1, 4, "p", (KT(128, "4,4", 1),), TILE)]),
    # 2x2: 15 samples of 9 rows, the 7-tile kernel and k_tower_rem<128>
    ((2, 2, 128, 1, 1), [(1, 0, 1, (KT(128, "7,6", 1), REM(128, "2,2")), ALL), (1, 7, 1, (KT(128, "7,6", 1), REM(128, "4,4")), TILE),
                         (1, 13, 1, (KT(128, "7,6", 1), REM(128, "5,5")), TILE), (1, 14, "p", (KT(128, "7,6", 1),), TILE)]),
    # 16 channels in f16x3 run zero-padded to 32 channels on the f16x3 kernels (nn_configure); in exact f32 as 16
    ((6, 6, 16, 2, 1), [(1, 0, 1, (KT(32, "7,6", 1), REM(32, "2,2")), ALL)]),
    ((6, 6, 16, 2, 0), [(1, 0, 1, (KT(16, "7,6", 0), KT(16, "2,2", 0)), ALL), (1, 1, 1, (KT(16, "7,6", 0), KT(16, "4,4", 0)), TILE),
                        (1, 2, 1, (KT(16, "7,6", 0), KT(16, "5,5", 0)), TILE)]),
    # exact f32, 64 channels: roles 0..3 of the four launches and the boundaries between them
    ((6, 6, 64, 2, 0), [(1, 0, 1, (KT(64, "7,6", 0), KT(64, "2,2", 0)), ALL), (1, 1, 0, (KT(64, "7,6", 0), KT(64, "2,2", 0)), TILE),
                        (1, 1, 1, (KT(64, "7,6", 0), KT(64, "4,4", 0)), ALL), (1, 2, 0, (KT(64, "7,6", 0), KT(64, "4,4", 0)), TILE),
                        (1, 2, 1, (KT(64, "7,6", 0), KT(64, "5,5", 0)), ALL), (1, 3, 0, (KT(64, "7,6", 0), KT(64, "5,5", 0)), TILE),
                        (1, 3, "p", (KT(64, "7,6", 0),), TILE)]),
    # exact f32 at 32 and 128 channels (the 32-channel bodies are also the safety net of 16- and 32-channel f16x3 networks)
    ((3, 3, 32, 1, 0), [(1, 0, 1, (KT(32, "7,6", 0), KT(32, "2,2", 0)), ALL), (1, 4, 1, (KT(32, "7,6", 0), KT(32, "4,4", 0)), TILE),
                        (1, 8, 1, (KT(32, "7,6", 0), KT(32, "5,5", 0)), TILE)]),
    ((3, 3, 128, 1, 0), [(1, 0, 1, (KT(128, "7,6", 0), KT(128, "2,2", 0)), ALL), (1, 4, 1, (KT(128, "7,6", 0), KT(128, "4,4", 0)), TILE),
                         (1, 7, 1, (KT(128, "7,6", 0), KT(128, "5,5", 0)), TILE)]),
    ((9, 9, 64, 1, 0), [(1, 0, 1, (KT(64, "7,6", 0), KT(64, "5,5", 0)), ALL), (1, 1, 1, (KT(64, "7,6", 0),), TILE)]),
    ((10, 10, 64, 1, 0), [(1, 0, 3, (KT(64, "4,4", 0),), ALL)]),      # NTT = 4, one sample per workgroup
    ((15, 7, 64, 1, 0), [(1, 0, 3, (KT(64, "4,4", 0),), TILE)]),      # the same at H != W, the largest board
]
CASES = [(g, c) for g, cs in GEOMETRIES for c in cs]


def _id(gc):
    (r, c, ch, nb, prec), (rounds, tcu, plus, bodies, probes) = gc
    return "%dx%d-%dch-prec%d-%dr+%dcu+%s-%s" % (r, c, ch, prec, rounds, tcu, plus, probes)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(geo):
    r, c, ch, nb, prec = geo
    return nn_plan.Plan(r, c, ch, 16, 8, prec, _cus())


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
    r, c, ch, nb, prec = geo
    torch.manual_seed(r * 131 + c * 17 + ch + nb)
    m = nn_ref.ResNetZeroRef(r, c, ch, nb)
    nn_ref.randomize_bn(m, 5)
    return m


@functools.lru_cache(maxsize=2)
def _inputs(geo):
    plan = _plan(geo)
    nmax = max(_n(plan, c) for g, c in CASES if g == geo)
    return nn_probe.positions(geo[0], geo[1], nmax, geo[0] * 7 + geo[1])


def _n_slots(geo):
    """the largest batch of any case on this board in this mode: the engine's size does not depend on the order of the tests"""
    return max(_n(_plan(g), c) for g, cs in GEOMETRIES for c in cs if (g[0], g[1], g[4]) == (geo[0], geo[1], geo[4]))


_engine = {}


def _engine_for(geo):
    """one engine at a time; the probes re-commit their weights on it (load_state_dict configures and commits anew)"""
    from dotsboxesaz_amd.engine import Engine
    key = (geo[0], geo[1], geo[4])
    if _engine.get("key") != key:
        _close_engine()
        n_slots = _n_slots(geo)
        _engine.update(key=key, e=Engine(geo[0], geo[1], n_slots, mcts_num_read=8, evaluator="resnet", nn_precision=geo[4]))
    return _engine["e"]


def _close_engine():
    if _engine.get("e") is not None:
        _engine["e"].close()
    _engine.clear()


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    _close_engine()


def _probes(ch, which, salt):
    if which == ALL:
        return nn_probe.probe_offsets(ch)
    # one probe per cout tile of 16 channels, at a different place of the tile from case to case
    return [t * 16 + 2 * ((salt + 3 * t) % 8) for t in range((ch + 15) // 16) if t * 16 + 2 * ((salt + 3 * t) % 8) + 2 <= ch]


def _compare_idx(plan, n, seed):
    idx = set(plan.workgroup_edges(n))
    idx.update(np.random.RandomState(seed).choice(n, min(32, n), replace=False).tolist())
    idx = sorted(idx)
    assert len(idx) <= MAX_COMPARED
    return idx


def _run_probes(e, m, X, ref, idx, c0s, expect_fallback=0):
    """{c0: (max |d log p| over the samples idx, the full p of the probe)}; ref is the Reference of X[idx]"""
    c = m.cfg
    out, v0 = {}, None
    for c0 in c0s:
        e.load_state_dict(nn_probe.probe_state_dict(m, c0, ref.s[c0]), "resnet", c["channels"], c["blocks"], c["head_channels"], c["value_fc"])
        p, v = e.predict(X)
        assert e.counters()["f32_fallback_evals"] == expect_fallback
        if v0 is None:
            v0 = v
        # the value head never changed -- but the two head convs share ONE power-of-two operand scale in f16x3 (pack_h3), so a
        # probe with another s may split the value head's weights into other (hi, lo) pairs: the same function in f32 grade
        assert np.abs(v - v0).max() < 1e-6
        pi = p[idx]
        assert np.isfinite(pi).all() and (pi > 0).all()
        out[c0] = (np.abs(nn_probe.log_of_p(pi) - ref.lp64(c0)), p)
    return out


@pytest.mark.parametrize("gc", CASES, ids=_id)
def test_tower_output_elementwise(gc):
    geo, case = gc
    bodies, which = case[3], case[4]
    plan = _plan(geo)
    n = _n(plan, case)
    launches = plan.launches(n)
    assert tuple(l.body for l in launches) == bodies, (n, launches)
    if case[2] == "p":
        assert len(launches) == 1 and launches[0].count % launches[0].S != 0
    m, X = _model(geo), _inputs(geo)[:n]
    idx = _compare_idx(plan, n, n)
    ref = nn_probe.Reference(m, X[idx])
    c0s = _probes(geo[2], which, n)
    e = _engine_for(geo)
    got = _run_probes(e, m, X, ref, idx, c0s)
    e32 = ref.e32(c0s)
    worst = max(c0s, key=lambda c0: got[c0][0].max())
    d = got[worst][0]
    e_hip = float(d.max())
    i, j = np.unravel_index(d.argmax(), d.shape)
    HW = plan.HW
    print("RATIO %-44s n %5d bodies %-60s E_hip %.2e E_32 %.2e ratio %5.2f (probe %d: sample %d, channel %d, position %d; %d samples, %d probes)"
          % (_id(gc), n, "+".join(bodies), e_hip, e32, e_hip / e32, worst, idx[i], worst + j // HW, j % HW, len(idx), len(c0s)))
    assert e_hip <= K[geo[4]] * e32, (e_hip, e32, worst, idx[i], j)


def test_f16x3_safety_net_elementwise():
    """Two samples whose plane 2 is 40000 leave f16's range, one in the two-cout-tile main launch, one in the <2,2> remainder.
    The groups the exact-f32 launch redoes meet the same bound; every other sample keeps the bits of a batch without them."""
    geo = (6, 6, 64, 2, 1)
    plan = _plan(geo)
    n = plan.round + 7
    assert tuple(l.body for l in plan.launches(n)) == (C2T, RR("2,2")) and plan.fallback_body() == KT(64, "7,6", 0)
    over = [7, plan.round + 3]
    redone = plan.redone(n, over)
    assert redone[:8] == list(range(4, 12)) and over[1] in redone and len(redone) == 12     # workgroup 5..9 -> two groups of 4
    m = _model(geo)
    X0 = _inputs(geo)[:n].copy()
    X = X0.copy()
    X[over, 2] = 40000.0
    ordinary = [i for i in redone if i not in over]
    idx = sorted(set(_compare_idx(plan, n, 1)) - set(over) | set(ordinary))
    ref = nn_probe.Reference(m, X[idx])
    c0s = _probes(64, TILE, 5)
    e = _engine_for(geo)
    clean = _run_probes(e, m, X0, ref, idx, c0s)
    got = _run_probes(e, m, X, ref, idx, c0s, expect_fallback=len(redone))
    e32 = ref.e32(c0s)
    keep = np.setdiff1d(np.arange(n), redone)
    pos = [idx.index(i) for i in ordinary]
    e_redone = 0.0
    for c0 in c0s:
        assert np.array_equal(got[c0][1][keep], clean[c0][1][keep])         # the neighbours: same bits
        e_redone = max(e_redone, float(got[c0][0][pos].max()))
        assert float(got[c0][0].max()) <= K[1] * e32
    # the overflowing samples themselves, under a scale that fits their (huge) tower output
    ref2 = nn_probe.Reference(m, X[over])
    got2 = _run_probes(e, m, X, ref2, over, c0s, expect_fallback=len(redone))
    e2, e32_2 = max(float(got2[c0][0].max()) for c0 in c0s), ref2.e32(c0s)
    print("RATIO safety net: redone neighbours E_hip %.2e E_32 %.2e ratio %.2f; overflowing samples E_hip %.2e E_32 %.2e ratio %.2f"
          % (e_redone, e32, e_redone / e32, e2, e32_2, e2 / e32_2))
    assert e_redone <= K[1] * e32
    assert e2 <= K[1] * e32_2
