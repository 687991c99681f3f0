"""HIP policy/value network (MFMA conv tower + heads) through the C ABI vs the
reference's golden outputs and the torch fp32 restatement -- rows N1, N3.
Tolerance: 1e-4 absolute on policy and value (north-star, fp32)."""
import numpy as np
import pytest
import torch

from oracle import nn_ref

pytestmark = pytest.mark.gpu
TOL = 1e-4


def engine_for(rows, cols, model, n_slots=64, precision=0):
    from dotsboxesaz_amd.engine import Engine
    e = Engine(rows, cols, n_slots, mcts_num_read=8, evaluator="resnet", nn_precision=precision)
    c = model.cfg
    e.load_state_dict(model.state_dict(), "resnet", c["channels"], c["blocks"], c["head_channels"], c["value_fc"])
    return e


# precision 0 = exact f32 MFMA; 1 = f16x3, the mode bench.py times and the drop-in entry points default to: BOTH are compared with
# the reference's own (p, v) (NeuralNetWrapper.predict_sync, nn.py:155-160, recorded in tests/golden/nn.npz)
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("tag", ["small33", "small66", "small23", "groups33", "groups23"])
def test_golden_committed_weights(golden_nn, tag, precision):
    """groups33 / groups23: networks with the reference's n_groups option (grouped convs, nn.py:33-47,61-71); the engine expands
    their [C][C/g][3][3] weights to the dense block-diagonal form when they are loaded."""
    g = golden_nn
    cfg = [int(x) for x in g[tag + "_cfg"]]
    r, c, ch, nb, hc, vf = cfg[:6]
    m = nn_ref.ResNetZeroRef(r, c, ch, nb, 3, hc, vf, n_groups=cfg[6] if len(cfg) > 6 else 1)
    m.load_state_dict({k[len(tag) + 3:]: torch.tensor(g[k]) for k in g.files if k.startswith(tag + "_w_")})
    e = engine_for(r, c, m, precision=precision)
    assert e.cfg.nn_precision == precision
    p, v = e.predict(g[tag + "_X"])
    assert e.counters()["f32_fallback_evals"] == 0
    assert p.shape == g[tag + "_p"].shape and v.shape == g[tag + "_v"].shape
    assert np.abs(p - g[tag + "_p"]).max() < TOL
    assert np.abs(v - g[tag + "_v"]).max() < TOL
    e.close()


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("tag,rows,cols", [("full33", 3, 3), ("full66", 6, 6), ("full99", 9, 9)])
def test_golden_full_size(golden_nn, tag, rows, cols, precision):
    """20 blocks x 64 channels, weights regenerated from the fixture's seed; both arithmetic modes against the reference's outputs."""
    g = golden_nn
    torch.manual_seed(0)
    m = nn_ref.ResNetZeroRef(rows, cols)
    nn_ref.randomize_bn(m, 3)
    e = engine_for(rows, cols, m, precision=precision)
    p, v = e.predict(g[tag + "_X"])
    assert e.counters()["f32_fallback_evals"] == 0  # the f16x3 figures are f16x3 figures, not the safety net's
    e.close()
    # always: against the torch fp32 restatement with the very same weights
    pr, vr = nn_ref.predict_sync(m, g[tag + "_X"])
    assert np.abs(p - pr).max() < TOL and np.abs(v - vr).max() < TOL
    # the reference's own outputs: the fixture holds them for the weights ITS run drew from the seed (6 MB of
    # weights are not committed); a torch build with another RNG stream cannot regenerate them -- say so, loudly
    cs = nn_ref.state_dict_checksum(m)
    if abs(cs - float(g[tag + "_checksum"])) > 1e-6 * cs:
        pytest.skip("seed-regenerated weights differ from the fixture's (checksum %r vs %r): golden comparison of %s "
                    "not possible with this torch build; the torch-restatement comparison above passed"
                    % (cs, float(g[tag + "_checksum"]), tag))
    assert np.abs(p - g[tag + "_p"]).max() < TOL
    assert np.abs(v - g[tag + "_v"]).max() < TOL


@pytest.mark.parametrize("rows,cols,ch,nb,n", [(6, 6, 64, 3, 1), (6, 6, 64, 3, 3), (6, 6, 64, 3, 4), (6, 6, 64, 3, 5),
                                               (6, 6, 64, 3, 333), (3, 3, 64, 2, 257), (9, 9, 64, 2, 77),
                                               (4, 2, 32, 2, 50), (6, 6, 128, 1, 19), (1, 1, 16, 1, 9),
                                               (10, 10, 64, 2, 21), (15, 7, 64, 2, 9)])  # the last two: largest boards
def test_ragged_batches_vs_torch(rows, cols, ch, nb, n):
    """Batch sizes around the samples-per-workgroup boundary; arbitrary float inputs."""
    torch.manual_seed(rows * 31 + cols + ch + n)
    m = nn_ref.ResNetZeroRef(rows, cols, ch, nb)
    nn_ref.randomize_bn(m, 5)
    e = engine_for(rows, cols, m, n_slots=128)
    X = torch.randn(n, 3, rows + 1, cols + 1).numpy()
    p, v = e.predict(X)
    pr, vr = nn_ref.predict_sync(m, X)
    assert np.abs(p - pr).max() < TOL, np.abs(p - pr).max()
    assert np.abs(v - vr).max() < TOL, np.abs(v - vr).max()
    assert np.allclose(p.sum(1), 1.0, atol=1e-5)
    e.close()


def test_results_independent_of_batch_composition():
    """Leaf-eval cache contract (utils/proxies.py:35-43): a sample's (p, v) must not
    depend on what else is in the batch -- bit-identical alone and inside a large batch."""
    torch.manual_seed(1)
    m = nn_ref.ResNetZeroRef(6, 6, 64, 4)
    nn_ref.randomize_bn(m, 5)
    e = engine_for(6, 6, m, n_slots=256)
    X = torch.randn(200, 3, 7, 7).numpy()
    p, v = e.predict(X)
    for i in (0, 3, 4, 77, 199):
        pi, vi = e.predict(X[i:i + 1])
        assert np.array_equal(pi[0], p[i]) and np.array_equal(vi[0], v[i])
    perm = np.random.RandomState(0).permutation(200)
    p2, v2 = e.predict(X[perm])
    assert np.array_equal(p2, p[perm]) and np.array_equal(v2, v[perm])
    e.close()


def test_predict_before_commit_is_an_error():
    from dotsboxesaz_amd import _lib
    from dotsboxesaz_amd.engine import Engine
    e = Engine(3, 3, 4, evaluator="resnet")
    with pytest.raises(_lib.DbazError):
        e.predict(np.zeros((1, 3, 4, 4), np.float32))
    with pytest.raises(_lib.DbazError):
        e.load_state_dict({"bn_input.weight": np.ones(3, np.float32)}, "resnet", 16, 1, 4, 8)  # incomplete
    e.close()


@pytest.mark.parametrize("rows,cols,ch,nb,n", [(6, 6, 64, 20, 64), (3, 3, 64, 20, 40), (9, 9, 64, 20, 10), (6, 6, 64, 3, 5),
                                               (4, 2, 32, 2, 50), (6, 6, 128, 2, 19), (2, 3, 8, 1, 12), (6, 6, 64, 2, 1500),
                                               (5, 3, 64, 2, 700)])
def test_f16x3_split_precision_mode(rows, cols, ch, nb, n, precision=1):
    """nn_precision=1: every f32 operand is an error-compensated (hi, lo) pair of halves on the
    f16 MFMA pipe with f32 accumulation.  Same 1e-4 north-star tolerance; the observed error is
    of the order of f32 rounding noise (asserted < 2e-5)."""
    torch.manual_seed(rows * 31 + cols + ch + n)
    m = nn_ref.ResNetZeroRef(rows, cols, ch, nb)
    nn_ref.randomize_bn(m, 5)
    e = engine_for(rows, cols, m, n_slots=max(128, n), precision=precision)
    e0 = engine_for(rows, cols, m, n_slots=max(128, n), precision=0)
    rng = np.random.RandomState(n)
    X = rng.randint(0, 2, size=(n, 3, rows + 1, cols + 1)).astype(np.float32)
    X[:, 2] = rng.randint(-2, rows * cols + 1, size=(n, 1, 1))
    p, v = e.predict(X)
    p0, v0 = e0.predict(X)
    pr, vr = nn_ref.predict_sync(m, X)
    err = max(np.abs(p - pr).max(), np.abs(v - vr).max())
    err0 = max(np.abs(p0 - pr).max(), np.abs(v0 - vr).max())
    print("f16x3 max abs err %.3g (exact-f32 MFMA path: %.3g)" % (err, err0))
    assert err < 2e-5, err
    if (rows, cols, ch) == (6, 6, 64) and n >= 1280:
        # the first 1 280 samples went through the main launch (two cout tiles per wave, 5 samples per workgroup), a batch of 7
        # goes through the remainder launch (one cout tile per wave): the two tilings accumulate in the same order -- bit-identical
        p7, v7 = e.predict(X[:7])
        assert np.array_equal(p7, p[:7]) and np.array_equal(v7, v[:7])
    assert np.allclose(p.sum(1), 1.0, atol=1e-5)
    e.close()
    e0.close()


@pytest.mark.parametrize("rows,cols,ch,precision,c2,perm,use_rem", [
    (3, 3, 64, 1, 1, True, 1),      # two-cout-tile main body with the row table
    (6, 5, 64, 1, 0, False, 1),     # two-cout-tile body rejected by the fill rule
    (2, 2, 32, 0, 0, False, 0)])    # exact f32: no remainder kernel, <2,2> / <4,4> / <5,5> launches of their own
def test_commit_twice_gives_the_same_network(rows, cols, ch, precision, c2, perm, use_rem):
    """dbaz_nn_commit again on the same handle, without dbaz_nn_configure: the plan (csrc/tower_plan.h) starts from the network's
    shape alone, not from what the last commit left, so the same launches evaluate the batch -- one full round of the main launch
    and the first tail body -- and (p, v) are the same bytes."""
    from oracle import nn_plan
    m = nn_ref.ResNetZeroRef(rows, cols, ch, 2)
    plan = nn_plan.Plan(rows, cols, ch, m.cfg["head_channels"], m.cfg["value_fc"], precision,
                        torch.cuda.get_device_properties(0).multi_processor_count)
    assert (plan.c2, plan.perm, plan.use_rem) == (c2, perm, use_rem)
    tails = plan.tail_bodies()
    n = plan.n_for(tails[0][1], 1) if tails else plan.round + 1
    assert len(plan.launches(n)) == 2
    torch.manual_seed(rows * 31 + cols + ch)
    nn_ref.randomize_bn(m, 5)
    e = engine_for(rows, cols, m, n_slots=n, precision=precision)
    X = _positions(rows, cols, n, 5)
    p, v = e.predict(X)
    e._ck(e._L.dbaz_nn_commit(e.h))
    p2, v2 = e.predict(X)
    e.close()
    assert np.isfinite(p).all() and np.abs(p.sum(1) - 1.0).max() < 1e-5
    assert p.tobytes() == p2.tobytes() and v.tobytes() == v2.tobytes()


def _scaled_block_net(K):
    """ResNetZero whose FUNCTION is that of an ordinary random-init net, but whose activations between conv1 and
    conv2 of block 1 are K times larger (bn1 scaled by K, conv2's weights by 1/K; ReLU is positively homogeneous)."""
    torch.manual_seed(4)
    m = nn_ref.ResNetZeroRef(6, 6, 64, 3)
    nn_ref.randomize_bn(m, 2)
    with torch.no_grad():
        blk = m.resnet.resblocks[1]
        blk.bn1.weight.mul_(K)
        blk.bn1.bias.mul_(K)
        blk.conv2.weight.div_(K)
    return m


def test_f16x3_range_overflow_falls_back_to_exact_f32():
    """f16x3 safety net: activations beyond f16's range (here ~4096 x the usual ones inside one block) must not
    produce garbage or stop play -- the affected evaluations are redone by the exact-f32 tower on the device, in the
    same step, and (p, v) stay within the 1e-4 tolerance of the torch fp32 restatement."""
    m = _scaled_block_net(4096.0)
    e = engine_for(6, 6, m, n_slots=64, precision=1)
    rng = np.random.RandomState(3)
    X = rng.randint(0, 2, size=(37, 3, 7, 7)).astype(np.float32)
    X[:, 2] = rng.randint(0, 37, size=(37, 1, 1))
    p, v = e.predict(X)
    pr, vr = nn_ref.predict_sync(m, X)
    assert np.isfinite(p).all() and np.abs(p - pr).max() < TOL and np.abs(v - vr).max() < TOL
    c = e.counters()
    assert 37 <= c["f32_fallback_evals"] <= 40  # every sample (in whole workgroups)
    e.close()
    # play continues: complete self-play games with this network, fallbacks counted, no error
    from dotsboxesaz_amd.engine import Engine
    e = Engine(6, 6, 8, mcts_num_read=12, noise=(0.8, 0.25), evaluator="resnet", nn_precision=1, seed=2)
    e.load_state_dict(m.state_dict(), "resnet", 64, 3, 16, 8)
    e.selfplay_start(8, 0)
    e.run()
    c = e.counters()
    assert c["games_finished"] == 8 and c["error_slots"] == 0 and c["f32_fallback_evals"] >= c["nn_evals"] > 0
    e.close()


def test_f16x3_fallback_only_touches_the_overflowing_samples():
    """Inputs are what overflows here (two samples with a huge plane-2 value): only their workgroups are redone in
    f32; an ordinary network, every output within tolerance, ordinary batches afterwards cost no fallback."""
    torch.manual_seed(9)
    m = nn_ref.ResNetZeroRef(6, 6, 64, 3)
    nn_ref.randomize_bn(m, 2)
    e = engine_for(6, 6, m, n_slots=2048, precision=1)
    rng = np.random.RandomState(5)
    n = 1500  # > 1024: the main launch (4 samples per workgroup) and a tail launch both run
    X = rng.randint(0, 2, size=(n, 3, 7, 7)).astype(np.float32)
    X[:, 2] = rng.randint(0, 37, size=(n, 1, 1))
    X[5, 2] = 40000.0
    X[1444, 2] = -35000.0
    p, v = e.predict(X)
    pr, vr = nn_ref.predict_sync(m, X)
    assert np.abs(p - pr).max() < TOL and np.abs(v - vr).max() < TOL
    c = e.counters()
    assert 2 <= c["f32_fallback_evals"] <= 20  # whole workgroups: the flagged 5-sample groups, redone in 4-sample groups
    e.predict(X[100:400])
    assert e.counters()["f32_fallback_evals"] == c["f32_fallback_evals"]
    e.close()


def test_no_fallback_debug_flag_is_rejected():
    """debug_flags bit 2 (DBAZ_DBG_NO_FALLBACK) used to skip the exact-f32 safety net, so overflowing f16x3 evaluations came
    back as success; the bit stays reserved and dbaz_create rejects it."""
    from dotsboxesaz_amd import _lib
    from dotsboxesaz_amd.engine import Engine
    with pytest.raises(_lib.DbazError) as ei:
        Engine(6, 6, 8, evaluator="resnet", debug_flags=2)
    assert ei.value.code == _lib.EINVAL and "DBAZ_DBG_NO_FALLBACK" in str(ei.value)


def test_f16x3_simplenn_still_reports_range_overflow():
    """SimpleNN has no f32 safety net: out-of-range activations remain a loud error."""
    from dotsboxesaz_amd import _lib
    torch.manual_seed(0)
    m = nn_ref.SimpleNNRef()
    with torch.no_grad():
        m.conv0.weight.mul_(1e5)
    e = simple_engine(m, 1, n_slots=8)
    with pytest.raises(_lib.DbazError):
        e.predict(np.ones((2, 3, 4, 4), np.float32))
    e.close()


# ---------------------------------------------------------------- SimpleNN (row N2)
def simple_engine(model, precision, n_slots=64):
    from dotsboxesaz_amd.engine import Engine
    e = Engine(3, 3, n_slots, mcts_num_read=8, evaluator="simplenn", nn_precision=precision)
    e.load_state_dict(model.state_dict(), "simplenn")
    return e


@pytest.mark.parametrize("precision", [0, 1])
def test_simplenn_golden_and_torch(golden_nn, precision):
    """dots_boxes_nn.SimpleNN (BN after ReLU, unpadded conv4, BatchNorm1d FCs) vs the reference's
    golden outputs (seed-regenerated weights) and the torch restatement."""
    g = golden_nn
    torch.manual_seed(0)
    m = nn_ref.SimpleNNRef()
    nn_ref.randomize_bn(m, 3)
    e = simple_engine(m, precision)
    pg, vg = e.predict(g["simple_X"])
    rng = np.random.RandomState(1)
    X = rng.randint(0, 2, size=(77, 3, 4, 4)).astype(np.float32)
    X[:, 2] = rng.randint(-1, 10, size=(77, 1, 1))
    p, v = e.predict(X)
    pr, vr = nn_ref.predict_sync(m, X)
    err = max(np.abs(p - pr).max(), np.abs(v - vr).max())
    print("SimpleNN precision %d max abs err %.3g" % (precision, err))
    assert err < 2e-5 and p.shape == (77, 32) and v.shape == (77, 1)
    p1, v1 = e.predict(X[5:6])
    assert np.array_equal(p1[0], p[5]) and np.array_equal(v1[0], v[5])
    e.close()
    cs = nn_ref.state_dict_checksum(m)
    if abs(cs - float(g["simple_checksum"])) > 1e-6 * cs:  # see test_golden_full_size
        pytest.skip("seed-regenerated SimpleNN weights differ from the fixture's (checksum %r vs %r): golden comparison "
                    "not possible with this torch build; the torch-restatement comparison passed" % (cs, float(g["simple_checksum"])))
    assert np.abs(pg - g["simple_p"]).max() < TOL and np.abs(vg - g["simple_v"]).max() < TOL


def test_simplenn_rejects_other_boards_and_plays():
    from dotsboxesaz_amd import _lib
    from dotsboxesaz_amd.engine import Engine
    from dotsboxesaz_amd import nn as dnn
    e = Engine(6, 6, 4, evaluator="simplenn")
    with pytest.raises(_lib.DbazError):
        e.load_state_dict({}, "simplenn")
    e.close()
    torch.manual_seed(1)
    model = dnn.SimpleNN()
    ref = nn_ref.SimpleNNRef()
    ref.load_state_dict(model.state_dict(), strict=True)  # reference key names
    e = Engine(3, 3, 16, mcts_num_read=20, noise=(0.8, 0.25), evaluator="simplenn", seed=2)
    e.load_state_dict(model.state_dict(), "simplenn")
    e.selfplay_start(16, 0)
    e.run()
    c = e.counters()
    got = e.fetch_samples()
    assert c["games_finished"] == 16 and c["error_slots"] == 0 and len(got["z"]) >= 16 * 9
    e.close()


def _positions(rows, cols, n, seed):
    """Feature planes of the kind get_features produces: 0/1 edge planes, constant plane 2 = 2 * boxes_to_close[to_play] as int8."""
    rng = np.random.RandomState(seed)
    X = (rng.rand(n, 3, rows + 1, cols + 1) < rng.rand(n, 1, 1, 1)).astype(np.float32)   # from empty to full boards
    X[:, 2] = rng.randint(-1, rows * cols + 1, size=(n, 1, 1))
    return X


@pytest.mark.parametrize("rows,cols,n", [(3, 3, 600), (9, 9, 300), (4, 2, 400)])
def test_f16x3_on_trained_like_statistics_other_boards(rows, cols, n):
    """The same trained-like statistics on the other BASELINE board sizes (3x3: the remainder bodies of the two-cout-tile geometry;
    9x9: the 7-tile one-cout-tile kernel with the LDS-decoded residual; 4x2: a non-square board), 20 x 64: f16x3 within 1e-4 of
    torch fp32 (observed ~1e-6), no exact-f32 fallback."""
    torch.manual_seed(rows * 10 + cols)
    m = nn_ref.ResNetZeroRef(rows, cols, 64, 20)
    maxima = nn_ref.trained_like_(m, _positions(rows, cols, 192, 3), 11)
    X = _positions(rows, cols, n, 4)
    pr, vr = nn_ref.predict_sync(m, X)
    e = engine_for(rows, cols, m, n_slots=max(64, n), precision=1)
    p, v = e.predict(X)
    c = e.counters()
    e.close()
    err = max(np.abs(p - pr).max(), np.abs(v - vr).max())
    print("trained-like %dx%d 20x64 (activations up to %.0f): f16x3 vs torch fp32 %.2e, fallback %d of %d" % (rows, cols, max(maxima), err, c["f32_fallback_evals"], n))
    assert err <= 1e-4 and c["f32_fallback_evals"] == 0


@pytest.mark.parametrize("seed", [7, 8])
def test_f16x3_on_trained_like_statistics_20x64(seed):
    """The mode bench.py times, on weights with the statistics of a TRAINED network instead of a fresh one:
    6x6, 20 blocks x 64 channels; per layer the BatchNorm variances spread over 3 decades (running statistics fitted to what the
    layer really sees, as training does), gamma over 3 decades -- the folded per-channel weight scale over ~3.7 decades --, means a
    couple of sigma off, and the residual stream grown over 20 blocks to |activation| ~ 150.  f16x3 must stay within the 1e-4
    north-star tolerance of torch fp32 WITHOUT leaning on the exact-f32 safety net: f32_fallback_evals / nn_evals is asserted 0."""
    torch.manual_seed(seed)
    m = nn_ref.ResNetZeroRef(6, 6, 64, 20)
    maxima = nn_ref.trained_like_(m, _positions(6, 6, 256, seed), seed)
    for name, bn in (("first", m.resnet.resblocks[0].bn1), ("last", m.resnet.resblocks[19].bn2)):
        sc = (bn.weight / (bn.running_var + 1e-5).sqrt()).abs().detach()
        assert float(sc.max() / sc.min()) > 1e3 and float(bn.running_var.max() / bn.running_var.min()) > 5e2, name
    assert max(maxima) > 50.0                                   # the stream did grow
    n = 1500
    X = _positions(6, 6, n, seed + 100)
    pr, vr = nn_ref.predict_sync(m, X)
    m64 = nn_ref.ResNetZeroRef(6, 6, 64, 20).double()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    m64.train(False)
    with torch.no_grad():
        lp64, v64 = m64(torch.tensor(X, dtype=torch.float64))
    p64, v64 = torch.exp(lp64).numpy(), v64.numpy()
    res = {}
    for prec in (0, 1):
        e = engine_for(6, 6, m, n_slots=2048, precision=prec)
        p, v = e.predict(X)
        c = e.counters()
        e.close()
        res[prec] = (max(np.abs(p - pr).max(), np.abs(v - vr).max()), max(np.abs(p - p64).max(), np.abs(v - v64).max()), c["f32_fallback_evals"])
    t64 = max(np.abs(pr - p64).max(), np.abs(vr - v64).max())
    print("trained-like 20x64 (activations up to %.0f): max |d(p, v)| vs torch fp32 / vs float64 -- f16x3 %.2e / %.2e, exact-f32 MFMA "
          "%.2e / %.2e, torch fp32 itself vs float64 %.2e; f32_fallback_evals %d of %d"
          % (max(maxima), res[1][0], res[1][1], res[0][0], res[0][1], t64, res[1][2], n))
    assert res[1][2] == 0                                       # fallback fraction 0 / 1500
    assert res[1][0] <= 1e-4 and res[0][0] <= 1e-4
    assert res[1][1] <= max(4 * t64, 2e-5)                      # as close to the float64 truth as a float32 evaluation is


@pytest.mark.parametrize("precision", [0, 1])
def test_whole_network_in_logit_space_vs_float64(precision):
    """The whole network -- tower, both heads, softmax and tanh -- where an error is not squeezed by the softmax or the tanh:
    log p and atanh v against float64, bounded by K times what torch's own float32 evaluation leaves (the criterion and the K of
    tests/test_hip_nn_elementwise.py; this covers the value head, which the probe head of that file does not).  6x6, 20 x 64,
    trained-like statistics, 300 positions: the <4,4> remainder in f16x3, the <2,2> one in exact f32 at 256 compute units.
    Compared: log p where p >= 1e-30 (f32 softmax outputs keep their relative precision down to 1.2e-38; log_softmax of torch
    has no such floor) and atanh v where |v| <= 0.99 (beyond, one f32 spacing of v, 6e-8, times atanh' = 1 / (1 - v^2) > 50
    exceeds the 1e-6 scale that is measured)."""
    from oracle import nn_probe
    torch.manual_seed(7)
    m = nn_ref.ResNetZeroRef(6, 6, 64, 20)
    nn_ref.trained_like_(m, _positions(6, 6, 256, 7), 7)
    n = 300
    X = _positions(6, 6, n, 107)
    m64 = nn_ref.ResNetZeroRef(6, 6, 64, 20).double()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    m64.train(False)
    m.train(False)
    with torch.no_grad():
        lp64, v64 = [t.numpy() for t in m64(torch.tensor(X, dtype=torch.float64))]
        lp32, v32 = [t.numpy().astype(np.float64) for t in m(torch.tensor(X))]
    e = engine_for(6, 6, m, n_slots=512, precision=precision)
    p, v = e.predict(X)
    c = e.counters()
    e.close()
    assert c["f32_fallback_evals"] == 0
    mp, mv = np.exp(lp64) >= 1e-30, np.abs(v64) <= 0.99
    assert mp.mean() > 0.9 and mv.mean() > 0.5, (mp.mean(), mv.mean())
    assert (p[mp] > 0).all() and (np.abs(v[mv]) < 1).all()
    with np.errstate(divide="ignore"):
        lp = np.log(p.astype(np.float64))
    e_p, e32_p = np.abs(lp - lp64)[mp].max(), np.abs(lp32 - lp64)[mp].max()
    e_v, e32_v = np.abs(np.arctanh(v.astype(np.float64)) - np.arctanh(v64))[mv].max(), np.abs(np.arctanh(v32) - np.arctanh(v64))[mv].max()
    print("RATIO whole network 6x6 20x64 trained-like, nn_precision %d: log p E_hip %.2e E_32 %.2e ratio %.2f; atanh v E_hip %.2e E_32 %.2e "
          "ratio %.2f (%.1f %% of the logits, %.1f %% of the values compared)"
          % (precision, e_p, e32_p, e_p / e32_p, e_v, e32_v, e_v / e32_v, 100 * mp.mean(), 100 * mv.mean()))
    assert e_p <= nn_probe.K[precision] * e32_p, (e_p, e32_p)
    assert e_v <= nn_probe.K[precision] * e32_v, (e_v, e32_v)


def test_f16x3_after_three_generations_of_training(tmp_path):
    """A checkpoint that really was TRAINED: three generations of the generation loop (self-play on the engine in f16x3 -> replay in
    HBM -> optimizer steps -> weights back into the engine) at 6x6 with the 20 x 64 network, then the engine's f16x3 (p, v) for the
    positions of the last generation's own games against torch fp32 of the checkpoint; the exact-f32 safety net must have redone
    nothing in any generation (printed: f32_fallback_evals / nn_evals)."""
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd import train as T
    from dotsboxesaz_amd.coach import Coach
    from dotsboxesaz_amd.self_play import unpack_rows
    params = dnn.resnet_params(6, 6, 64, 20)
    params["nn"]["model_class"] = dnn.ResNetZero
    params["nn"]["chkpts_filename"] = str(tmp_path / "model_gen{}.pt")
    params["nn"]["train_params"] = {"nb_epochs": 4, "train_batch_size": 1024, "val_batch_size": 1024, "lr": 2e-2,
                                    "lr_scheduler": T.GenerationLrScheduler({0: 2e-2}), "optimizer_params": {"momentum": 0.9, "weight_decay": 1e-4},
                                    "pos_average": True, "train_split": 0.9, "max_samples_per_gen": 10 ** 9, "symmetries": None}
    params["self_play"] = {"num_games": 384, "reuse_mcts_tree": True, "noise": (0.8, 0.25),
                           "mcts": {"mcts_num_read": 64, "mcts_cpuct": (1.25, 19652), "temperature": {0: 1.0, 12: 0.02}}}
    params["elo"] = None
    torch.manual_seed(0)
    np.random.seed(0)
    coach = Coach(params, 6, 6, n_slots=384)
    assert coach.nn_precision == 1
    evals = fallback = steps = 0
    for g in range(4):                       # generation 0 trains nothing (min(2g, nb_epochs) epochs); 1, 2, 3 do
        sp = coach.selfplay(g)
        evals += sp["nn_evals"]
        fallback += sp["f32_fallback_evals"]
        steps = coach.train_nn(g, None)
    assert steps >= 40, steps
    ck = torch.load(params["nn"]["chkpts_filename"].format(3), map_location="cpu", weights_only=True)
    ref = nn_ref.ResNetZeroRef(6, 6, 64, 20)
    ref.load_state_dict(ck["model_dict"], strict=True)
    rows = coach.store.chunks[-1]["rows"]
    s = unpack_rows(rows[:3000].cpu().numpy(), coach.engine.F, coach.engine.A)
    X = s["x"].reshape(-1, 3, 7, 7).astype(np.float32)
    assert coach.engine.cfg.nn_precision == 1
    p, v = coach.engine.predict(X)           # the engine holds generation 3's weights (train_nn pushed them back)
    c = coach.engine.counters()
    pr, vr = nn_ref.predict_sync(ref, X)
    err = max(np.abs(p - pr).max(), np.abs(v - vr).max())
    print("after 3 trained generations (%d optimizer steps): f16x3 vs torch fp32 max |d(p, v)| %.2e on %d positions of the last games; "
          "f32_fallback_evals / nn_evals over the four self-play runs = %d / %d; policy max %.2f"
          % (steps, err, len(X), fallback + c["f32_fallback_evals"], evals, float(p.max())))
    coach.close()
    assert err <= 1e-4 and fallback == 0 and c["f32_fallback_evals"] == 0
