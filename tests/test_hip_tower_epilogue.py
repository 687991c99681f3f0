"""The layer epilogue of the two-cout-tile tower body (conv_lds_h3_c2, csrc/nn.hip) and of the remainder bodies beside it.

The epilogue's bias is loaded INSIDE the K-loop (two steps before the last MFMA on the deep ring), where a wave still works on
the layer before; and the residual add is one of two straight code streams picked by a wave-uniform branch on the layer's parity.
What can go wrong: a layer runs with the bias of its neighbour, the wrong stream is taken, or the register residual is lost where
it crosses a block.

Cases: 6x6 (row table, 4 tiles per wave pair) and 7x7 (natural order, 3 tiles), 64 channels, heads 16 / 8; one block (one layer
of each kind) and two (the register residual crosses a block; layer l + 1's bias must not be layer l's).  n is one full round of
the main body plus a tail, as in test_hip_tower_ring.py.

(a) the main body gives the bits of the single-sample remainder body (which loads its bias in its own K-loop, per cout tile).
(b) the BatchNorm shift of ONE channel of the last cout tile of ONE layer is set to a large value of its own, in turn in the first
    and in the last layer.  The CHANGE of (log p, v) that the engine shows must follow the change torch float64 shows, under the
    tower criterion of test_hip_nn_elementwise.py:  E_hip = max |D_hip - D_64|  <=  K * E_32,  E_32 = max |D_32 - D_64| of torch's
    own float32, K = 8.  An epilogue that takes another layer's bias moves the shift to another layer and D with it.
The CPU test shows that (b) has teeth: torch float32 with the shifts of two neighbouring layers swapped fails it."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import nn_plan, nn_probe, nn_ref

K = nn_probe.K[1]

# (rows, cols, samples per workgroup, tiles per wave pair, row table)
GEOMETRIES = [(6, 6, 5, 4, True), (7, 7, 3, 3, False)]
HC, VFC = 16, 8
# (channel of the last cout tile, shift) for the first and for the last layer: far from randomize_bn's N(0, 0.1) and from each other
SHIFTS = {"first": (61, 2.5), "last": (50, 4.0)}


def _model(rows, cols, blocks):
    torch.manual_seed(rows * 131 + cols * 17 + blocks * 5 + HC)
    m = nn_ref.ResNetZeroRef(rows, cols, 64, blocks, head_channels=HC, value_fc=VFC)
    return nn_ref.randomize_bn(m, 7)


def _layer_bn(m, layer):
    blk = m.resnet.resblocks[layer // 2]
    return blk.bn2 if layer & 1 else blk.bn1


def _shifted(m, which):
    """a copy of m with one BatchNorm shift replaced: `which` = "first" | "last" layer of the tower"""
    layer = 0 if which == "first" else 2 * m.cfg["blocks"] - 1
    ch, val = SHIFTS[which]
    m2 = copy.deepcopy(m)
    with torch.no_grad():
        _layer_bn(m2, layer).bias[ch] = val
    return m2


def _swapped(m, layer):
    """a copy of m in which layers `layer` and `layer + 1` use each other's BatchNorm shift (what an epilogue would compute that
    holds its neighbour's bias)"""
    m2 = copy.deepcopy(m)
    a, b = _layer_bn(m2, layer), _layer_bn(m2, layer + 1)
    with torch.no_grad():
        t = a.bias.clone()
        a.bias.copy_(b.bias)
        b.bias.copy_(t)
    return m2


def _torch_out(m, X, dtype):
    """(log p, v) of torch's own evaluation in dtype, as float64 [n, A + 1]"""
    mm = copy.deepcopy(m).to(dtype)
    mm.train(False)
    with torch.no_grad():
        lp, v = mm(torch.as_tensor(X, dtype=dtype))
    return np.concatenate([lp.double().numpy(), v.double().numpy().reshape(len(X), 1)], axis=1)


def _criterion(d_test, d_64, d_32):
    """(E_test, E_32) of a change of (log p, v)"""
    return float(np.abs(d_test - d_64).max()), float(np.abs(d_32 - d_64).max())


# ------------------------------------------------------------------ CPU: the criterion of (b) has teeth
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("which", ["first", "last"])
def test_swapped_shifts_fail_the_criterion(which, blocks):
    rows = cols = 6
    m = _model(rows, cols, blocks)
    m2 = _shifted(m, which)
    X = torch.randn(12, 3, rows + 1, cols + 1, generator=torch.Generator().manual_seed(3)).numpy()
    d_64 = _torch_out(m2, X, torch.float64) - _torch_out(m, X, torch.float64)
    d_32 = _torch_out(m2, X, torch.float32) - _torch_out(m, X, torch.float32)
    assert np.abs(d_64).max() > 1e-2, "the shift must move the outputs far above float32 noise"
    for layer in range(2 * blocks - 1):
        d_mut = _torch_out(_swapped(m2, layer), X, torch.float32) - _torch_out(_swapped(m, layer), X, torch.float32)
        e_mut, e_32 = _criterion(d_mut, d_64, d_32)
        touched = layer in ((0,) if which == "first" else (2 * blocks - 2,))
        print("swap %d/%d, shift in the %s layer: E_mut %.2e E_32 %.2e ratio %.1f" % (layer, layer + 1, which, e_mut, e_32, e_mut / e_32))
        if touched:  # the swap moves the large shift into the neighbouring layer
            assert e_mut > 4 * K * e_32, (e_mut, e_32)
    # and torch float32 itself passes, trivially: the yardstick is its own distance
    assert _criterion(d_32, d_64, d_32)[0] <= K * _criterion(d_32, d_64, d_32)[1]


# ------------------------------------------------------------------ GPU
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _big_n():
    return 2 * _cus() * 16 + 7  # at least one full round for any S <= 16


def _engine(rows, cols, model, n_slots):
    from dotsboxesaz_amd.engine import Engine
    e = Engine(rows, cols, n_slots, mcts_num_read=8, evaluator="resnet", nn_precision=1)
    c = model.cfg
    e.load_state_dict(model.state_dict(), "resnet", c["channels"], c["blocks"], c["head_channels"], c["value_fc"])
    return e


@functools.lru_cache(maxsize=None)
def _inputs(rows, cols):
    return torch.randn(_big_n(), 3, rows + 1, cols + 1, generator=torch.Generator().manual_seed(rows * 7 + cols)).numpy()


@functools.lru_cache(maxsize=None)
def _run(rows, cols, blocks, which=None):
    """(model, p, v) of the whole batch in one predict call; which: None | "first" | "last" (the shifted model)"""
    m = _model(rows, cols, blocks)
    if which is not None:
        m = _shifted(m, which)
    e = _engine(rows, cols, m, _big_n())
    p, v = e.predict(_inputs(rows, cols))  # raises if an activation left f16's range
    assert e.counters()["f32_fallback_evals"] == 0
    e.close()
    return m, p, v


def _compared(plan, S):
    """test_hip_tower_ring.py's choice: first, three in between and last workgroup of the full rounds, and the tail"""
    n = _big_n()
    mode, n_full = plan.split(n)
    assert plan.round <= n_full < n, (mode, n_full)
    wgs = n_full // S
    idx = []
    for wg in (0, wgs // 4, wgs // 2 + 1, (3 * wgs) // 4 + 2, wgs - 1):
        idx += [wg * S, wg * S + S // 2, wg * S + S - 1]
    idx += [n_full, n - 2, n - 1]
    idx = sorted(set(i for i in idx if 0 <= i < n))
    assert len(idx) >= 15
    return idx


def _plan(rows, cols, S, ntt, table):
    plan = nn_plan.Plan(rows, cols, 64, HC, VFC, 1, _cus())
    assert plan.c2 and (plan.S_c2, plan.NT_c2, plan.perm) == (S, ntt, table), plan.main_body()
    return plan


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("rows,cols,S,ntt,table", GEOMETRIES)
def test_main_body_equals_remainder_body_bit_for_bit(rows, cols, S, ntt, table, blocks):
    idx = _compared(_plan(rows, cols, S, ntt, table), S)
    X = _inputs(rows, cols)
    for which in (None, "last"):  # the shifted model too: its bias is the one a neighbouring layer must not see
        m, p, v = _run(rows, cols, blocks, which)
        e = _engine(rows, cols, m, 64)
        out = [e.predict(X[i:i + 1]) for i in idx]  # one sample = one workgroup of k_tower_rem
        assert e.counters()["f32_fallback_evals"] == 0
        e.close()
        ps, vs = np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
        assert np.array_equal(p[idx], ps), np.abs(p[idx] - ps).max()
        assert np.array_equal(v[idx], vs), np.abs(v[idx] - vs).max()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("rows,cols,S,ntt,table", GEOMETRIES)
def test_change_of_one_bias_follows_float64(rows, cols, S, ntt, table, blocks, which):
    idx = _compared(_plan(rows, cols, S, ntt, table), S)
    X = _inputs(rows, cols)[idx]
    m, p, v = _run(rows, cols, blocks)
    m2, p2, v2 = _run(rows, cols, blocks, which)

    def hip(p_, v_):
        assert (p_[idx] > 0).all()
        return np.concatenate([nn_probe.log_of_p(p_[idx]), v_[idx].astype(np.float64).reshape(len(idx), 1)], axis=1)

    d_hip = hip(p2, v2) - hip(p, v)
    d_64 = _torch_out(m2, X, torch.float64) - _torch_out(m, X, torch.float64)
    d_32 = _torch_out(m2, X, torch.float32) - _torch_out(m, X, torch.float32)
    assert np.abs(d_64).max() > 1e-2, "the shift must move the outputs far above float32 noise"
    e_hip, e_32 = _criterion(d_hip, d_64, d_32)
    print("RATIO %dx%d %d block(s), shift in the %s layer: max |D_64| %.2e E_hip %.2e E_32 %.2e ratio %.2f"
          % (rows, cols, blocks, which, np.abs(d_64).max(), e_hip, e_32, e_hip / e_32))
    assert e_hip <= K * e_32, (e_hip, e_32)
