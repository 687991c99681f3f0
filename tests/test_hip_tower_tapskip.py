"""The two-cout-tile tower body (k_tower<64, NT, 0, 1, true>, f16x3, 64 channels) hands its position rows to the tiles through
the table of csrc/tower_perm.h and drops the taps that an edge tile never needs.  A dropped MFMA would have added +-0, so the
main launch must give the SAME BITS as the one-cout-tile remainder bodies (k_tower_rem), which evaluate a sample alone and whose
code knows nothing of the table.

The main body only takes full rounds of (compute units x samples per workgroup) samples and Engine.predict chunks by n_slots,
so the engines here have n_slots >= n."""
import functools

import numpy as np
import pytest
import torch

from oracle import nn_ref

pytestmark = pytest.mark.gpu
TOL = 1e-4  # tests/test_hip_nn.py


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _engine(rows, cols, model, n_slots):
    from dotsboxesaz_amd.engine import Engine
    e = Engine(rows, cols, n_slots, mcts_num_read=8, evaluator="resnet", nn_precision=1)
    c = model.cfg
    e.load_state_dict(model.state_dict(), "resnet", c["channels"], c["blocks"], c["head_channels"], c["value_fc"])
    return e


@functools.lru_cache(maxsize=None)
def _run(rows, cols, n):
    """one batch of n random samples through one predict call: (model, X, p, v)"""
    torch.manual_seed(rows * 31 + cols + n)
    m = nn_ref.ResNetZeroRef(rows, cols, 64, 2)
    nn_ref.randomize_bn(m, 5)
    X = torch.randn(n, 3, rows + 1, cols + 1).numpy()
    e = _engine(rows, cols, m, n)
    p, v = e.predict(X)  # raises if an activation left f16's range
    assert e.counters()["f32_fallback_evals"] == 0
    e.close()
    return m, X, p, v


def _singles(rows, cols, m, X, idx):
    """the samples idx one at a time: each is a remainder launch of one workgroup (k_tower_rem)"""
    e = _engine(rows, cols, m, 64)
    out = [e.predict(X[i:i + 1]) for i in idx]
    assert e.counters()["f32_fallback_evals"] == 0
    e.close()
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def _big_n():
    return 2 * _cus() * 16 + 7  # at least one full round for any S <= 16


# S: samples per workgroup of the main body (what 160 KB of LDS hold of min(16, 256 / HW) samples)
@pytest.mark.parametrize("rows,cols,S", [(6, 6, 5), (3, 3, 15), (5, 5, 6), (6, 5, 5)])
def test_main_body_equals_remainder_body_bit_for_bit(rows, cols, S):
    """6x6 (5 samples per workgroup) and 3x3 (15) run the tap-skipping streams; 5x5 and 6x5 (H != W: x and y must not be
    swapped) run them or the natural order, whichever their geometry allows."""
    n = _big_n()
    rnd = _cus() * S
    n_full = (n // rnd) * rnd
    m, X, p, v = _run(rows, cols, n)
    step = max(1, S // 5)
    idx = list(range(0, S, step))[:5]                       # first workgroup, every residue (6x6) / a spread of them
    idx += [n_full - 1 - r for r in range(0, S, step)][:5]  # last workgroup of the full rounds
    idx += [n_full // 2 + 1, n_full // 2 + S + 2, n_full // 3]
    idx += [n_full, n - 2, n - 1]                           # the tail behind the full rounds
    idx = sorted(set(i for i in idx if 0 <= i < n))
    assert len(idx) >= 12
    ps, vs = _singles(rows, cols, m, X, idx)
    assert np.array_equal(p[idx], ps), np.abs(p[idx] - ps).max()
    assert np.array_equal(v[idx], vs), np.abs(v[idx] - vs).max()


def test_partial_workgroup_in_the_main_launch():
    """A tail too long for one round of the 4-sample remainder body stays with the main launch, whose last workgroup then holds
    fewer than S samples (rows behind them are invalid lanes of whatever tile the table put them in)."""
    cus = _cus()
    n = cus * 5 + cus * 4 + 1
    while n % 5 == 0:
        n += 1
    assert n - cus * 9 <= 4
    m, X, p, v = _run(6, 6, n)
    idx = sorted(set(list(range(n - 6, n)) + [0, 4, cus * 5 - 1, cus * 5, cus * 7 + 3, n - 9]))
    ps, vs = _singles(6, 6, m, X, idx)
    assert np.array_equal(p[idx], ps), np.abs(p[idx] - ps).max()
    assert np.array_equal(v[idx], vs), np.abs(v[idx] - vs).max()


def test_main_body_vs_torch():
    n = _big_n()
    m, X, p, v = _run(6, 6, n)
    idx = np.sort(np.random.RandomState(0).choice(n, 64, replace=False))
    pr, vr = nn_ref.predict_sync(m, X[idx])
    assert np.abs(p[idx] - pr).max() < TOL, np.abs(p[idx] - pr).max()
    assert np.abs(v[idx] - vr).max() < TOL, np.abs(v[idx] - vr).max()
    assert np.allclose(p.sum(1), 1.0, atol=1e-5)
