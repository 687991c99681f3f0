"""The four patterned streams of the two-cout-tile tower body (k_tower<64, 4, 0, 1, true> under the row table) do not issue the
head block of a K-step -- its ring DMA piece, the bias loads of the step before last, the ring reads of the next step's weight
fragments -- at the same place: one half of the workgroup issues it behind the step barrier, the other behind its hi*hi phase
(csrc/nn.hip, DBAZ_STAGGER).  Every accumulator still receives the same MFMAs in the same order, so the main launch must give
the SAME BITS as the single-sample remainder body (k_tower_rem), which has no ring, no row table and no staggered head.  A slot
overwritten or read too early, a bias used before it landed or a wait that names the wrong reads would change them.

tests/test_hip_tower_ring.py samples 3 samples of 5 workgroups; here EVERY sample of the first, a middle and the last workgroup of
the full round is compared, and the tail: every row of every tile of all four patterns.  Geometries: the row-table ones, because
only their streams changed -- 6x6 (S = 5, 245 rows), 3x3 (S = 15, 240 rows), 5x5 (S = 6, 216 rows) -- and 7x7 (natural order,
three tiles per wave pair) as the control that an untouched stream still agrees.  One block has both layer parities and the last
layer's self-fetch; two blocks have a residual layer that is followed by another layer.  BatchNorm is randomised, so every layer
has another non-zero bias.

One full round of the main launch (compute units x samples per workgroup) and a tail of 7; Engine.predict chunks by n_slots, so
the engines here have n_slots >= n."""
import functools

import numpy as np
import pytest
import torch

from oracle import nn_plan, nn_ref

pytestmark = pytest.mark.gpu

TAIL = 7


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(rows, cols):
    return nn_plan.Plan(rows, cols, 64, 16, 8, 1, _cus())


def _engine(rows, cols, model, n_slots):
    from dotsboxesaz_amd.engine import Engine
    e = Engine(rows, cols, n_slots, mcts_num_read=8, evaluator="resnet", nn_precision=1)
    c = model.cfg
    e.load_state_dict(model.state_dict(), "resnet", c["channels"], c["blocks"], c["head_channels"], c["value_fc"])
    return e


@functools.lru_cache(maxsize=None)
def _run(rows, cols, blocks):
    """one batch of random samples through the SAME predict call twice: (model, X, p, v)"""
    n = _plan(rows, cols).round + TAIL
    torch.manual_seed(rows * 137 + cols * 19 + blocks * 7)
    m = nn_ref.ResNetZeroRef(rows, cols, 64, blocks, head_channels=16)
    nn_ref.randomize_bn(m, 11)
    X = torch.randn(n, 3, rows + 1, cols + 1).numpy()
    e = _engine(rows, cols, m, n)
    p, v = e.predict(X)  # raises if an activation left f16's range
    p2, v2 = e.predict(X)
    assert e.counters()["f32_fallback_evals"] == 0
    e.close()
    assert np.array_equal(p, p2) and np.array_equal(v, v2), "the same call gave other bits the second time"
    return m, X, p, v


def _singles(rows, cols, m, X, idx):
    """the samples idx one at a time: each is a remainder launch of one workgroup (k_tower_rem)"""
    e = _engine(rows, cols, m, 64)
    out = [e.predict(X[i:i + 1]) for i in idx]
    assert e.counters()["f32_fallback_evals"] == 0
    e.close()
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


# (rows, cols, samples per workgroup, tiles per wave pair, rows of a full workgroup, row table)
GEOMETRIES = [
    (6, 6, 5, 4, 245, True),
    (3, 3, 15, 4, 240, True),
    (5, 5, 6, 4, 216, True),
    (7, 7, 3, 3, 192, False),  # control: natural order, the stream is the parent's
]


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("rows,cols,S,ntt,R,table", GEOMETRIES)
def test_staggered_body_equals_remainder_body_bit_for_bit(rows, cols, S, ntt, R, table, blocks):
    plan = _plan(rows, cols)
    # the case is what its name says: the body, its image and the path its geometry takes (the kernel's arithmetic)
    assert plan.c2 and (plan.S_c2, plan.NT_c2, plan.S_c2 * plan.HW, plan.perm) == (S, ntt, R, table), plan.main_body()
    assert plan.main_body() == "k_tower<64,%d,0,1,true>/%s" % (ntt, "table" if table else "natural")
    n = plan.round + TAIL
    mode, n_full = plan.split(n)
    assert mode != 0 and n_full == plan.round, (mode, n_full)  # one full round in the main body, the tail in a remainder body
    m, X, p, v = _run(rows, cols, blocks)
    wgs = n_full // S
    idx = []
    for wg in (0, wgs // 2, wgs - 1):         # every sample of the first, a middle and the last workgroup of the full round
        idx += list(range(wg * S, wg * S + S))
    idx += list(range(n_full, n))             # the tail behind it
    assert len(set(idx)) == 3 * S + TAIL and max(idx) == n - 1
    ps, vs = _singles(rows, cols, m, X, idx)
    assert np.array_equal(p[idx], ps), np.abs(p[idx] - ps).max()
    assert np.array_equal(v[idx], vs), np.abs(v[idx] - vs).max()
