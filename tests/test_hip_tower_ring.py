"""The two-cout-tile tower body (k_tower<64, NT, 0, 1, true>) streams the weight fragments of a layer's K-steps 2..17 through a
deep ring of LDS slots that lies at the start of the layer's DESTINATION image (dead during the K-loop: the residual stream is in
registers and the epilogue rewrites every valid row), with the DMA several steps ahead and counted waits at the step ends.  A
slot that is overwritten too early, read too early or left in the image would change the results, so the main launch must
give the SAME BITS as the one-cout-tile remainder bodies (k_tower_rem), which evaluate a sample alone, take their weights
straight into registers and know nothing of the ring.

Cases: the smallest shapes at which the ring can go wrong -- one block (two layers: one hand-over, both image parities used once)
and three (odd and even layers repeat); the row-table geometries (6x6: 245 rows, 3x3: 240 rows), the natural order with 4 tiles
per wave pair (8x8: 243 rows), 3 tiles (7x7: 192 rows, the smallest image the shipped heads reach) and the two-tile body
(3x3 with 64 head channels: 128 rows), which keeps the two-slot ring: not every image of that body could hold the slots.

The main body only takes full rounds of (compute units x samples per workgroup) samples and Engine.predict chunks by n_slots,
so the engines here have n_slots >= n."""
import functools

import numpy as np
import pytest
import torch

from oracle import nn_plan, nn_ref

pytestmark = pytest.mark.gpu

WRING_UNITS = 512   # csrc/tower_plan.h: 16-byte units per ring slot
S4 = (64 + 8) // 4  # 16-byte units per LDS row of a 64-channel image
RING_P = 3          # csrc/nn.hip, DBAZ_RING_P: the prefetch distance = the slots asked for


def ring_slots(ntt):
    """csrc/nn.hip, wring_deep_slots: the slots the body of ntt tiles per wave pair keeps in its destination image.  The plan picks
    that body for more than 64 * (ntt - 1) rows, and the slots must end inside those rows; fewer than 3 is the two-slot ring
    behind the images (0)."""
    units = (64 * (ntt - 1) + 1) * S4
    p = RING_P
    while p > 2 and p * WRING_UNITS > units:
        p -= 1
    return p if p > 2 else 0


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _engine(rows, cols, model, n_slots):
    from dotsboxesaz_amd.engine import Engine
    e = Engine(rows, cols, n_slots, mcts_num_read=8, evaluator="resnet", nn_precision=1)
    c = model.cfg
    e.load_state_dict(model.state_dict(), "resnet", c["channels"], c["blocks"], c["head_channels"], c["value_fc"])
    return e


def _big_n():
    return 2 * _cus() * 16 + 7  # at least one full round for any S <= 16


@functools.lru_cache(maxsize=None)
def _run(rows, cols, blocks, hc):
    """one batch of random samples through the SAME predict call twice: (model, X, p, v)"""
    n = _big_n()
    torch.manual_seed(rows * 131 + cols * 17 + blocks * 5 + hc)
    m = nn_ref.ResNetZeroRef(rows, cols, 64, blocks, head_channels=hc)
    nn_ref.randomize_bn(m, 7)
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


# (rows, cols, head channels, samples per workgroup, tiles per wave pair, rows of a full workgroup, deep slots, row table)
GEOMETRIES = [
    (6, 6, 16, 5, 4, 245, 3, True),
    (3, 3, 16, 15, 4, 240, 3, True),
    (8, 8, 16, 3, 4, 243, 3, False),
    (7, 7, 16, 3, 3, 192, 3, False),
    (3, 3, 64, 8, 2, 128, 0, False),   # the two-tile body: these 2 304 units would hold the slots, not every two-tile image does -> two-slot ring
]


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("rows,cols,hc,S,ntt,R,slots,table", GEOMETRIES)
def test_deep_ring_body_equals_remainder_body_bit_for_bit(rows, cols, hc, S, ntt, R, slots, table, blocks):
    cus = _cus()
    plan = nn_plan.Plan(rows, cols, 64, hc, 8, 1, cus)
    # the case is what its name says: the body, its image and the path its geometry takes (the kernel's arithmetic)
    assert plan.c2 and (plan.S_c2, plan.NT_c2, plan.S_c2 * plan.HW, plan.perm) == (S, ntt, R, table), plan.main_body()
    assert ring_slots(plan.NT_c2) == slots
    assert slots * WRING_UNITS <= R * S4, "a slot would reach the zero region of the image"
    n = _big_n()
    mode, n_full = plan.split(n)
    assert plan.round <= n_full < n, (mode, n_full)  # full rounds in the main body and a tail (8x8: in the main body as well)
    m, X, p, v = _run(rows, cols, blocks, hc)
    wgs = n_full // S
    idx = []
    for wg in (0, wgs // 4, wgs // 2 + 1, (3 * wgs) // 4 + 2, wgs - 1):  # first, three in between, last workgroup of the full rounds
        idx += [wg * S, wg * S + S // 2, wg * S + S - 1]
    idx += [n_full, n - 2, n - 1]                                         # the tail behind the full rounds
    idx = sorted(set(i for i in idx if 0 <= i < n))
    assert len(idx) >= 15
    ps, vs = _singles(rows, cols, m, X, idx)
    assert np.array_equal(p[idx], ps), np.abs(p[idx] - ps).max()
    assert np.array_equal(v[idx], vs), np.abs(v[idx] - vs).max()
