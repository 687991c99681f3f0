"""The training step on HIP (csrc/train.hip, csrc/train_net.hip) at every class of its launch plan (csrc/train_plan.h) against
torch in FLOAT64 on the CPU.

The cases, their batch sizes (computed from the plan and the device's compute-unit count), the models and the criterion live in
oracle/train_cases.py; tests/test_train_plan.py (CPU) proves that the tables reach every launch class at 64, 256 and 304
compute units, that the decided models keep every ReLU input of the float64 reference at least 1.0 away from zero, and that the
criterion rejects a float32 result with one sample, chunk, row block or K step missing.

Criterion (the existing training tests', unchanged): e_hip <= max(4 e_torch32, floor) relative to each tensor's largest
magnitude, floors 2e-6 for outputs and running statistics, 2e-6 (tower) / 2e-5 (whole network) for gradients; conv biases in
front of a BatchNorm, and gradient tensors that are analytically zero, are bounded absolutely (train_cases.judge).  Large cases
use "decided" models, so EVERY sample takes part in every comparison; small cases use random models with a seed search.

Measured on an MI355X (256 compute units): see EXPERIMENTS.md, "Training step at every launch-plan class"."""
import time

import pytest
import torch

from oracle import train_cases as TC
from oracle import train_plan

pytestmark = pytest.mark.gpu

TOWER_IDS = [c.id for c in TC.tower_cases(256)]
NET_IDS = [c.id for c in TC.net_cases(256)]


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def report(case, rows, zero_rule, t0):
    worst = max(rows, key=lambda r: r[3])
    ratio = max((r[1] / r[2] for r in rows if r[2] > 0 and not r[0].endswith(TC.CONV_BIAS)), default=0.0)
    for r in rows:
        print("  %-40s e_hip %.3g  e_t32 %.3g  e_hip/bound %.3g" % r)
    print("CASE %s n=%d: worst e_hip/bound %.3g (%s), largest e_hip/e_t32 %.3g, zero rule %s, %.2f s"
          % (case.id, case.n, worst[3], worst[0], ratio, zero_rule, time.time() - t0))


@pytest.mark.parametrize("cid", TOWER_IDS)
def test_tower_class_vs_float64(cid):
    """dbaz_trainer_forward / _backward: output, input gradient, every parameter gradient and running statistic, all samples"""
    t0 = time.time()
    case = {c.id: c for c in TC.tower_cases(device_cus())}[cid]
    blocks, x, gout = TC.build_tower_case(case)
    t64 = TC.torch_tower(blocks, x, gout, torch.float64)
    t32 = TC.torch_tower(blocks, x, gout, torch.float32)
    hip = TC.hip_tower(blocks, x, gout)
    assert hip["nbt"] == [1]
    margin = float(t64["margin"].min())
    print("smallest |ReLU input| %.3g" % margin)
    assert margin >= (TC.DECIDED_MIN if case.decided else TC.UNSAFE)
    rows, failures, zero_rule = TC.judge(hip, t32, t64, TC.FLOORS_TOWER)
    report(case, rows, zero_rule, t0)
    assert not failures, failures


@pytest.mark.parametrize("cid", NET_IDS)
def test_network_class_vs_float64(cid):
    """dbaz_trainer_net_forward / _backward: logp, v, the loss, every parameter gradient and running statistic, all samples"""
    t0 = time.time()
    case = {c.id: c for c in TC.net_cases(device_cus())}[cid]
    model, x, pi, z = TC.build_net_case(case)
    t64 = TC.torch_net(model, x, pi, z, torch.float64)
    t32 = TC.torch_net(model, x, pi, z, torch.float32)
    hip = TC.hip_net(model, x, pi, z)
    assert hip["nbt"] == [1] and hip["logp"].shape == t64["logp"].shape and hip["v"].shape == (case.n, 1)
    margin = float(t64["margin"].min())
    print("smallest |ReLU input| %.3g" % margin)
    assert margin >= (TC.DECIDED_MIN if case.decided else TC.UNSAFE)
    rows, failures, zero_rule = TC.judge(hip, t32, t64, TC.FLOORS_NET, outputs=("logp", "v"))
    report(case, rows, zero_rule, t0)
    assert not failures, failures


# ---- boards the plan refuses
@pytest.mark.parametrize("board,needle", [((1, 97), "209328 bytes of LDS"), ((14, 14), "at most 196 positions")])
def test_refused_boards_are_refused_on_the_host(board, needle):
    """1x97: k_wgrad_h3 would need 209 328 B of LDS for one sample; 14x14: 225 positions.  The plan refuses both before anything is
    allocated or launched, and train_tower.supported() sends their models to torch."""
    from dotsboxesaz_amd import nn as dnn, train_tower
    rows, cols = board
    with pytest.raises(ValueError, match="unsupported"):
        train_plan.Plan(rows, cols)
    before = train_tower.handles_created
    with pytest.raises(train_tower.TrainerError, match="board %dx%d unsupported.*%s" % (rows, cols, needle)):
        train_tower.TowerTrainer(rows, cols, 64, 1, 4)
    assert train_tower.handles_created == before
    m = dnn.ResNetZero(dnn.resnet_params(rows, cols, 64, 1)).cuda().train(True)
    x = torch.zeros(2, 3, rows + 1, cols + 1, device="cuda")
    assert not train_tower.supported(m, x) and not train_tower.net_supported(m, x)
    assert train_tower.supported(dnn.ResNetZero(dnn.resnet_params(13, 13, 64, 1)).cuda().train(True), torch.zeros(2, 3, 14, 14, device="cuda"))


def test_training_forward_of_a_refused_board_falls_back_to_torch():
    from dotsboxesaz_amd import nn as dnn, train as T, train_tower
    torch.manual_seed(4)
    m = dnn.ResNetZero(dnn.resnet_params(1, 97, 64, 1)).cuda().train(True)
    x = (torch.rand(3, 3, 2, 98, device="cuda") < 0.4).float()
    before = train_tower.handles_created
    p, v = T.training_forward(m, x)                       # used to raise TrainerError
    pr, vr = T.training_forward(m, x, hip_tower=False)
    assert train_tower.handles_created == before and not type(p.grad_fn).__name__.startswith(("_NetFn", "_TowerFn"))
    assert torch.allclose(p, pr, rtol=1e-5, atol=1e-6) and torch.allclose(v, vr, rtol=1e-5, atol=1e-6)
    with pytest.raises(RuntimeError):
        T.training_forward(m, x, hip_tower=True)


# ---- exact properties (bitwise)
EXACT = [((6, 6), 2, 37), ((2, 3), 1, 9)]


def tower_setup(board, nb, n):
    blocks, _ = TC.make_blocks(nb, 7 * nb + n)
    x, gout = TC.tower_batch(n, board[0] + 1, board[1] + 1, n)
    return blocks, x, gout


def net_setup(board, nb, n):
    model = TC.make_model(board[0], board[1], nb, 11 * nb + n)
    return (model,) + TC.net_batch(board[0], board[1], n, 2 * (board[0] + 1) * (board[1] + 1), 5 + n)


def tensors_of(res):
    out = {k: v for k, v in res.items() if isinstance(v, torch.Tensor)}
    out.update({"grad " + k: v for k, v in res["grads"].items()})
    out.update({"stat " + k: v for k, v in res["stats"].items()})
    return out


def assert_same_bits(a, b, what):
    ta, tb = tensors_of(a), tensors_of(b)
    assert ta.keys() == tb.keys() and len(ta) > 4
    for k in ta:
        assert torch.equal(ta[k], tb[k]), (what, k)


@pytest.mark.parametrize("board,nb,n", EXACT)
def test_handle_size_does_not_change_results(board, nb, n):
    """every activation and mask stride uses max_batch: a handle of 64 and one of exactly n give the same bits, both entry points"""
    blocks, x, gout = tower_setup(board, nb, n)
    assert_same_bits(TC.hip_tower(blocks, x, gout, max_batch=64), TC.hip_tower(blocks, x, gout, max_batch=n), "tower")
    model, xn, pi, z = net_setup(board, nb, n)
    assert_same_bits(TC.hip_net(model, xn, pi, z, max_batch=64), TC.hip_net(model, xn, pi, z, max_batch=n), "network")


@pytest.mark.parametrize("board,nb,n", EXACT)
def test_one_handle_reused_for_other_batch_sizes(board, nb, n):
    """n = 64, then n, then 64 through ONE handle: the first and third pass are equal bit for bit (nothing of a pass survives in the handle)"""
    from dotsboxesaz_amd import train_tower
    tr = train_tower.TowerTrainer(board[0], board[1], 64, nb, 64)
    blocks, x64, g64 = tower_setup(board, nb, 64)
    _, x, gout = tower_setup(board, nb, n)
    first = TC.hip_tower(blocks, x64, g64, trainer=tr)
    TC.hip_tower(blocks, x, gout, trainer=tr)
    assert_same_bits(first, TC.hip_tower(blocks, x64, g64, trainer=tr), "tower")
    model, xn64, pi64, z64 = net_setup(board, nb, 64)
    _, xn, pi, z = net_setup(board, nb, n)
    first = TC.hip_net(model, xn64, pi64, z64, trainer=tr)
    TC.hip_net(model, xn, pi, z, trainer=tr)
    assert_same_bits(first, TC.hip_net(model, xn64, pi64, z64, trainer=tr), "network")
    tr.close()


@pytest.mark.parametrize("board,nb,n", EXACT)
def test_power_of_two_scaling_of_the_upstream_gradient_is_exact(board, nb, n):
    """every scale in the kernels is a power of two taken from the tensor's own maximum and the f64 sums commute with it: an upstream
    gradient times 2^k gives every gradient times exactly 2^k"""
    blocks, x, gout = tower_setup(board, nb, n)
    base = TC.hip_tower(blocks, x, gout)
    model, xn, pi, z = net_setup(board, nb, n)
    nbase = TC.hip_net(model, xn, pi, z)
    for k in (-40, -20, 20, 40):
        f = 2.0 ** k
        got = TC.hip_tower(blocks, x, gout * f)
        assert torch.equal(got["grad_x"], base["grad_x"] * f), k
        for name in base["grads"]:
            assert torch.equal(got["grads"][name], base["grads"][name] * f), ("tower", k, name)
        ngot = TC.hip_net(model, xn, pi, z, scale=f)
        for name in nbase["grads"]:
            assert torch.equal(ngot["grads"][name], nbase["grads"][name] * f), ("network", k, name)


@pytest.mark.parametrize("board,nb,n", EXACT)
def test_zero_upstream_gradient_and_zero_input(board, nb, n):
    blocks, x, gout = tower_setup(board, nb, n)
    got = TC.hip_tower(blocks, x, gout * 0.0)
    assert float(got["grad_x"].abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in got["grads"].values())
    model, xn, pi, z = net_setup(board, nb, n)
    ngot = TC.hip_net(model, xn, pi, z, scale=0.0)
    assert all(float(g.abs().max()) == 0.0 for g in ngot["grads"].values())
    for res in (TC.hip_tower(blocks, x * 0.0, gout), TC.hip_net(model, xn * 0.0, pi, z)):
        assert all(bool(torch.isfinite(t).all()) for t in tensors_of(res).values())
