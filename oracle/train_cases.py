"""Cases, models and the comparison criterion of the training-step tests -- TEST INFRASTRUCTURE ONLY.

* the case tables of tests/test_hip_train_classes.py (tower_cases / net_cases): every batch size is computed from the launch plan
  (oracle/train_plan.py) and the device's compute-unit count, and every case carries the predicates on the plan that say
  which launch class it is there for; tests/test_train_plan.py asserts them at 64, 256 and 304 compute units;
* "decided" models: networks in which no ReLU input of the float64 reference comes near zero, so that no float32 evaluation
  can land on the other side of a ReLU and EVERY sample of a large batch is comparable tightly (decide_bn and friends);
* float64 / float32 torch references that record the smallest |ReLU input| per sample, the HIP runners, and the criterion
  e_hip <= max(4 e_torch32, floor) of the existing training tests (judge);
* mutants of a float32 result (a sample, a chunk, 32 rows, a K step left out of one sum) the criterion has to reject."""
import collections
import copy

import torch
import torch.nn.functional as F

from . import nn_ref, train_plan

UNSAFE = 1.5e-6          # random models: a ReLU input closer to 0 than this may flip in a float32 evaluation (seed search)
DECIDED_MIN = 1.0        # decided models: the smallest |ReLU input| of the float64 reference
BIG_RELU_INPUTS = 3e5    # cases with more ReLU inputs than this use decided models

Case = collections.namedtuple("Case", "id board nb n decided value_fc why")


# ---------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------
def n_6x6_many_chunks(cus):
    """smallest n >= max(1 338, 4 cus + 1) with n mod 4 = 1 and n mod 5 != 0: 6x6 with more chunks than workgroups, a partial last
    chunk, two k_bn_apply passes (M > 65 536) and kchunk = 192 in the M-split GEMMs"""
    n = max(1338, 4 * cus + 1)
    while n % 4 != 1 or n % 5 == 0:
        n += 1
    return n


def tower_cases(cus):
    P = train_plan.Plan
    p11, p99, p1010 = P(1, 1, cus), P(9, 9, cus), P(10, 10, cus)
    return [
        Case("1x1-n1", (1, 1), 1, 1, False, 8, "M = 4, one column-sum workgroup, BatchNorm over 4 elements"),
        Case("1x1-n70", (1, 1), 1, 70, False, 8, "S = 64 and a partial conv workgroup; one full and one partial k_wgrad_h3 chunk"),
        Case("13x13-n3", (13, 13), 1, 3, False, 8, "S = 1, Swh = 1, partial thirteenth tile, padding rows in the last K step"),
        Case("7x15-n3", (7, 15), 1, 3, False, 8, "R = 256 exactly, H < W"),
        Case("15x7-n3", (15, 7), 1, 3, False, 8, "R = 256 exactly, H > W"),
        Case("3x6-n20", (3, 6), 1, 20, False, 8, "k_wgrad_h3<8> with H + 1 = 4; chunks 7, 7, 6"),
        Case("6x3-n13", (6, 3), 1, 13, False, 8, "generic k_wgrad_h3 with H + 1 = 7; chunks 6, 6, 1"),
        Case("6x6-n40", (6, 6), 1, 40, False, 8, "n a multiple of S and of Swh"),
        Case("13x13-n17", (13, 13), 1, 17, True, 8, "k_wgrad_reduce: 4-in-flight loop + tail"),
        Case("13x13-n61", (13, 13), 1, 61, True, 8, "k_wgrad_reduce: 16-in-flight loop just entered"),
        Case("13x13-n77", (13, 13), 1, 77, True, 8, "k_wgrad_reduce: both loops"),
        Case("13x13-n83", (13, 13), 1, 83, True, 8, "k_wgrad_reduce: both loops and the tail"),
        Case("9x9-chunks", (9, 9), 1, cus * p99.Swh + 1, True, 8, "workgroup 0: a full chunk, then a partial one"),
        Case("10x10-chunks", (10, 10), 1, cus * p1010.Swh + 1, True, 8, "Swh = 1, workgroup 0 walks two chunks"),
        Case("1x1-chunks", (1, 1), 1, cus * p11.Swh + 1, True, 8, "1x1: workgroup 0 walks a full chunk, then one sample"),
        Case("6x6-chunks", (6, 6), 1, n_6x6_many_chunks(cus), True, 8, "more chunks than workgroups, partial last chunk, two k_bn_apply passes"),
        Case("1x1-32blocks", (1, 1), 32, 8, True, 8, "L = TL_MAX"),
    ]


def net_cases(cus):
    p11 = train_plan.Plan(1, 1, cus)
    return [
        Case("6x6-n257", (6, 6), 1, 257, True, 8, "M-split GEMMs: kchunk = 64, two steps per split"),
        Case("6x6-n513", (6, 6), 2, 513, True, 8, "M-split GEMMs: kchunk = 96 (odd step count); FC weight gradient kchunk = 64, last split one row"),
        Case("6x6-chunks", (6, 6), 1, n_6x6_many_chunks(cus), True, 8, "kchunk = 192; the head row grids saturated and striding"),
        Case("1x1-wrap", (1, 1), 1, max(cus * p11.Swh, 8192) + 1, True, 8, "k_stem_conv and k_head_out wrap; A = 8, KF = 128"),
        Case("13x13-vf256", (13, 13), 1, 3, False, 256, "A = 392, NO = 648, KF = 6 272"),
        Case("3x3-vf1", (3, 3), 1, 70, False, 1, "NO = 33, NOp = 36"),
        Case("2x3-vf17", (2, 3), 1, 9, False, 17, "NO = 41, NOp = 44"),
        Case("15x7-n3", (15, 7), 1, 3, False, 8, "H != W through the stem taps and the FC row order"),
    ]


def relu_inputs(case, net):
    """ReLU inputs of a case: what decides between a random model with a seed search and a decided model"""
    H, W = case.board[0] + 1, case.board[1] + 1
    per_sample = 64 * H * W * 2 * case.nb
    if net:
        per_sample += 64 * H * W + 32 * H * W + case.value_fc
    return case.n * per_sample


def class_predicates(cus):
    """{launch class: (case list name, case id, predicate on (plan, case))}: what tests/test_train_plan.py asserts of the tables"""
    def gem(p, c, name):
        return p.gemms(c.n, c.value_fc)[name]
    return {
        "k_wgrad_h3: a full chunk, then the partial last chunk in one workgroup":
            ("tower", "9x9-chunks", lambda p, c: p.wgrad_chunks(c.n) == cus + 1 and p.wgrad_walk(c.n, 0) == [p.Swh, 1] and p.Swh == 2),
        "k_wgrad_h3: two chunks per workgroup at Swh = 1":
            ("tower", "10x10-chunks", lambda p, c: p.Swh == 1 and p.wgrad_walk(c.n, 0) == [1, 1]),
        "k_wgrad_h3: chunks > workgroups on 1x1":
            ("tower", "1x1-chunks", lambda p, c: p.wgrad_chunks(c.n) == cus + 1 and p.wgrad_walk(c.n, 0) == [p.Swh, 1]),
        "k_wgrad_h3: more than two chunks per workgroup, partial last chunk":
            ("tower", "6x6-chunks", lambda p, c: p.wgrad_chunks(c.n) > cus and c.n % p.Swh != 0 and p.pwc == 8),
        "k_wgrad_h3<8> with H + 1 != 7":
            ("tower", "3x6-n20", lambda p, c: p.pwc == 8 and p.H == 4 and [min(p.Swh, c.n - i * p.Swh) for i in range(p.wgrad_chunks(c.n))] == [7, 7, 6]),
        "k_wgrad_h3<0> with H + 1 = 7":
            ("tower", "6x3-n13", lambda p, c: p.pwc == 0 and p.H == 7 and [min(p.Swh, c.n - i * p.Swh) for i in range(p.wgrad_chunks(c.n))] == [6, 6, 1]),
        "Swh = 1 and S = 1, partial thirteenth tile, three empty tiles, padding rows in the last K step":
            ("tower", "13x13-n3", lambda p, c: p.S == 1 and p.Swh == 1 and p.conv_tiles(c.n) == (12, 4, 3) and p.wgrad_pad_rows() == 14),
        "S = 64 (1x1) with a partial conv workgroup":
            ("tower", "1x1-n70", lambda p, c: p.S == 64 and c.n % p.S != 0 and c.n > p.S),
        "one column-sum workgroup, M = 4":
            ("tower", "1x1-n1", lambda p, c: p.M(c.n) == 4 and train_plan.red_blocks(p.M(c.n)) == 1),
        "R = 256 exactly (H < W)": ("tower", "7x15-n3", lambda p, c: p.S * p.HW == 256 and p.H < p.W),
        "R = 256 exactly (H > W)": ("tower", "15x7-n3", lambda p, c: p.S * p.HW == 256 and p.H > p.W),
        "n a multiple of S and Swh": ("tower", "6x6-n40", lambda p, c: c.n % p.S == 0 and c.n % p.Swh == 0),
        "k_wgrad_reduce: 4-in-flight loop + tail only":
            ("tower", "13x13-n17", lambda p, c: p.reduce_loops(c.n)[0] == 0 and p.reduce_loops(c.n)[1] >= 1 and p.reduce_loops(c.n)[2] >= 1),
        "k_wgrad_reduce: 16-in-flight loop just entered (nparts = 61)":
            ("tower", "13x13-n61", lambda p, c: p.wgrad_grid(c.n) == 61 and p.reduce_loops(c.n)[0] == 1),
        "k_wgrad_reduce: the 16-in-flight loop, then the 4-in-flight loop":
            ("tower", "13x13-n77", lambda p, c: p.reduce_loops(c.n) == ((1, 1, 0) if cus >= 77 else (1, 0, 0))),
        # (nparts <= compute units: a device of 64 has no partials behind the first trip of the 16-in-flight loop)
        "k_wgrad_reduce: all three loops":
            ("tower", "13x13-n83", lambda p, c: p.reduce_loops(c.n) == ((1, 1, 1) if cus >= 83 else (1, 0, 0))),
        "bn_apply_grid with two passes":
            ("tower", "6x6-chunks", lambda p, c: train_plan.bn_apply_passes(p.M(c.n) * 16) == 2),
        "L = TL_MAX": ("tower", "1x1-32blocks", lambda p, c: 2 * c.nb == train_plan.TL_MAX),
        "M-split GEMMs: two K steps per split":
            ("net", "6x6-n257", lambda p, c: gem(p, c, "head_wgrad")[1] == 64 and gem(p, c, "stem_wgrad")[1] == 64),
        "M-split GEMMs: an odd number of K steps per split":
            ("net", "6x6-n513", lambda p, c: gem(p, c, "head_wgrad")[1] == 96),
        "FC weight gradient: kchunk = 64, z = 9, last split one row":
            ("net", "6x6-n513", lambda p, c: gem(p, c, "fc_wgrad")[1:] == (64, 9, 1)),
        "M-split GEMMs: kchunk = 192; head row grids saturated and striding":
            ("net", "6x6-chunks", lambda p, c: gem(p, c, "head_wgrad")[1] == 192 and p.M(c.n) > 32 * train_plan.NET_HB),
        "k_stem_conv and k_head_out wrap; FC forward kchunk = 32":
            ("net", "1x1-wrap", lambda p, c: c.n > train_plan.STEM_S * train_plan.NET_SB and c.n > 4 * 1024 and gem(p, c, "fc_forward")[:2] == (128, 32)),
        "value_fc = 256: A + VF spans many 64-column tiles":
            ("net", "13x13-vf256", lambda p, c: 2 * p.HW + c.value_fc == 648 and p.HW * 32 == 6272),
        "value_fc = 1: NOp padded": ("net", "3x3-vf1", lambda p, c: 2 * p.HW + c.value_fc == 33),
        "value_fc = 17: NOp padded": ("net", "2x3-vf17", lambda p, c: 2 * p.HW + c.value_fc == 41),
        "H != W through stem and FC": ("net", "15x7-n3", lambda p, c: p.H != p.W and p.HW == 128),
    }


# ---------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------
def dead_set(channels, seed):
    """one channel in eight, seeded offset: every 16-channel tile keeps live and dead channels"""
    return (torch.arange(channels) % 8) == (seed % 8)


def random_bn(bn, g):
    c = bn.num_features
    bn.weight.data = torch.rand(c, generator=g) + 0.5
    bn.bias.data = torch.randn(c, generator=g) * 0.2
    bn.running_mean.data = torch.randn(c, generator=g) * 0.1
    bn.running_var.data = torch.rand(c, generator=g) + 0.5


def decide_bn(bn, g, dead=None):
    """a BatchNorm in front of a ReLU whose outputs stay away from 0: beta = +-8 gamma (1 .. 1.25) per channel"""
    random_bn(bn, g)
    c = bn.num_features
    if dead is None:
        dead = dead_set(c, int(torch.randint(0, 8, (1,), generator=g)))
    mag = 8.0 * bn.weight.data * (1.0 + 0.25 * torch.rand(c, generator=g))
    bn.bias.data = torch.where(dead, -mag, mag)


def make_blocks(nb, seed, decided=False):
    """the tower alone (dbaz_trainer_forward): (blocks, dead channels of the residual stream or None)"""
    torch.manual_seed(seed)
    blocks = torch.nn.Sequential(*[nn_ref._Block(64, 3) for _ in range(nb)])
    g = torch.Generator().manual_seed(seed + 1)
    dead = dead_set(64, seed) if decided else None
    for blk in blocks:
        for bn, shared in ((blk.bn1, False), (blk.bn2, True)):
            if decided:
                decide_bn(bn, g, dead if shared else None)
            else:
                random_bn(bn, g)
    return blocks, dead


def tower_batch(n, H, W, seed, dead=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(n, 64, H, W, generator=g))      # the tower input is a post-ReLU activation
    gout = torch.randn(n, 64, H, W, generator=g) * 1e-3        # gradients are small numbers: exercises the dynamic scaling
    if dead is not None:
        x[:, dead] = 0.0                                       # the residual stream keeps ONE dead set (see decide_bn)
    return x, gout


def make_model(rows, cols, nb, seed, value_fc=8, decided=False):
    from dotsboxesaz_amd import nn as dnn
    torch.manual_seed(seed)
    m = dnn.ResNetZero(dnn.resnet_params(rows, cols, 64, nb, value_fc=value_fc))
    g = torch.Generator().manual_seed(seed + 1)
    dead = dead_set(64, seed)
    for name, mod in m.named_modules():
        if not isinstance(mod, torch.nn.BatchNorm2d):
            continue
        if not decided or name == "bn_input":
            random_bn(mod, g)
        else:
            decide_bn(mod, g, dead if (name == "resnet.bn0" or name.endswith(".bn2")) else None)
    if decided:
        ph, vh = m.policy_head, m.value_head
        vf = vh.fc0.out_features
        vh.fc0.weight.data *= 0.02
        sign = torch.where(torch.rand(vf, generator=g) < 0.5, -1.0, 1.0)
        if vf > 1:
            sign[0], sign[1] = 1.0, -1.0
        vh.fc0.bias.data = sign * (4.0 + torch.rand(vf, generator=g))
        ph.fc.weight.data *= 0.05
        ph.fc.bias.data *= 0.05
        # |fc1's output| <= 1 + 0.3 |b| <= 1.3 whatever value_fc is: tanh stays below 0.87
        w1 = vh.fc1.weight.data
        vh.fc1.weight.data = w1 / (6.0 * float(w1.abs().sum()))   # fc0's outputs: |bias| <= 5 and |w . h| well below 1
        vh.fc1.bias.data *= 0.3
    return m


def net_batch(rows, cols, n, A, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, 3, rows + 1, cols + 1, generator=g) < 0.4).float()
    pi = torch.softmax(torch.randn(n, A, generator=g) * 2.0, dim=1)
    z = (torch.rand(n, 1, generator=g) < 0.5).float() * 2.0 - 1.0
    return x, pi, z


# ---------------------------------------------------------------------------------------------------------------------------
# torch references (float64 = ground truth, float32 = the yardstick) and the HIP runs
# ---------------------------------------------------------------------------------------------------------------------------
class _Margin:
    """per sample: the smallest |ReLU input| seen"""

    def __init__(self):
        self.m = None

    def __call__(self, pre):
        v = pre.detach().abs().flatten(1).min(1)[0].double()
        self.m = v if self.m is None else torch.minimum(self.m, v)
        return F.relu(pre)


def blocks_forward(blocks, x, relu=F.relu):
    for blk in blocks:
        y = relu(blk.bn1(blk.conv1(x)))
        x = relu(blk.bn2(blk.conv2(y)) + x)
    return x


def network_forward(model, x, relu=F.relu):
    """train.training_forward's torch path (nn.py:108-122) with the ReLUs passed in"""
    r, ph, vh = model.resnet, model.policy_head, model.value_head
    x = model.bn_input(x)
    x = relu(r.bn0(r.conv0(x)))
    x = blocks_forward(r.resblocks, x, relu)
    p = relu(ph.bn0(ph.conv0(x)))
    v = relu(vh.bn0(vh.conv0(x)))
    p = F.log_softmax(ph.fc(p.view(p.size(0), -1)), dim=1)
    v = relu(vh.fc0(v.view(v.size(0), -1)))
    return p, torch.tanh(vh.fc1(v))


def _collect(module, outs):
    res = dict(outs)
    res["grads"] = {k: p.grad.detach().double().cpu() for k, p in module.named_parameters()}
    res["stats"] = {k: v.detach().double().cpu() for k, v in module.state_dict().items() if "running" in k}
    res["nbt"] = sorted(set(int(v) for k, v in module.state_dict().items() if "num_batches_tracked" in k))
    return res


def torch_tower(blocks, x, gout, dtype, watch=None):
    """watch: module -> list of submodules whose (input, output gradient) are kept in res["captured"] (mutants)"""
    b = copy.deepcopy(blocks).to(dtype).train(True)
    got = capture(watch(b))[0] if watch else None
    xx = x.to(dtype).clone().requires_grad_(True)
    margin = _Margin()
    out = blocks_forward(b, xx, margin)
    out.backward(gout.to(dtype))
    res = _collect(b, {"out": out.detach().double(), "grad_x": xx.grad.double()})
    res["margin"], res["captured"], res["module"] = margin.m, got, b
    return res


def hip_tower(blocks, x, gout, max_batch=None, trainer=None):
    from dotsboxesaz_amd import train_tower

    class M:  # the container shape train_tower expects: model.resnet.resblocks / conv0
        pass
    b = copy.deepcopy(blocks).cuda().train(True)
    m = M()
    m.resnet = M()
    m.resnet.resblocks, m.resnet.conv0 = b, torch.nn.Conv2d(3, 64, 3)
    xx = x.cuda().clone().requires_grad_(True)
    assert train_tower.supported(m, xx)
    tr = trainer
    if tr is None and max_batch is not None:
        tr = train_tower.TowerTrainer(x.shape[2] - 1, x.shape[3] - 1, 64, len(b), max_batch)
    out = train_tower.resblocks_forward(m, xx, trainer=tr)
    out.backward(gout.cuda())
    torch.cuda.synchronize()
    res = _collect(b, {"out": out.detach().double().cpu(), "grad_x": xx.grad.double().cpu()})
    if tr is not None and trainer is None:
        tr.close()
    return res


def _loss(p, v, pi, z, scale):
    from dotsboxesaz_amd import train as T
    loss, _ = T.AlphaZeroLoss.tensors(p, v, pi, z)
    return loss * scale


def torch_net(model, x, pi, z, dtype, scale=1.0, watch=None):
    m = copy.deepcopy(model).to(dtype).train(True)
    got = capture(watch(m))[0] if watch else None
    margin = _Margin()
    p, v = network_forward(m, x.to(dtype), margin)
    loss = _loss(p, v, pi.to(dtype), z.to(dtype), scale)
    loss.backward()
    res = _collect(m, {"logp": p.detach().double(), "v": v.detach().double(), "loss": float(loss.detach())})
    res["margin"], res["captured"], res["module"] = margin.m, got, m
    return res


def hip_net(model, x, pi, z, scale=1.0, max_batch=None, trainer=None):
    from dotsboxesaz_amd import train_tower
    m = copy.deepcopy(model).cuda().train(True)
    xc = x.cuda()
    assert train_tower.net_supported(m, xc)
    tr = trainer
    if tr is None and max_batch is not None:
        tr = train_tower.TowerTrainer(x.shape[2] - 1, x.shape[3] - 1, 64, len(m.resnet.resblocks), max_batch)
    p, v = train_tower.network_forward(m, xc, trainer=tr)
    loss = _loss(p, v, pi.cuda(), z.cuda(), scale)
    loss.backward()
    torch.cuda.synchronize()
    res = _collect(m, {"logp": p.detach().double().cpu(), "v": v.detach().double().cpu(), "loss": float(loss.detach())})
    if tr is not None and trainer is None:
        tr.close()
    train_tower._trainers.clear()
    return res


def build_tower_case(case, max_tries=40):
    """(blocks, x, gout): decided cases as they are; random ones with the seed search of the existing tower test"""
    H, W = case.board[0] + 1, case.board[1] + 1
    blocks, dead = make_blocks(case.nb, 7 * case.nb + case.n, case.decided)
    if case.decided:
        return (blocks,) + tower_batch(case.n, H, W, case.n, dead)
    for seed in range(case.n, case.n + max_tries):
        x, gout = tower_batch(case.n, H, W, seed)
        b = copy.deepcopy(blocks).double().train(True)
        margin = _Margin()
        with torch.no_grad():
            blocks_forward(b, x.double(), margin)
        if float(margin.m.min()) >= UNSAFE:
            return blocks, x, gout
    raise AssertionError("no batch without a ReLU input at rounding distance from 0 in %d seeds" % max_tries)


def build_net_case(case, max_tries=40):
    """(model, x, pi, z)"""
    rows, cols = case.board
    A = 2 * (rows + 1) * (cols + 1)
    model = make_model(rows, cols, case.nb, 11 * case.nb + case.n, case.value_fc, case.decided)
    if case.decided:
        return (model,) + net_batch(rows, cols, case.n, A, 5 + case.n)
    for seed in range(5 + case.n, 5 + case.n + max_tries):
        x, pi, z = net_batch(rows, cols, case.n, A, seed)
        m = copy.deepcopy(model).double().train(True)
        margin = _Margin()
        with torch.no_grad():
            network_forward(m, x.double(), margin)
        if float(margin.m.min()) >= UNSAFE:
            return model, x, pi, z
    raise AssertionError("no batch without a ReLU input at rounding distance from 0 in %d seeds" % max_tries)


# ---------------------------------------------------------------------------------------------------------------------------
# the criterion
# ---------------------------------------------------------------------------------------------------------------------------
def rel(a, ref):
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


FLOORS_TOWER = {"out": 2e-6, "grad": 2e-6, "stat": 2e-6}
FLOORS_NET = {"out": 2e-6, "grad": 2e-5, "stat": 2e-6}
CONV_BIAS = ("conv0.bias", "conv1.bias", "conv2.bias")


def _layer_scale(k, g64):
    """largest float64 bn.weight gradient of the layer tensor k belongs to (None where the layer has no BatchNorm)"""
    parent, _, leaf = k.rsplit(".", 1)[0].rpartition(".")   # "resnet.resblocks.0" + "conv2" / "bn2"; "policy_head" + "bn0"
    if leaf[:-1] not in ("conv", "bn"):
        return None
    bn = (parent + "." if parent else "") + "bn" + leaf[-1]
    key = bn + ".weight"
    return float(g64[key].abs().max()) if key in g64 else None


def judge(hip, t32, t64, floors, K=4.0, outputs=("out", "grad_x")):
    """The criterion of the training tests: every output, gradient and running statistic of `hip` is as close to the float64
    truth as torch float32 is, e_hip <= max(K e_t32, floor) relative to the tensor's largest magnitude.  Conv biases in front of a
    training-mode BatchNorm (gradient exactly 0) are bounded absolutely against their weight gradient; so is every gradient
    tensor whose float64 maximum is below 1e-6 of its layer's bn.weight gradient maximum (analytically zero), against that scale.
    Returns (rows, failures, zero_rule): rows = [(name, e_hip, e_t32, e_hip / bound)]."""
    rows, zero_rule = [], []

    def one(name, a, b32, b64, floor):
        e_hip, e_t32 = rel(a, b64), rel(b32, b64)
        rows.append((name, e_hip, e_t32, e_hip / max(K * e_t32, floor)))

    for k in outputs:
        one(k, hip[k], t32[k], t64[k], floors["out"])
    if "loss" in t64:
        bound = max(K * abs(t32["loss"] - t64["loss"]), floors["out"] * abs(t64["loss"]))
        rows.append(("loss", abs(hip["loss"] - t64["loss"]), abs(t32["loss"] - t64["loss"]), abs(hip["loss"] - t64["loss"]) / bound))
    g64 = t64["grads"]
    for k in g64:
        if k.endswith(CONV_BIAS):
            scale = float(g64[k.replace("bias", "weight")].abs().max())
            rows.append((k, float(hip["grads"][k].abs().max()), 0.0, float(hip["grads"][k].abs().max()) / (1e-4 * scale + 1e-12)))
            continue
        scale = _layer_scale(k, g64)
        if scale is not None and float(g64[k].abs().max()) < 1e-6 * scale:
            zero_rule.append(k)
            rows.append((k, float(hip["grads"][k].abs().max()), float(t32["grads"][k].abs().max()),
                         float(hip["grads"][k].abs().max()) / (1e-4 * scale + 1e-12)))
            continue
        one(k, hip["grads"][k], t32["grads"][k], g64[k], floors["grad"])
    for k in t64["stats"]:
        one(k, hip["stats"][k], t32["stats"][k], t64["stats"][k], floors["stat"])
    failures = [r for r in rows if not r[3] <= 1.0]
    return rows, failures, zero_rule


# ---------------------------------------------------------------------------------------------------------------------------
# mutants: float32 results with one term of one sum left out (or added twice), re-formed from hooked tensors
# ---------------------------------------------------------------------------------------------------------------------------
def capture(module_list):
    """forward / backward hooks: {module: (input, grad_output)} filled during one forward + backward pass"""
    got, handles = {}, []
    for mod in module_list:
        def fwd(m, inp, out):
            got.setdefault(m, [None, None])[0] = inp[0].detach()

        def bwd(m, gin, gout):
            got.setdefault(m, [None, None])[1] = gout[0].detach()
        handles += [mod.register_forward_hook(fwd), mod.register_full_backward_hook(bwd)]
    return got, handles


def conv_wgrad(conv, x, g):
    return torch.nn.grad.conv2d_weight(x, conv.weight.shape, g, padding=conv.padding)


def mutate(res, key, delta):
    out = dict(res)
    out["grads"] = dict(res["grads"])
    out["grads"][key] = res["grads"][key] + delta.double()
    return out
