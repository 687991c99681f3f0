"""Both heads of the network in logit space: what predict() returns against float64, where softmax and tanh squeeze nothing.

TEST INFRASTRUCTURE (oracle), beside nn_probe.py.  The probe head of that file reads the tower; its head is a selection (0 / 1
conv weights, an identity FC) and cannot see the heads' own arithmetic.  Here the network keeps its real heads:

    policy   z = fc(relu(bn0(conv0(t))))                     log p = log_softmax(z)
    value    u = fc1(relu(fc0(relu(bn0(conv0(t))))))          v = tanh(u)

evaluated once in torch float64 (the truth) and once in torch float32 (the yardstick), in the operation order of
nn_ref.ResNetZeroRef.forward.  The engine returns float32 (p, v); compared are

    E_p = max |log p - log p64|      over p64 >= 1e-30     (f32 softmax outputs keep their relative precision down to 1.2e-38)
    E_v = max |atanh v - u64|        over |v64| <= 0.99    (beyond, one f32 spacing of v times atanh' exceeds what is measured)

against  K * E_32 + allow:  E_32 is the same distance for torch float32's own z and u (BEFORE they are squeezed into a float32 p
and v), and allow is what returning float32 costs per element -- derived, not measured: one f32 spacing of p is at most 2^-23
relative, i.e. 2^-23 in log p; one f32 spacing of v is at most 2^-23 (|v| < 1), i.e. 2^-23 / (1 - v64^2) through atanh.

tests/test_nn_heads_ref.py shows on the CPU that the criterion has teeth at K = 16 (the mutants below), tests/test_hip_nn_heads.py
applies it to the engine.  SimpleNN (nn_ref.SimpleNNRef: v = tanh(value_fc(x))) goes through the same Reference."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nn_probe, nn_ref

K_MAX = nn_probe.K_MAX
# E <= K_HEAD[nn_precision] * E_32 + allow: nn_probe's rule -- twice the largest ratio (E - allow) / E_32 observed on the MI355X
# per arithmetic mode, rounded up to a power of two (EXPERIMENTS.md, section 1, holds the table); never above K_MAX
K_HEAD = {0: 16, 1: 16}
ALLOW_P = 2.0 ** -23
P_MIN, V_MAX = 1e-30, 0.99


def allow_v(v64):
    return 2.0 ** -23 / (1.0 - np.asarray(v64, np.float64) ** 2)


def _fold(conv, bn):
    """1x1 conv + eval BatchNorm as one affine map (what nn_commit folds): w [oc, C], b [oc]"""
    sc = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return conv.weight[:, :, 0, 0] * sc[:, None], (conv.bias - bn.running_mean) * sc + bn.bias


def _head_act(head, t, hook):
    """relu(bn0(conv0(t))) [n, hc, H, W]; with a hook in the folded form, hook(w [hc, C]) -> w"""
    if hook is None:
        return F.relu(head.bn0(head.conv0(t)))
    w, b = _fold(head.conv0, head.bn0)
    return F.relu(torch.einsum("oc,nchw->nohw", hook(w), t) + b[None, :, None, None])


def evaluate(model, X, dtype=torch.float64, policy_w=None, value_w=None, act=None, z_hook=None, h_hook=None):
    """dict of numpy float64 arrays: z [n, A], lp = log_softmax(z), u [n] (pre-tanh), v = tanh(u), ap / av (the flattened head
    activations [n, hc * HW]), h (value FC0 after its ReLU), every operation in `dtype`.  The hooks are the mutants' (None: the model as it is):
    policy_w / value_w(folded head conv weight) -> weight; act(ap, av) -> (ap, av); z_hook(z, ap, fc) -> z; h_hook(h) -> h."""
    m = copy.deepcopy(model).to(dtype)
    m.train(False)
    with torch.no_grad():
        x = torch.as_tensor(np.asarray(X), dtype=dtype)
        if hasattr(m, "resnet"):
            t = m.resnet(m.bn_input(x))
            ap = _head_act(m.policy_head, t, policy_w).reshape(x.size(0), -1)
            av = _head_act(m.value_head, t, value_w).reshape(x.size(0), -1)
            if act is not None:
                ap, av = act(ap, av)
            z = m.policy_head.fc(ap)
            if z_hook is not None:
                z = z_hook(z, ap, m.policy_head.fc)
            h = F.relu(m.value_head.fc0(av))
            if h_hook is not None:
                h = h_hook(h)
            u = m.value_head.fc1(h)
        else:       # SimpleNNRef: both heads are one Linear on the same vector
            for i in range(5):
                x = getattr(m, "bn%d" % i)(F.relu(getattr(m, "conv%d" % i)(x)))
            x = x.reshape(x.size(0), -1)
            x = m.bn_fc0(F.relu(m.fc0(x)))
            ap = av = m.bn_fc1(F.relu(m.fc1(x)))
            z, u, h = m.policy_fc(ap), m.value_fc(av), av
        out = dict(z=z, lp=F.log_softmax(z, dim=1), u=u.reshape(-1), v=torch.tanh(u).reshape(-1), ap=ap, av=av, h=h)
    return {k: t.double().numpy() for k, t in out.items()}


def as_f32_outputs(lp, u):
    """(p, v) float32 of logits evaluated some other way: exp and tanh in float64, rounded once (at most half a spacing)"""
    return np.exp(np.asarray(lp, np.float64)).astype(np.float32), np.tanh(np.asarray(u, np.float64)).astype(np.float32)


class Reference:
    """float64 and float32 of one (model, batch): z, log p, u, v, the two masks, the yardsticks E32_p and E32_v."""

    def __init__(self, model, X):
        self.model, self.X = model, np.asarray(X)
        self.f64 = evaluate(model, X, torch.float64)
        self.f32 = evaluate(model, X, torch.float32)
        self.z, self.lp, self.u, self.v = (self.f64[k] for k in ("z", "lp", "u", "v"))
        self.mask_p = np.exp(self.lp) >= P_MIN
        self.mask_v = np.abs(self.v) <= V_MAX
        self.allow_p = ALLOW_P
        self.allow_v = allow_v(self.v)
        self.e32_p = float(np.abs(self.f32["lp"] - self.lp)[self.mask_p].max()) if self.mask_p.any() else 0.0
        self.e32_v = float(np.abs(self.f32["u"] - self.u)[self.mask_v].max()) if self.mask_v.any() else 0.0

    def deltas(self, p, v):
        """(|log p - log p64| [n, A], |atanh v - u64| [n]) of float32 outputs; elements outside the masks are 0"""
        p, v = np.asarray(p, np.float64), np.asarray(v, np.float64).reshape(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            dp = np.where(self.mask_p, np.abs(np.log(p) - self.lp), 0.0)
            dv = np.where(self.mask_v, np.abs(np.arctanh(v) - self.u), 0.0)
        return dp, dv

    def errors(self, p, v):
        """E_p, E_v and the indices of the worst elements: (E_p, E_v, (sample, action), sample)"""
        dp, dv = self.deltas(p, v)
        ip = tuple(int(i) for i in np.unravel_index(dp.argmax(), dp.shape))
        iv = int(dv.argmax())
        return float(dp[ip]), float(dv[iv]), ip, iv

    def excess(self, p, v, k):
        """how far (p, v) is outside the criterion at K = k: (max E_p / (k E32_p + allow_p), max over the elements of
        |d atanh v| / (k E32_v + allow_v)); <= 1 passes"""
        dp, dv = self.deltas(p, v)
        return float(dp.max() / (k * self.e32_p + self.allow_p)), float((dv / (k * self.e32_v + self.allow_v)).max())

    def ratios(self, p, v):
        """what K_HEAD is set from: ((E_p - allow_p) / E32_p, max over the elements of (|d atanh v| - allow_v) / E32_v)"""
        dp, dv = self.deltas(p, v)
        rv = ((dv - self.allow_v)[self.mask_v] / self.e32_v).max() if self.mask_v.any() else 0.0
        return float((dp.max() - self.allow_p) / self.e32_p), float(rv)

    def mutant(self, **hooks):
        """float32 (p, v) of torch float32 damaged by the hooks"""
        r = evaluate(self.model, self.X, torch.float32, **hooks)
        return as_f32_outputs(r["lp"], r["u"])


def value_head_alive(model, X):
    """a condition on the inputs: the LAST 16-output tile of value FC0 holds an output that is nonzero (float64) in a quarter of
    the samples, and u moves from sample to sample -- behind dead ReLUs the value head is a constant, E32_v is 0 and a wrong FC0
    tile cannot be seen (value_fc = 1 is dead for every other seed)"""
    r = evaluate(model, X, torch.float64)
    h = r["h"]
    last = h[:, (h.shape[1] - 1) // 16 * 16:]
    return bool(((last > 0).mean(axis=0) >= 0.25).any() and r["u"].std() > 1e-3)


def trained_like_model(rows, cols, channels, blocks, head_channels, value_fc, seed):
    """a ResNetZeroRef with trained-like statistics (nn_ref.trained_like_ on 256 positions) whose value head is alive on those
    positions: the first of seed, seed + 1000, ... that is"""
    for s in range(seed, seed + 20000, 1000):
        torch.manual_seed(s)
        m = nn_ref.ResNetZeroRef(rows, cols, channels, blocks, head_channels=head_channels, value_fc=value_fc)
        X = nn_probe.positions(rows, cols, 256, s)
        nn_ref.trained_like_(m, X, s)
        if value_head_alive(m, X):
            return m
    raise ValueError("no seed gives a live value head")


# ---------------------------------------------------------------- mutants of torch fp32 (what a subtly wrong head would compute)
def _lo_lost(rows):
    def hook(w):
        w = w.clone()
        w[rows] = nn_probe.f16_round(w[rows])
        return w
    return hook


def mutant_policy_lo_lost(hc, tile=0):
    """(a) the `lo` half of the folded head-conv weights lost in one 16-output tile: its policy rows"""
    return dict(policy_w=_lo_lost(slice(tile * 16, min(hc, tile * 16 + 16))))


def mutant_value_lo_lost(hc):
    """(b) the same in the tile that holds the first value row (rows hc .. of [policy | value]): its value rows"""
    tile = hc // 16
    return dict(value_w=_lo_lost(slice(0, min(2 * hc, tile * 16 + 16) - hc)))


def live_k(ref):
    """the last K element of the policy FC whose float64 head activation is nonzero in at least half of the samples (the most
    often live one where there is none): behind a dead activation a dropped element cannot be seen"""
    live = (ref.f64["ap"] > 0).mean(axis=0)
    ks = np.nonzero(live >= 0.5)[0]
    return int(ks[-1]) if len(ks) else int(live.argmax())


def mutant_last_k_dropped(ref):
    """(c) the last (live) K element of the last policy output dropped"""
    k = live_k(ref)

    def hook(z, ap, fc):
        z = z.clone()
        z[:, -1] -= fc.weight[-1, k] * ap[:, k]
        return z
    return dict(z_hook=hook)


def mutant_fc0_tail_dropped():
    """(d) value FC0 outputs 16.. dropped (value_fc > 16: the second and later 16-output tiles)"""
    def hook(h):
        h = h.clone()
        h[:, 16:] = 0
        return h
    return dict(h_hook=hook)


def mutant_last_tile_bias_lost(A):
    """(e) the FC bias of the last 16-output tile of the policy lost"""
    o0 = (A - 1) // 16 * 16

    def hook(z, ap, fc):
        z = z.clone()
        z[:, o0:] -= fc.bias[o0:]
        return z
    return dict(z_hook=hook)


def mutant_clamp_off_by_one(S):
    """(f) sample ns - 1 of every workgroup of S samples gets the head activations of sample ns - 2: min(jrow, ns - 1) off by one"""
    def hook(ap, av):
        ap, av = ap.clone(), av.clone()
        n = ap.shape[0]
        for w0 in range(0, n, S):
            ns = min(S, n - w0)
            if ns >= 2:
                ap[w0 + ns - 1], av[w0 + ns - 1] = ap[w0 + ns - 2], av[w0 + ns - 2]
        return ap, av
    return dict(act=hook)
