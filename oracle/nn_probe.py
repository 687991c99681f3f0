"""Probe head: makes the OUTPUT OF THE TOWER observable through predict(), element by element.

TEST INFRASTRUCTURE (oracle).  dbaz_nn_predict returns only (softmax p, tanh v).  With the policy head below, p is the tower
output itself:
  policy_head.conv0  1x1 selection: head channel j = tower channel c0 + j (weight 1.0, bias 0)
  policy_head.bn0    running_mean 0, running_var 1, beta 0, gamma s (a power of two): head = s' * t, s' = s / sqrt(1 + eps);
                     the head's ReLU changes nothing, t >= 0 is the post-ReLU output of the last block
  policy_head.fc     selection: logit j * HW + q = head channel j at position q for j in {0, 1}, bias 0
so that  log p = log_softmax(s' * t[c0:c0+2, :])  over the 2 * HW logits, and C / 2 probes read every element of t.  The value
head keeps the model's weights.

The truth is the float64 torch tower, evaluated ONCE per (model, batch); every probe's expected log p comes from that t in
numpy.  The yardstick is torch's own float32 tower against the same truth, with the head formula carried out in float32.

The criterion (tests/test_hip_nn_elementwise.py):  E = max |log p - log p_f64| over the compared elements; E_test <= k * E_32.
tests/test_nn_probe_ref.py shows on the CPU that it has teeth: torch fp32 with a lost `lo` half in one cout tile or one position
tile, or with one dropped tap, fails it at k = 16 by a factor of 4 or more."""
import copy
import math

import numpy as np
import torch
import torch.nn.functional as F

# E_test <= K[nn_precision] * E_32: twice the largest ratio observed on the MI355X per arithmetic mode, rounded up to a power
# of two (EXPERIMENTS.md holds the table); 16 is the most the criterion allows
K = {0: 8, 1: 8}
K_MAX = 16
BN_EPS = 1e-5
LOGIT_MAX = 8.0


def positions(rows, cols, n, seed):
    """Feature planes of the kind get_features produces: 0/1 edge planes from empty to full boards, integer plane 2."""
    rng = np.random.RandomState(seed)
    X = (rng.rand(n, 3, rows + 1, cols + 1) < rng.rand(n, 1, 1, 1)).astype(np.float32)
    X[:, 2] = rng.randint(-1, rows * cols + 1, size=(n, 1, 1))
    return X


def tower(model, X, dtype=torch.float64, weight_hook=None, act_hook=None, out_hook=None):
    """t = post-ReLU output of the last block, numpy [n, C, H, W], evaluated in `dtype` (float64: the truth; float32: torch's own
    evaluation).  The hooks mutate the LAST block (test_nn_probe_ref.py): weight_hook(conv2.weight) -> weight,
    act_hook(conv2's input) -> input, out_hook(conv2's output, conv2's input, weight) -> output."""
    m = copy.deepcopy(model).to(dtype)
    m.train(False)
    with torch.no_grad():
        x = m.bn_input(torch.as_tensor(np.asarray(X), dtype=dtype))
        r = m.resnet
        x = F.relu(r.bn0(r.conv0(x)))
        for i, blk in enumerate(r.resblocks):
            last = i == len(r.resblocks) - 1
            y = F.relu(blk.bn1(blk.conv1(x)))
            w = blk.conv2.weight
            if last and weight_hook is not None:
                w = weight_hook(w)
            if last and act_hook is not None:
                y = act_hook(y)
            z = F.conv2d(y, w, blk.conv2.bias, padding=1)
            if last and out_hook is not None:
                z = out_hook(z, y, w)
            x = F.relu(blk.bn2(z) + x)
    return x.numpy()


def scale_for(t):
    """the power of two s with s * max(t) in (LOGIT_MAX / 2, LOGIT_MAX] (at most 2^10: a pair of dead channels)"""
    return 2.0 ** min(10, math.floor(math.log2(LOGIT_MAX / max(float(np.max(t)), 1e-30))))


def probe_offsets(channels):
    return list(range(0, channels, 2))


def probe_state_dict(model, c0, s):
    """the model's state_dict with the policy head replaced by the probe of tower channels c0, c0 + 1"""
    c = model.cfg
    C, hc, HW = c["channels"], c["head_channels"], (c["rows"] + 1) * (c["cols"] + 1)
    assert hc >= 2 and 0 <= c0 and c0 + 2 <= C
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    w = torch.zeros(hc, C, 1, 1)
    for j in range(min(hc, C - c0)):
        w[j, c0 + j, 0, 0] = 1.0
    fc = torch.zeros(2 * HW, hc * HW)
    idx = torch.arange(2 * HW)
    fc[idx, idx] = 1.0      # x.reshape(n, -1) is channel-major: input j * HW + q = head channel j at position q
    sd["policy_head.conv0.weight"] = w
    sd["policy_head.conv0.bias"] = torch.zeros(hc)
    sd["policy_head.bn0.running_mean"] = torch.zeros(hc)
    sd["policy_head.bn0.running_var"] = torch.ones(hc)
    sd["policy_head.bn0.weight"] = torch.full((hc,), float(s))
    sd["policy_head.bn0.bias"] = torch.zeros(hc)
    sd["policy_head.fc.weight"] = fc
    sd["policy_head.fc.bias"] = torch.zeros(2 * HW)
    return sd


def _log_softmax(z):
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def expected_log_p(t, c0, s, dtype=np.float64):
    """log_softmax(s' * t[:, c0:c0+2]) [n, 2 * HW], every operation in `dtype`"""
    t = np.asarray(t, dtype=dtype)
    n = t.shape[0]
    sp = dtype(dtype(s) / np.sqrt(dtype(1.0) + dtype(BN_EPS)))
    return _log_softmax(t[:, c0:c0 + 2].reshape(n, -1) * sp).astype(np.float64)


def log_of_p(p):
    """log of a float32 softmax output, in float64 (the probe keeps every p above e^-8 / (2 HW): far inside f32's normal range)"""
    return np.log(np.asarray(p, dtype=np.float64))


def errors(lp, lp64):
    """max |d log p| over the compared elements"""
    return float(np.abs(np.asarray(lp, np.float64) - lp64).max())


class Reference:
    """t64 and t32 of one (model, batch), and what every probe must return for it."""

    def __init__(self, model, X):
        self.t64 = tower(model, X, torch.float64)
        self.t32 = tower(model, X, torch.float32)
        self.channels = self.t64.shape[1]
        # one scale per probe, from the two channels it reads: every probe uses the range of logits it is allowed
        self.s = {c0: scale_for(self.t64[:, c0:c0 + 2]) for c0 in probe_offsets(self.channels)}
        self._lp64 = {}

    def lp64(self, c0):
        if c0 not in self._lp64:
            self._lp64[c0] = expected_log_p(self.t64, c0, self.s[c0], np.float64)
        return self._lp64[c0]

    def e32(self, c0s=None):
        """the yardstick: torch fp32's own max |d log p| over the probes c0s (all of them by default)"""
        c0s = probe_offsets(self.channels) if c0s is None else c0s
        return max(errors(expected_log_p(self.t32, c0, self.s[c0], np.float32), self.lp64(c0)) for c0 in c0s)

    def per_probe(self, t, c0s=None):
        """{c0: max |d log p|} of a tower output t evaluated some other way (float32 head arithmetic)"""
        c0s = probe_offsets(self.channels) if c0s is None else c0s
        return {c0: errors(expected_log_p(t, c0, self.s[c0], np.float32), self.lp64(c0)) for c0 in c0s}


# ---------------------------------------------------------------- mutants of torch fp32 (what a subtly wrong kernel would compute)
def f16_round(x):
    return x.to(torch.float16).to(x.dtype)


def mutant_weight_lo_lost(c_lo=16, c_hi=32):
    """the `lo` half of the (hi, lo) weight pair lost in one cout tile of the last conv2"""
    def hook(w):
        w = w.clone()
        w[c_lo:c_hi] = f16_round(w[c_lo:c_hi])
        return w
    return dict(weight_hook=hook)


def mutant_act_lo_lost(S=4, tile=1):
    """the `lo` half of the activations lost in one 16-position tile of every workgroup of S samples (rows tile * 16 .. + 15 of
    the workgroup's sample-major rows)"""
    def hook(y):
        n, C, H, W = y.shape
        rows = y.permute(0, 2, 3, 1).reshape(n * H * W, C).clone()
        for r0 in range(tile * 16, n * H * W, S * H * W):
            rows[r0:r0 + 16] = f16_round(rows[r0:r0 + 16])
        return rows.reshape(n, H, W, C).permute(0, 3, 1, 2).contiguous()
    return dict(act_hook=hook)


def mutant_dropped_tap(py=1, px=1, sample=0):
    """one corner tap (dy = dx = -1) dropped at one position of one sample"""
    def hook(z, y, w):
        z = z.clone()
        z[sample, :, py, px] -= w[:, :, 0, 0] @ y[sample, :, py - 1, px - 1]
        return z
    return dict(out_hook=hook)
