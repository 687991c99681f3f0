#!/bin/bash
# Diagnostic: builds a STAMPED copy of the library (never the shipped one) and prints where a
# k_tower wave spends its cycles.  Usage on the GPU box: bash tools/stamp_build_run.sh
# (DBAZ_LIB=build/stamp_p2/libdbaz_hip.so bash tools/stamp_build_run.sh: another stamped build, see tools/build_stamp.sh)
set -e
cd "$(dirname "$0")/.."
# the stamped library is built in the build container: tools/build_stamp.sh -> build/stamp/libdbaz_hip.so
python - <<'PY'
import ctypes as C, numpy as np, torch, sys
sys.path.insert(0, ".")
from dotsboxesaz_amd import _lib
import os
_lib.LIB_PATH = os.environ.get("DBAZ_LIB") or "build/stamp/libdbaz_hip.so"
print("library", _lib.LIB_PATH)
from dotsboxesaz_amd.engine import Engine
from dotsboxesaz_amd import nn as dnn
e = Engine(6, 6, 8192, evaluator="resnet", nn_precision=1)
torch.manual_seed(0)
m = dnn.ResNetZero(dnn.resnet_params(6, 6))
e.load_state_dict(m.state_dict(), "resnet", **m.shape)
X = np.random.RandomState(0).randint(0, 2, size=(8192, 3, 7, 7)).astype(np.float32)
for _ in range(60):   # ~0.2 s of back-to-back launches so that the clock settles
    e.predict(X)
n_wg = 2048
out = np.zeros((n_wg, 8, 16), np.uint64)  # STAMP_WORDS of csrc/nn.hip
L = _lib.load()
L.dbaz_debug_read_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
rc = L.dbaz_debug_read_stamps(e.h, out.ctypes.data, n_wg)
o = out.astype(np.float64)
# only workgroups of the MAIN launch that ran: rows of idle entries are zero, and the first `cus` rows were overwritten by a
# tail launch (smaller workgroups) whenever the batch left a tail
ran = o[:, 0, 4] > 0
ran[:256] = False
o = o[ran]
tot = o[..., 4]
print("rc", rc, "waves", (tot > 0).sum())
names = ["prologue(loads)", "main loop", "epilogue", "barrier wait", "layers total"]
for i, nme in enumerate(names):
    print("%-18s mean %10.0f cycles/wave   %5.1f %% of layers total" % (nme, o[..., i].mean(), 100 * o[..., i].mean() / tot.mean()))
print("16x16x32, two cout tiles per wave, 5 samples per workgroup; per layer: total %.0f, main %.0f (MFMA floor per wave: 18 steps x 24 MFMAs x 16 = %d; per SIMD twice that)" % (tot.mean() / 40, o[..., 1].mean() / 40, 18 * 24 * 16))
for w in range(8):
    print("wave", w, ["%.0f" % (o[:, w, i].mean() / 40) for i in range(5)])
# step ends of the two-cout-tile body's K-loop (18 steps, 17 step barriers per layer).  Every interval ends with a stamp, which
# drains lgkmcnt itself: its cost (two stamps back to back, once per layer) is taken off.  The first interval therefore holds
# the wait for the step's LDS reads as well, and the stamped loop is slower than the shipped one: the activation reads of the
# next step are drained at every step end instead of flying across the barrier.
st = o[..., 12].mean() / 40
print("one stamp costs %.0f cycles" % st)
for i, nme, cnt in ((10, "last MFMA issued -> return from the step-end s_waitcnt", 18), (11, "from there -> return from s_barrier", 17)):
    per = o[..., i].mean() / 40
    print("%-56s %6.0f cycles per layer and wave, %6.0f without the stamps" % (nme, per, per - cnt * st))
print("(MFMA floor per SIMD and layer: 2 waves x 360 MFMAs x 16 = 11520 cycles)")
for w in range(8):
    print("wave", w, "step-end wait / step barrier per layer, stamps taken off:",
          ["%.0f" % (o[:, w, i].mean() / 40 - c * o[:, w, 12].mean() / 40) for i, c in ((10, 18), (11, 17))])
# step heads: return from the step barrier (step 0: the layer's first fragment reads are issued) -> the step's first MFMA is
# issued, 18 per layer, one stamp's cost taken off each.  The stamp drains lgkmcnt, so behind a head that stands at the start of
# its step the interval holds the return of the four ring reads too (an upper bound of the head's cost); a stream whose head
# stands behind its hi*hi phase (DBAZ_STAGGER) has nothing but the stamp there.
print("step heads (step barrier -> first MFMA issued), 18 per layer; cycles per layer and wave, raw / stamps taken off / per step:")
for w in range(8):
    raw = o[:, w, 13].mean() / 40
    net = raw - 18 * o[:, w, 12].mean() / 40
    print("wave", w, "head %6.0f / %6.0f / %5.1f   = %4.1f %% of the layer" % (raw, net, net / 18, 100 * net / (o[:, w, 4].mean() / 40)))
whole = o[..., 7].mean()
print("whole workgroup %.0f cycles: conv0 phase %.0f (%.1f %%), 40 layers %.0f (%.1f %%), head convs + output %.0f (%.1f %%)"
      % (whole, o[..., 5].mean(), 100 * o[..., 5].mean() / whole, tot.mean(), 100 * tot.mean() / whole, o[..., 6].mean(),
         100 * o[..., 6].mean() / whole))
rt = o[..., 8]
ok = rt > 0
print("in-kernel clock (shader cycles / 100 MHz realtime ticks), median over workgroups: %.0f MHz" % (np.median(o[..., 7][ok] / rt[ok]) * 100))
PY
