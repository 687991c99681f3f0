"""The (hi, lo) split of the f16x3 tower (csrc/h3_split.h) on EVERY f32 bit pattern.

The shipped split forms lo = rn_f16(x - hi) with one v_fma_mixlo_f16 / v_fma_mixhi_f16 (inline assembly); the reference spelling
in the same header widens hi, subtracts in f32 and rounds again.  tests/h3_split_sweep.hip is a stand-alone program whose one
kernel sends all 2^32 patterns through both -- NaNs of every payload, +-inf, f32 subnormals, values whose lo is an f16 subnormal,
values above 65 504 -- and counts the inputs whose hi or lo half differs (two NaNs count as equal).  It also counts the inputs with
a non-zero lo, a subnormal lo and an infinite hi, so that the sweep provably visited those classes.  The program is compiled here
and started as a child process."""
import os
import subprocess

import pytest

from dotsboxesaz_amd import build as hip_build

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_split_equals_reference_on_every_f32(tmp_path):
    exe = str(tmp_path / "h3_split_sweep")
    cmd = [hip_build.HIPCC, "--offload-arch=" + hip_build.ARCH, "-O3", "-std=c++17", "-I", hip_build.CSRC,
           os.path.join(HERE, "h3_split_sweep.hip"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    words = r.stdout.split()
    got = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    print(got)
    assert got["patterns"] == 1 << 32
    assert got["nonzero_lo"] > 0 and got["subnormal_lo"] > 0 and got["inf_hi"] > 0, got
    assert got["mismatch"] == 0, got
