"""playout_is_full (csrc/playout_cap.h), the one rule of playout cap randomization, run on the host: tests/playout_cap_main.cpp
compiled for the host only under AddressSanitizer and UBSan (no device code, no GPU, no preload) and compared with the pure-Python
Philox restatement of tests/playout_cap_ref.py -- and, where the library loads without a device, with dbaz_playout_cap_is_full."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
import playout_cap_ref as PR

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SEEDS = (7, 77, 0x0123456789ABCDEF)
GAMES = list(range(64)) + [2 ** 32 + 1]
PLIES = list(range(64))
PROBS = (0.0, 2.0 ** -32, 0.1, 0.25, 0.5, 1.0 - 2.0 ** -32, 1.0)


def test_check_value_of_the_header_comment():
    assert PR.philox4x32_10((1, 2, 3, 0x33333333), (7, 0))[0] == 1157962352
    assert [PR.thresh(p) for p in PROBS] == [0, 1, 429496729, 1 << 30, 1 << 31, (1 << 32) - 1, 1 << 32]


@pytest.fixture(scope="module")
def grid():
    """(cases, the reference's answers) of the whole grid"""
    cases = [(s, g, i, p) for s in SEEDS for p in PROBS for g in GAMES for i in PLIES]
    return cases, np.array([PR.is_full(*c) for c in cases])


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    assert os.path.exists(HIPCC), "hipcc builds the library too: it is part of the toolchain"
    exe = tmp_path_factory.mktemp("playout_cap") / "playout_cap"
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "dotsboxesaz_amd", "csrc"),
                    os.path.join(REPO, "tests", "playout_cap_main.cpp"), "-o", str(exe)], check=True)

    def run(cases):
        text = "".join("%x %d %d %s\n" % (s, g, i, float(p).hex()) for s, g, i, p in cases)
        r = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)  # 3: the check value; a sanitizer report has a message
        out = np.array([[int(t) for t in line.split()] for line in r.stdout.strip().split("\n")], dtype=np.uint64)
        assert len(out) == len(cases)
        return out
    return run


def test_header_on_the_host_vs_python_philox(rule, grid):
    cases, want = grid
    got = rule(cases)
    words = np.array([PR.philox4x32_10((g & 0xFFFFFFFF, g >> 32, i, PR.PURPOSE), (s & 0xFFFFFFFF, s >> 32))[0] for s, g, i, _ in cases], np.uint64)
    assert np.array_equal(got[:, 1], words)
    assert np.array_equal(got[:, 2], np.array([PR.thresh(p) for _, _, _, p in cases], np.uint64))
    assert np.array_equal(got[:, 0].astype(bool), want)
    probs = np.array([c[3] for c in cases])
    assert want[probs == 1.0].all() and not want[probs == 0.0].any()


def test_library_export_vs_python_philox(grid):
    """dbaz_playout_cap_is_full needs no device; a library that does not load without one is the ABI tests' finding, not this one's"""
    from dotsboxesaz_amd import _lib
    try:
        _lib.load()
    except (ImportError, OSError) as err:  # pragma: no cover
        pytest.fail("libdbaz_hip.so does not load here: %s" % err)
    from dotsboxesaz_amd import playout_cap as PC
    cases, want = grid
    n = len(GAMES) * len(PLIES)
    k = 0
    for s in SEEDS:
        for p in PROBS:
            got = PC.is_full(s, np.array(GAMES, np.int64)[:, None], np.array(PLIES)[None, :], p)
            assert got.shape == (len(GAMES), len(PLIES)) and got.dtype == bool
            assert np.array_equal(got.ravel(), want[k:k + n]), (s, p)
            k += n
    assert PC.is_full(7, 3, 5, 0.25) is PR.is_full(7, 3, 5, 0.25)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            PC.is_full(7, 0, 0, bad)
    assert _lib.load().dbaz_playout_cap_is_full(7, 0, 0, float("nan")) == -1


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", [0.25, 0.5, 0.1])
def test_frequency_of_full_searches(seed, p):
    """over games 0..63 x plies 0..63 the count of full draws lies within 5 sigma of n p (the nine cases: inside 1.8 sigma)"""
    n = 64 * 64
    k = sum(PR.is_full(seed, g, i, p) for g in range(64) for i in range(64))
    sigma = np.sqrt(n * p * (1 - p))
    print("seed %x p %.2f: %d full of %d, %.2f sigma" % (seed, p, k, n, (k - n * p) / sigma))
    assert abs(k - n * p) <= 5 * sigma


@pytest.mark.parametrize("seed", [7, 77])
def test_every_game_has_both_kinds_early(seed):
    for g in range(64):
        kinds = {PR.is_full(seed, g, i, 0.25) for i in range(24)}
        assert kinds == {True, False}, g
