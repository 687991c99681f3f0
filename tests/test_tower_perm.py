"""csrc/tower_perm.h: the row table of the two-cout-tile tower body (which LDS row each lane of each position tile processes)
and the taps its edge tiles drop.  Host-only C++, checked through a small g++ driver (CPU test)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dotsboxesaz_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "tower_perm.h"
int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    int tab[TOWER_PERM_ROWS];
    const int dropped = tower_perm_build(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), tab);
    printf("%d\n", dropped);
    for (int T = 0; T < TOWER_PERM_TILES; T++) printf("%d%c", dropped ? tower_perm_drop(T) : 0, T == 15 ? '\n' : ' ');
    for (int i = 0; i < TOWER_PERM_ROWS; i++) printf("%d%c", tab[i], i == TOWER_PERM_ROWS - 1 ? '\n' : ' ');
    return 0;
}
"""

TOP, BOTTOM, LEFT, RIGHT = 0o007, 0o700, 0o111, 0o444
# wave pair g owns tiles 4g .. 4g+3; its tiles 0 and 1 are the edge tiles
PATTERN = [TOP, LEFT, 0, 0, TOP, RIGHT, 0, 0, BOTTOM, RIGHT, 0, 0, BOTTOM, LEFT, 0, 0]
GEOMETRIES = [(7, 7, 5), (4, 4, 15), (6, 7, 6), (8, 8, 4), (10, 10, 2)]
MUST_MEET = {(7, 7, 5), (4, 4, 15)}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("tower_perm")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return exe


def _table(exe, H, W, S):
    r = subprocess.run([exe, str(H), str(W), str(S)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    return int(lines[0]), [int(x) for x in lines[1].split()], [int(x) for x in lines[2].split()]


def _inside(H, W, y, x):
    m = 0
    for tap in range(9):
        yy, xx = y + tap // 3 - 1, x + tap % 3 - 1
        if 0 <= yy < H and 0 <= xx < W:
            m |= 1 << tap
    return m


@pytest.mark.parametrize("H,W,S", GEOMETRIES)
def test_row_table(driver, H, W, S):
    dropped, drops, tab = _table(driver, H, W, S)
    assert len(tab) == 256 and sorted(tab) == list(range(256))
    if (H, W, S) in MUST_MEET:
        assert dropped == 24
    if dropped:
        assert dropped == 24 and drops == PATTERN
        HW = H * W
        for T in range(16):
            for j in range(16):
                r = tab[T * 16 + j]
                if r < S * HW:  # a real row: every tap its tile drops lies outside the image
                    p = r % HW
                    assert _inside(H, W, p // W, p % W) & drops[T] == 0, (T, j, r)
    else:
        assert tab == list(range(256)) and drops == [0] * 16


def test_full_tiles_without_padding_cannot_meet_the_pattern(driver):
    """64 positions, 4 samples: 256 real rows, 24 one-border rows and 16 corners for 32 slots of every border."""
    dropped, drops, tab = _table(driver, 8, 8, 4)
    assert dropped == 0 and tab == list(range(256))


def test_other_tile_counts_keep_the_identity(driver):
    for H, W, S in ((7, 7, 3), (4, 4, 16), (10, 10, 3)):  # 10, 16 tiles of 256 rows, 300 rows
        dropped, _, tab = _table(driver, H, W, S)
        if (H, W, S) != (4, 4, 16):
            assert dropped == 0 and tab == list(range(256))
        else:
            assert sorted(tab) == list(range(256))
