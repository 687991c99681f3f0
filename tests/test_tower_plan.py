"""csrc/tower_plan.h: the launch plan of the inference tower and tower_split, host-only C++ that csrc/nn.hip uses unchanged,
compiled with g++ and compared with the restatement oracle/nn_plan.py over every accepted board (CPU test)."""
import os
import shutil
import subprocess

import pytest

from oracle import nn_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dotsboxesaz_amd", "csrc")

CHANNELS = (16, 32, 64, 128)
HEADS = ((16, 8), (8, 8), (32, 64), (2, 1))     # (head_channels, value_fc)
HEADS_REFUSED = ((128, 64),)                    # ... and one the large boards cannot hold: the error path
CUS = (64, 256, 304)
FIELDS = ("S", "NT", "NTT", "S_small", "S_mid", "S_big", "c2", "S_c2", "NT_c2", "use_rem", "conv_lds", "conv_lds_c2")
CONSTANTS = ("MAXT", "MAXROWS", "MAXS", "WRING_BYTES", "LDS_BUDGET", "LDS_BUDGET_C2", "LDS_TOTAL", "REM_STATIC_LDS")

# stdin: one "rows cols" per line.  stdout: "K <the constants>", then per board x channels x precision x heads
#   "P rows cols channels precision hc vf <the fields>"   or   "E rows cols channels precision hc vf <error text>"
# and behind every P line, per compute-unit count and batch size n,  "S cus n mode n_full".
DRIVER = r"""
#include <cstdio>
#include "tower_plan.h"
int main()
{
    printf("K %d %d %d %zu %zu %zu %zu %zu\n", MAXT, MAXROWS, MAXS, TOWER_WRING_BYTES, TOWER_LDS_BUDGET, TOWER_LDS_BUDGET_C2,
           TOWER_LDS_TOTAL, TOWER_REM_STATIC_LDS);
    const int channels[4] = {16, 32, 64, 128}, heads[5][2] = {{16, 8}, {8, 8}, {32, 64}, {2, 1}, {128, 64}}, cus_list[3] = {64, 256, 304};
    int rows, cols;
    while (scanf("%d %d", &rows, &cols) == 2)
        for (int ch : channels)
            for (int prec = 0; prec < 2; prec++)
                for (const auto &h : heads) {
                    TowerPlan p;
                    const char *why = tower_plan_build(rows + 1, cols + 1, tower_padded_channels(ch, prec), h[0], h[1], prec, p);
                    if (why) { printf("E %d %d %d %d %d %d %s\n", rows, cols, ch, prec, h[0], h[1], why); continue; }
                    printf("P %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %zu\n", rows, cols, ch, prec, h[0], h[1], p.S, p.NT,
                           p.NTT, p.S_small, p.S_mid, p.S_big, p.c2, p.S_c2, p.NT_c2, p.use_rem, p.conv_lds, p.conv_lds_c2);
                    const int tails[4] = {p.S_small, p.S_mid, p.S_big, p.S_huge()};
                    for (int cus : cus_list) {
                        const int round = cus * p.S_main();
                        int ns[18] = {0, 1, round - 1, round, round + 1, 2 * round + 1}, nn = 6;
                        for (int s : tails)
                            for (int d = -1; d <= 1 && s > 0; d++) ns[nn++] = round + cus * s + d;
                        for (int i = 0; i < nn; i++) {
                            int n_full;
                            const int mode = tower_split(cus, p.S_main(), p.S_small, p.S_mid, p.S_big, p.S_huge(), ns[i], n_full);
                            printf("S %d %d %d %d\n", cus, ns[i], mode, n_full);
                        }
                    }
                }
    return 0;
}
"""


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    """what the driver prints: (constants, {case: fields or error text}, {case: [(cus, n, mode, n_full)]}), one process for all"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("tower_plan")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, src, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    boards = "".join("%d %d\n" % b for b in nn_plan.accepted_boards())
    r = subprocess.run([exe], input=boards, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    consts, plans, splits, cur = None, {}, {}, None
    for line in r.stdout.splitlines():
        t = line.split(" ", 7 if line[0] == "E" else -1)
        if t[0] == "S":
            cur.append(tuple(int(x) for x in t[1:]))
        elif t[0] == "K":
            consts = [int(x) for x in t[1:]]
        else:
            case = tuple(int(x) for x in t[1:7])
            plans[case] = t[7] if t[0] == "E" else [int(x) for x in t[7:]]
            if t[0] == "P":
                cur = splits[case] = []
    return consts, plans, splits


def _cases():
    for rows, cols in nn_plan.accepted_boards():
        for ch in CHANNELS:
            for prec in (0, 1):
                for hc, vf in HEADS + HEADS_REFUSED:
                    yield rows, cols, ch, prec, hc, vf


def _plan(case, cus=256):
    rows, cols, ch, prec, hc, vf = case
    try:
        return nn_plan.Plan(rows, cols, ch, hc, vf, prec, cus)
    except ValueError as e:
        return str(e)


def test_constants(header):
    assert header[0] == [getattr(nn_plan, k) for k in CONSTANTS]


def test_plan_fields_and_errors(header):
    """every field of TowerPlan, and every refusal, for 390 boards x 4 channel counts x 2 precisions x 4 head shapes (none of
    these 12 480 is refused) and a fifth head shape that is refused on the larger boards"""
    plans = header[1]
    assert len(nn_plan.accepted_boards()) == 390 and list(plans) == list(_cases())
    assert sum(1 for c in plans if c[4:] in HEADS) == 12480 and len(plans) == 12480 // 4 * 5
    refused = 0
    for case, got in plans.items():
        p = _plan(case)
        if isinstance(p, str):
            refused += 1
            assert got == p == "board / channels / head_channels too large for the LDS-resident tower", case
        else:
            assert got == [getattr(p, f) for f in FIELDS], case
    assert 0 < refused < len(plans) // 5 and all(c[4:] in HEADS_REFUSED for c, v in plans.items() if isinstance(v, str))


def test_split(header):
    """tower_split == Plan.split at the batch sizes around a round and around the limit of every tail body"""
    plans, splits = header[1], header[2]
    checked = 0
    for case, rows in splits.items():
        at = 0
        for cus in CUS:
            p = _plan(case, cus)
            ns = [0, 1, p.round - 1, p.round, p.round + 1, 2 * p.round + 1]
            for s in (p.S_small, p.S_mid, p.S_big, p.S_huge):
                if s > 0:
                    ns += [p.round + cus * s + d for d in (-1, 0, 1)]
            want = [(cus, n) + p.split(n) for n in ns]
            assert rows[at:at + len(want)] == want, (case, cus)
            at += len(want)
        assert at == len(rows), case
        checked += at
    assert len(splits) == sum(1 for v in plans.values() if not isinstance(v, str)) and checked > 18 * len(splits)
