"""csrc/train_plan.h: the launch plan of the training step, host-only C++ that csrc/train.hip and csrc/train_net.hip use unchanged,
compiled with g++ and compared with the restatement oracle/train_plan.py over every board the size check accepts (CPU test).

Also here, because tests/test_hip_train_classes.py (GPU) leans on them: the case tables reach every launch class at 64, 256 and
304 compute units; the decided models keep every ReLU input of the float64 reference at least 1.0 from zero, for every sample;
and the criterion of the training tests rejects float32 results with one term of one sum damaged."""
import functools
import os
import shutil
import subprocess

import pytest
import torch

from oracle import train_cases as TC
from oracle import train_plan as TP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dotsboxesaz_amd", "csrc")
CUS = (64, 256, 304)

# stdin: "rows cols cus n" per line.  stdout: first "K <the constants>", then per line
#   n == 0:  "P <the plan's fields>"  or  "E <error text>"
#   n > 0:   "L <the launch sizes of a batch of n>"
DRIVER = r"""
#include <cstdio>
#include "train_plan.h"
int main()
{
    printf("K %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %zu\n", TT, TC, TL_MAX, RED_BLOCKS, WG_MAXLD, WH_SB, NET_WG, NET_HB, NET_OB,
           NET_SB, STEM_S, FC_SPLITS, FCF_SPLITS, HW_SPLITS, STEM_SPLITS, TRAIN_MAX_POSITIONS, TRAIN_CONV_ROWS, TRAIN_WH_ROWS, TRAIN_WH_LDS_BUDGET,
           TRAIN_LDS_LIMIT);
    int rows, cols, cus, n;
    while (scanf("%d %d %d %d", &rows, &cols, &cus, &n) == 4) {
        TrainPlan p;
        char why[256];
        const bool ok = train_plan_build(rows, cols, p, why, sizeof(why));
        if (n == 0) {
            if (ok) printf("P %d %d %d %d %d %d %zu %zu\n", p.H, p.W, p.HW, p.S, p.Swh, p.pwc, p.conv_lds, p.wgrad_h3_lds);
            else printf("E %s\n", why);
            continue;
        }
        if (!ok) return 1;
        const long long M = (long long)n * p.HW;
        const int hs = net_head_wgrad_splits(M), KF = p.HW * 32;
        printf("L %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", train_conv_grid(p, n), train_wgrad_chunks(p, n),
               train_wgrad_grid(p, cus, n), red_blocks(M), bn_apply_passes(M * 16), bn_apply_grid(M * 16), net_stem_grid(n), net_head_conv_grid(M),
               net_head_bn_apply_grid(M), net_head_out_grid(n), net_head_rows_grid(M), net_head_bwd_data_grid(M), hs, net_stem_wgrad_splits(M),
               gemm_kchunk((int)M, hs), gemm_splits((int)M, hs), gemm_kchunk(n, FC_SPLITS), gemm_splits(n, FC_SPLITS), gemm_kchunk(KF, FCF_SPLITS),
               gemm_splits(KF, FCF_SPLITS));
    }
    return 0;
}
"""

# the boards the issue names: k_wgrad_h3's images of ONE sample exceed 160 KB
LDS_REFUSED = ([(1, c) for c in range(79, 98)] + [(2, c) for c in range(60, 65)] + [(3, 47), (3, 48)] + [(r, 1) for r in range(87, 98)])


def _plan(rows, cols, cus=256):
    try:
        return TP.Plan(rows, cols, cus)
    except ValueError as e:
        return str(e)


def _queries():
    q = []
    for rows, cols in TP.accepted_boards():
        q.append((rows, cols, 0, 0))
        if isinstance(_plan(rows, cols), str):
            continue
        for cus in CUS:
            q += [(rows, cols, cus, n) for n in TP.Plan(rows, cols, cus).thresholds()]
    return q + [(14, 14, 0, 0), (0, 5, 0, 0), (97, 97, 0, 0)]


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    """(constants, [(query, answer)]) of one run of the driver"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("train_plan")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, src, "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    q = _queries()
    r = subprocess.run([exe], input="".join("%d %d %d %d\n" % t for t in q), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0][0] == "K" and len(lines) == len(q) + 1
    return [int(x) for x in lines[0].split()[1:]], list(zip(q, lines[1:]))


def test_constants(header):
    assert header[0] == [getattr(TP, k) for k in TP.CONSTANTS]
    assert TP.WH_ROWS == TP.WG_MAXLD * TP.TT // 32


def test_plan_fields_refusals_and_launch_sizes(header):
    """every field of TrainPlan, every refusal with its text, and every grid / chunk count / split-K step at the batch sizes around every
    threshold, for three compute-unit counts"""
    plans = refused = sizes = 0
    for (rows, cols, cus, n), line in header[1]:
        p = _plan(rows, cols, cus or 256)
        if n == 0 and isinstance(p, str):
            assert line == "E " + p, (rows, cols)
            refused += 1
        elif n == 0:
            assert line[0] == "P" and [int(x) for x in line.split()[1:]] == p.fields(), (rows, cols)
            plans += 1
        else:
            assert line[0] == "L" and [int(x) for x in line.split()[1:]] == p.launch_sizes(n), (rows, cols, cus, n)
            sizes += 1
    assert plans == len(TP.accepted_boards()) - len(LDS_REFUSED) and refused == len(LDS_REFUSED) + 3 and sizes > 100 * plans


def test_the_header_refuses_exactly_the_boards_whose_lds_exceeds_the_limit(header):
    answers = {q[:2]: line for q, line in header[1] if q[3] == 0}
    over = [b for b in TP.accepted_boards() if TP.wh_lds_bytes(1, b[0] + 1, b[1] + 1) > TP.LDS_LIMIT]
    assert sorted(over) == sorted(LDS_REFUSED) and len(over) == 37
    assert TP.wh_lds_bytes(1, 2, 98) == 209328
    for b in TP.accepted_boards():
        if b in over:
            assert answers[b].startswith("E board %dx%d unsupported" % b) and ("%d bytes of LDS" % TP.wh_lds_bytes(1, b[0] + 1, b[1] + 1)) in answers[b]
        else:
            assert answers[b][0] == "P" and TP.Plan(*b).wgrad_h3_lds <= TP.LDS_LIMIT and TP.Plan(*b).conv_lds <= TP.LDS_LIMIT
    assert answers[(14, 14)].startswith("E board 14x14 unsupported") and "at most 196 positions" in answers[(14, 14)]


@pytest.mark.parametrize("cus", CUS)
def test_case_tables_reach_every_launch_class(cus):
    tables = {"tower": {c.id: c for c in TC.tower_cases(cus)}, "net": {c.id: c for c in TC.net_cases(cus)}}
    assert [c.id for c in TC.tower_cases(cus)] == [c.id for c in TC.tower_cases(256)]     # (the GPU test's parameter ids)
    assert [c.id for c in TC.net_cases(cus)] == [c.id for c in TC.net_cases(256)]
    preds = TC.class_predicates(cus)
    assert len(preds) >= 27
    for name, (tab, cid, pred) in preds.items():
        c = tables[tab][cid]
        assert pred(TP.Plan(c.board[0], c.board[1], cus), c), (name, cid, c.n)
    # every case is there for a class, and large cases are decided
    assert set((t, c) for t, c, _ in preds.values()) == set(("tower", i) for i in tables["tower"]) | set(("net", i) for i in tables["net"])
    for tab, net in (("tower", False), ("net", True)):
        for c in tables[tab].values():
            assert c.decided or TC.relu_inputs(c, net) < TC.BIG_RELU_INPUTS, c.id


def test_network_forward_restates_training_forward():
    """oracle/train_cases.network_forward (the float64 / float32 reference of the class tests) == train.training_forward's torch path, bit for bit"""
    from dotsboxesaz_amd import train as T
    model = TC.make_model(2, 3, 1, 5).train(True)
    x = TC.net_batch(2, 3, 9, 24, 1)[0]
    import copy
    a, b = copy.deepcopy(model), copy.deepcopy(model)
    pa, va = TC.network_forward(a, x)
    pb, vb = T.training_forward(b, x, hip_tower=False)
    assert torch.equal(pa, pb) and torch.equal(va, vb)


# ---- decided models and mutants: one float64 and one float32 pass per large case, shared
LARGE = [("tower", c.id) for c in TC.tower_cases(256) if c.decided] + [("net", c.id) for c in TC.net_cases(256) if c.decided]


def _watch_tower(b):
    return [b[0].conv2, b[0].bn1]


def _watch_net(m):
    blk = m.resnet.resblocks[0]
    return [blk.conv2, blk.bn1, m.policy_head.fc, m.policy_head.conv0]


@functools.lru_cache(maxsize=None)
def reference(tab, cid):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    if tab == "tower":
        case = {c.id: c for c in TC.tower_cases(256)}[cid]
        blocks, x, gout = TC.build_tower_case(case)
        return case, TC.torch_tower(blocks, x, gout, torch.float64), TC.torch_tower(blocks, x, gout, torch.float32, watch=_watch_tower)
    case = {c.id: c for c in TC.net_cases(256)}[cid]
    model, x, pi, z = TC.build_net_case(case)
    return case, TC.torch_net(model, x, pi, z, torch.float64), TC.torch_net(model, x, pi, z, torch.float32, watch=_watch_net)


@pytest.mark.parametrize("tab,cid", LARGE)
def test_decided_models_keep_every_relu_input_away_from_zero(tab, cid):
    """the float64 reference's smallest |ReLU input| is at least 1.0 for EVERY sample (no sample is left out of any comparison: judge
    compares whole tensors), and the value head stays out of tanh's saturation"""
    case, t64, _ = reference(tab, cid)
    assert t64["margin"].shape == (case.n,) and float(t64["margin"].min()) >= TC.DECIDED_MIN, float(t64["margin"].min())
    if tab == "net":
        assert float((t64["v"].abs() < 0.9).double().mean()) >= 0.9 and float(t64["v"].abs().max()) > 0.05


def mutants(tab, case, t32):
    """{name: mutated float32 result}: one term of one sum wrong, re-formed from the hooked (input, output gradient) pairs"""
    m, got = t32["module"], t32["captured"]
    pre = "" if tab == "tower" else "resnet.resblocks."
    blk = m[0] if tab == "tower" else m.resnet.resblocks[0]
    p = TP.Plan(case.board[0], case.board[1], 256)
    out = {}
    xin, g = got[blk.conv2]
    out["last sample missing from a conv weight gradient"] = TC.mutate(t32, pre + "0.conv2.weight", -TC.conv_wgrad(blk.conv2, xin[-1:], g[-1:]))
    last, grid = p.wgrad_chunks(case.n) - 1, p.wgrad_grid(case.n)
    ns = case.n - last * p.Swh
    if ns < p.Swh and last - grid >= 0:
        stale = slice((last - grid) * p.Swh + ns, (last - grid + 1) * p.Swh)
        out["previous chunk's samples in place of the partial last chunk's zeros"] = TC.mutate(
            t32, pre + "0.conv2.weight", TC.conv_wgrad(blk.conv2, xin[stale], g[stale]))
    y, gy = got[blk.bn1]
    rows_y, rows_g = y.permute(0, 2, 3, 1).reshape(-1, 64), gy.permute(0, 2, 3, 1).reshape(-1, 64)
    yhat = (rows_y - rows_y.mean(0)) / torch.sqrt(rows_y.var(0, unbiased=False) + 1e-5)
    mut = TC.mutate(t32, pre + "0.bn1.weight", -(rows_g[-32:] * yhat[-32:]).sum(0))
    out["last 32 rows missing from a layer's dgamma / dbeta"] = TC.mutate(mut, pre + "0.bn1.bias", -rows_g[-32:].sum(0))
    if tab == "net":
        h, gl = got[m.policy_head.fc]
        out["last batch row missing from the policy FC weight gradient"] = TC.mutate(t32, "policy_head.fc.weight", -(gl[-1:].t() @ h[-1:]))
        a, ga = got[m.policy_head.conv0]
        rows_a, rows_ga = a.permute(0, 2, 3, 1).reshape(-1, 64), ga.permute(0, 2, 3, 1).reshape(-1, 16)
        kchunk = p.gemms(case.n, case.value_fc)["head_wgrad"][1]
        step = slice(kchunk - 32, kchunk)                    # the last K step of split 0
        out["last K step of a split missing from the head-conv weight gradient"] = TC.mutate(
            t32, "policy_head.conv0.weight", -(rows_ga[step].t() @ rows_a[step]).reshape(16, 64, 1, 1))
    return out


@pytest.mark.parametrize("tab,cid", LARGE)
def test_the_criterion_rejects_damaged_float32_results(tab, cid):
    """untouched torch float32 passes the criterion at K = 1; each mutant is rejected at K = 4 (the factor by which it misses is printed
    and recorded in EXPERIMENTS.md)"""
    case, t64, t32 = reference(tab, cid)
    floors, outputs = (TC.FLOORS_TOWER, ("out", "grad_x")) if tab == "tower" else (TC.FLOORS_NET, ("logp", "v"))
    assert not TC.judge(t32, t32, t64, floors, K=1.0, outputs=outputs)[1]
    muts = mutants(tab, case, t32)
    assert len(muts) >= (3 if tab == "tower" else 5) - (0 if "previous chunk's samples in place of the partial last chunk's zeros" in muts else 1)
    for name, mut in muts.items():
        rows, failures, _ = TC.judge(mut, t32, t64, floors, outputs=outputs)
        factor = max(r[3] for r in rows)
        print("MUTANT %-6s %-14s %-72s rejected by %.3gx" % (tab, cid, name, factor))
        assert failures and factor > 1.0, (name, factor)
