"""Exact training targets on the GPU (csrc/endgame.hip k_endgame_candidates / k_endgame_list / k_endgame_targets, dbaz_exact_targets,
dbaz_dataset_exact_targets): bit for bit against the numpy restatement (targets_ref.py), against the solved 3x3 table as an
independent yardstick, through the resident dataset and its batches, and through one generation of the coach."""
import numpy as np
import pytest

from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.endgame import Endgame, random_rows
import endgame_ref as ER
import targets_ref as TR

pytestmark = pytest.mark.gpu

MODES = [(p, z) for p in ("keep", "uniform", "restrict") for z in (False, True)]

# rows -> what the reference must find in them (conditions on the inputs, asserted before anything is compared): unfinished rows,
# rows whose O is a proper subset of the free edges, rows whose first free edge is outside O (a one-hot pi there has S == 0),
# rows whose z = (i % 3) - 1 differs from v, rows with n_free = 17
ROW_SETS = {
    "4x4": (4, 4, lambda: random_rows(4, 4, 40, np.arange(40) % 17, seed=3), dict(unfinished=37, proper=26, fallback=11, z_changed=25, deep=0)),
    "6x6": (6, 6, lambda: random_rows(6, 6, 54, np.arange(54) % 18, seed=5), dict(unfinished=48, proper=26, fallback=4, deep=3)),
    "2x7": (2, 7, lambda: random_rows(2, 7, 34, np.arange(34) % 17, seed=11), dict(unfinished=32, proper=23, fallback=14, deep=0)),
    "1x1": (1, 1, lambda: random_rows(1, 1, 8, np.arange(8) % 5, seed=2), dict(unfinished=6, proper=0, fallback=0, deep=0)),
    "4x4 play": (4, 4, lambda: TR.late_positions(4, 4, 99)[0], None),
    "6x6 play": (6, 6, lambda: TR.late_positions(6, 6, 264)[0], None),
}
_sets = {}


def first_free(R, C, x):
    acts = np.array(ER.board(R, C)[0])
    free = x[:, acts] == 0
    return np.where(free.any(axis=1), acts[free.argmax(axis=1)], -1)


def row_set(name):
    """(R, C, x, the two pi inputs, z, the reference's facts), built once and left unchanged"""
    if name not in _sets:
        R, C, make, want = ROW_SETS[name]
        x = make()
        n, A = len(x), 2 * (R + 1) * (C + 1)
        acts = ER.board(R, C)[0]
        legal = np.zeros((n, A), bool)
        legal[:, acts] = x[:, acts] == 0
        pi = np.random.RandomState(len(name)).rand(n, A).astype(np.float32) * legal
        pi = (pi / np.maximum(pi.sum(axis=1, keepdims=True), np.float32(1e-30))).astype(np.float32)
        hot = np.zeros((n, A), np.float32)
        ff = first_free(R, C, x)
        hot[np.nonzero(ff >= 0)[0], ff[ff >= 0]] = 1.0
        z = (np.arange(n) % 3 - 1).astype(np.float32)
        facts = TR.solve_rows(R, C, x)
        touched = [f for f in facts if f["touched"]]
        found = dict(unfinished=len(touched), proper=sum(len(f["O"]) < f["n_free"] for f in touched),
                     fallback=sum(f["touched"] and ff[i] not in f["O"] for i, f in enumerate(facts)),
                     z_changed=sum(f["touched"] and z[i] != f["v"] for i, f in enumerate(facts)), deep=sum(f["n_free"] == 17 for f in facts))
        if want is not None:
            assert {k: found[k] for k in want} == want, found
        else:
            assert {f["v"] for f in touched} == {-1, 0, 1} and len(touched) == n >= 60
        if name == "1x1":
            assert sorted(f["v"] for f in touched) == [-1, -1, -1, 1, 1, 1]
        _sets[name] = (R, C, x, pi, hot, z, facts)
    return _sets[name]


def check(got, want, x_pi_z, facts, what):
    """every output bit for bit; untouched rows against the inputs"""
    gpi, gz, info = got
    pi, z = x_pi_z
    assert gpi.dtype == np.float32 and gz.dtype == np.float32 and info["n_free"].dtype == np.int16 and info["mass"].dtype == np.float32
    for k, g, w in (("pi", gpi, want["pi"]), ("z", gz, want["z"]), ("mass", info["mass"], want["mass"])):
        bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, (what, k, bad[:8], [facts[i]["n_free"] for i in bad[:8]])
    assert np.array_equal(info["n_free"], want["n_free"]), what
    assert np.array_equal(info["relabelled"], want["relabelled"] != 0), what
    same = want["relabelled"] == 0
    assert np.array_equal(gpi[same].view(np.uint32), pi[same].view(np.uint32)) and np.array_equal(gz[same].view(np.uint32), z[same].view(np.uint32))
    assert (info["mass"][same] == 0).all()


# ---------------------------------------------------------------- 1. the stateless call against the reference
@pytest.mark.parametrize("name", list(ROW_SETS))
def test_stateless_call_equals_the_reference(name):
    R, C, x, pi, hot, z, facts = row_set(name)
    g = Endgame(R, C)
    for which, p in (("random", pi), ("one-hot", hot)):
        p0, z0 = p.copy(), z.copy()
        for pm, zm in MODES:
            got = g.targets(x, p, z, pm, zm)
            check(got, TR.apply_targets(facts, p, z, pm, zm), (p, z), facts, (name, which, pm, zm))
            assert np.array_equal(p, p0) and np.array_equal(z, z0)  # the caller's arrays stay
    if name != "1x1":
        fb = [i for i, f in enumerate(facts) if f["touched"] and hot[i][f["O"]].sum() == 0]
        got = g.targets(x, hot, z, "restrict", True)
        uni = g.targets(x, hot, z, "uniform", True)
        assert len(fb) >= 4 and (got[2]["mass"][fb] == 0).all() and np.array_equal(got[0][fb], uni[0][fb]) and (got[0][fb].sum(axis=1) > 0.999).all()
    g.close()


def test_many_rows_torch_tensors_and_a_side_stream():
    """more rows than one pass of any of the kernels' grids takes, as device tensors on another stream: the same bytes"""
    import torch
    R, C, x0, pi0, _, z0, facts0 = row_set("4x4")
    n = 70001
    src = (np.arange(n) * 7) % len(x0)
    x, pi, z = x0[src], pi0[src], z0[src]
    facts = [facts0[i] for i in src]
    base = TR.apply_targets(facts0, pi0, z0, "restrict", True)  # every row is relabelled on its own
    want = {k: base[k][src] for k in ("pi", "z", "n_free", "mass", "relabelled")}
    g = Endgame(R, C)
    xt, pt, zt = torch.as_tensor(x).cuda().reshape(n, 3, 5, 5), torch.as_tensor(pi).cuda(), torch.as_tensor(z).cuda().reshape(n, 1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gp, gz, info = g.targets(xt, pt, zt)
    side.synchronize()
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (gp, gz, *info.values())) and gz.shape == (n, 1)
    assert torch.equal(pt.cpu(), torch.as_tensor(pi)) and torch.equal(zt.cpu().ravel(), torch.as_tensor(z))
    check((gp.cpu().numpy(), gz.cpu().numpy().ravel(), {k: v.cpu().numpy() for k, v in info.items()}), want, (pi, z), facts, "many rows")
    # the scratch has grown for this call: a small call afterwards is served from the same handle
    check(g.targets(x0, pi0, z0, "uniform", True), TR.apply_targets(facts0, pi0, z0, "uniform", True), (pi0, z0), facts0, "after")
    g.close()


# ---------------------------------------------------------------- 2. max_free
def test_smaller_max_free_leaves_deeper_rows_alone():
    R, C, x, pi, _, z, _ = row_set("4x4")
    g = Endgame(4, 4, max_free=10)
    facts = TR.solve_rows(4, 4, x, max_free=10)
    deep = np.array([f["n_free"] > 10 for f in facts])
    assert set(np.array([f["n_free"] for f in facts])[deep]) == set(range(11, 17))
    for pm, zm in MODES:
        got = g.targets(x, pi, z, pm, zm)
        check(got, TR.apply_targets(facts, pi, z, pm, zm), (pi, z), facts, (pm, zm))
        assert not got[2]["relabelled"][deep].any()
    g.close()


# ---------------------------------------------------------------- 3. the solved 3x3 table as an independent yardstick
def test_uniform_targets_are_optimal_by_the_solved_3x3_table():
    from dotsboxesaz_amd.solver import ILLEGAL, Solver
    from test_hip_endgame import random_games
    x, left = random_games(3, 3, 8, seed=41)
    sv, g = Solver(3, 3).solve(), Endgame(3, 3)
    before = sv.score(x, np.zeros((len(x), 32), np.float32))
    rows = (left <= 16) & (before["q"] != ILLEGAL).any(axis=1)  # unfinished, within reach
    assert rows.sum() >= 60 and set(before["value"][rows]) == {-1, 1}  # nine boxes: no draw
    x = x[rows]
    pi, z, info = g.targets(x, np.full((len(x), 32), 1 / 32, np.float32), np.zeros(len(x), np.float32), "uniform", True)
    after = sv.score(x, pi)
    sv.close()
    g.close()
    assert info["relabelled"].all()
    assert np.array_equal(after["value"].astype(np.float32), z)
    assert np.abs(after["policy_mass"] - 1.0).max() <= 1e-6


# ---------------------------------------------------------------- 4. the resident dataset
_facts_by_row = {}


def dataset_reference(x, pi, z, pi_mode, z_mode):
    """the reference on fetched dataset rows; a position is solved once however often it comes"""
    facts = []
    for row in x:
        k = row.tobytes()
        if k not in _facts_by_row:
            _facts_by_row[k] = TR.solve_rows(3, 3, row[None])[0]
        facts.append(_facts_by_row[k])
    out = TR.apply_targets(facts, pi, z, pi_mode, z_mode)
    return out, TR.stats_ref(facts, out)


def played_rows():
    """(engine, every second replay row of 64 self-play games on 3x3, on the device)"""
    import torch
    from dotsboxesaz_amd.engine import Engine
    from dotsboxesaz_amd.self_play import _DevBuf
    e = Engine(3, 3, 32, mcts_num_read=16, noise=(0.8, 0.25), evaluator="formula", seed=5)
    e.selfplay_start(64, 0)
    e.run()
    ptr, n, rb = e.replay_rows_dev()
    rows = torch.as_tensor(_DevBuf(ptr, n * rb), device=torch.device("cuda", 0)).view(n, rb)[::2].clone()
    e.fetch_samples()
    return e, rows


def same_stats(got, want):
    return all(got[k] == want[k] for k in ("rows", "relabelled", "finished", "z_changed")) and np.array_equal(got["by_free"], want["by_free"])


def test_dataset_is_relabelled_in_place():
    from oracle import train_ref
    from dotsboxesaz_amd.train_data import ReplayDataset, ReplayStore
    e, rows = played_rows()
    g = Endgame(3, 3)
    for avg in (False, True):
        e.dataset_select(2)
        e.dataset_begin()
        e.dataset_add_rows(rows)
        m = e.dataset_finish(avg)
        x, pi, z = e.dataset_fetch()
        assert m == len(x) and (m < rows.shape[0] if avg else m == rows.shape[0])
        want, want_stats = dataset_reference(x, pi, z, "restrict", True)
        stats = e.dataset_exact_targets(g, "restrict", True)
        assert same_stats(stats, want_stats), (stats, want_stats)
        # every class of n_free the kernel is launched for is there (a 3x3 game cannot end early before 15 edges are drawn)
        assert 0 < stats["relabelled"] < m and stats["z_changed"] > 0 and (stats["by_free"][10:17] > 0).all() and stats["by_free"][:10].sum() > 0
        x2, pi2, z2 = e.dataset_fetch()
        assert np.array_equal(x2, x)
        assert np.array_equal(pi2.view(np.uint32), want["pi"].view(np.uint32)) and np.array_equal(z2.view(np.uint32), want["z"].view(np.uint32))
        assert not np.array_equal(pi2, pi)
        idx = np.concatenate([np.nonzero(want["relabelled"])[0][:24], np.arange(8), [m - 1]]).astype(np.int32)
        for sym in (0, 3, 5):
            b, p, zz = e.dataset_batch(idx, sym)
            rb_, rp_ = train_ref.apply_symmetry(x2[idx].astype(np.float32).reshape(-1, 3, 4, 4), pi2[idx], sym)
            assert np.array_equal(b.cpu().numpy(), rb_) and np.array_equal(p.cpu().numpy(), rp_) and np.array_equal(zz.cpu().numpy().ravel(), z2[idx])
        # a second "uniform" pass over rows that a first one has relabelled changes nothing
        first = e.dataset_exact_targets(g, "uniform", True)
        _, pi3, z3 = e.dataset_fetch()
        again = e.dataset_exact_targets(g, "uniform", True)
        _, pi4, z4 = e.dataset_fetch()
        assert np.array_equal(pi4.view(np.uint32), pi3.view(np.uint32)) and np.array_equal(z4.view(np.uint32), z3.view(np.uint32))
        assert first["z_changed"] == 0 and again["z_changed"] == 0 and np.array_equal(again["by_free"], stats["by_free"])
    # ReplayDataset(exact=g): the host copy behind ds[i] holds the relabelled values, also after a relabel of a dataset that was read
    store = ReplayStore(e)
    np.random.seed(3)
    store.add_generation(0, rows, train_split=0.5)
    np.random.seed(4)
    plain = ReplayDataset(store, train=True, slot=3)
    x, pi, z = (a.copy() for a in plain._arrays())
    assert plain.exact_stats is None
    want, want_stats = dataset_reference(x.reshape(len(x), -1).astype(np.int16), pi, z, "restrict", True)
    np.random.seed(4)
    ds = ReplayDataset(store, train=True, slot=3, exact=g)
    assert len(ds) == len(plain) and same_stats(ds.exact_stats, want_stats) and ds.exact_stats["relabelled"] > 0
    i = int(np.nonzero((want["pi"] != pi).any(axis=1) & (want["z"] != z))[0][-1])  # a row whose pi and z both change
    f_i, p_i, v_i = ds[i]
    assert np.array_equal(f_i, x[i]) and np.array_equal(p_i, want["pi"][i]) and v_i[0] == want["z"][i] != z[i] and not np.array_equal(p_i, pi[i])
    ds.relabel(g, "uniform", True)  # after ds[i] has filled the host copy
    want_u, _ = dataset_reference(x.reshape(len(x), -1).astype(np.int16), want["pi"], want["z"], "uniform", True)
    assert np.array_equal(ds[i][1], want_u["pi"][i])
    store2 = store.dataset(train=False, slot=3, exact=g, exact_pi="uniform", exact_z=False)
    assert store2.exact_stats["rows"] == len(store2) > 0
    g.close()
    e.close()


# ---------------------------------------------------------------- 5. errors
def test_errors_and_the_empty_call():
    from dotsboxesaz_amd.engine import Engine
    R, C, x, pi, _, z, _ = row_set("4x4")
    g = Endgame(4, 4)
    for bad in ((3, 1), (-1, 0), (2, 2)):
        with pytest.raises(_lib.DbazError) as ei:
            g.targets(x, pi, z, *bad)
        assert ei.value.code == _lib.EINVAL
    L = _lib.load()
    assert L.dbaz_exact_targets(g.h, 4, None, 0, 0, None, None, None, None, None, None) == _lib.EINVAL        # rows without x
    import torch
    xt = torch.as_tensor(x).cuda()
    assert L.dbaz_exact_targets(g.h, 4, xt.data_ptr(), 1, 0, None, None, None, None, None, None) == _lib.EINVAL  # uniform without pi
    assert L.dbaz_exact_targets(g.h, 4, xt.data_ptr(), 0, 1, None, None, None, None, None, None) == _lib.EINVAL  # solved z without z
    assert L.dbaz_exact_targets(g.h, 0, None, 2, 1, None, None, None, None, None, None) == _lib.OK               # n == 0: nothing is read
    assert L.dbaz_exact_targets(g.h, 0, None, 3, 0, None, None, None, None, None, None) == _lib.EINVAL           # ... but the modes are checked
    p0, z0, info = g.targets(np.zeros((0, 75), np.int16), np.zeros((0, 50), np.float32), np.zeros(0, np.float32))
    assert p0.shape == (0, 50) and z0.shape == (0,) and info["n_free"].shape == (0,)
    e = Engine(3, 3, 4, mcts_num_read=10, evaluator="formula", nodes_per_slot=64)
    g3 = Endgame(3, 3)
    for args, code in (((g3, "restrict", True), _lib.ESTATE),   # no finished dataset in the slot
                       ((g, "restrict", True), _lib.EINVAL),    # another board size
                       ((g3, 3, True), _lib.EINVAL)):
        with pytest.raises(_lib.DbazError) as ei:
            e.dataset_exact_targets(*args)
        assert ei.value.code == code, args
    e.dataset_begin()
    assert e.dataset_finish(False) == 0
    empty = e.dataset_exact_targets(g3, "uniform", True)          # an empty dataset: nothing to do
    assert empty["rows"] == 0 and empty["relabelled"] == 0 and not empty["by_free"].any()
    e.close()
    g3.close()
    g.close()


# ---------------------------------------------------------------- 6. the coach
def test_one_generation_with_exact_targets(tmp_path):
    import torch
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd import train as T
    from dotsboxesaz_amd.coach import Coach
    params = dnn.resnet_params(3, 3, 32, 2, 4, 8)
    params["nn"]["model_class"] = dnn.ResNetZero
    params["nn"]["chkpts_filename"] = str(tmp_path / "model_gen{}.pt")
    params["nn"]["train_params"] = {"nb_epochs": 1, "train_batch_size": 64, "val_batch_size": 32, "lr": 1e-2,
                                    "lr_scheduler": T.GenerationLrScheduler({0: 1e-2}),
                                    "optimizer_params": {"momentum": 0.9, "weight_decay": 1e-4},
                                    "pos_average": True, "train_split": 0.9, "max_samples_per_gen": 100000, "symmetries": None}
    params["self_play"] = {"num_games": 16, "reuse_mcts_tree": True, "noise": (0.8, 0.25),
                           "mcts": {"mcts_num_read": 16, "mcts_cpuct": (1.25, 19652), "temperature": {0: 1.0, 6: 0.02}}}
    params["elo"] = None
    torch.manual_seed(0)
    np.random.seed(0)
    coach = Coach(params, 3, 3, n_slots=16, exact_targets=True)
    log = coach.learn_to_play(0, 0)
    st = log[0]["exact_targets"]
    assert [r["generation"] for r in log] == [0] and log[0]["selfplay"]["rows"] > 16 * 8
    assert st["relabelled"] > 0 and st["relabelled"] == int(st["by_free"].sum()) and st["rows"] >= st["relabelled"]
    assert isinstance(coach.exact_targets, Endgame) and coach.exact_targets.max_free == 16
    coach.close()
    plain = Coach(params, 3, 3, n_slots=16)
    assert "exact_targets" not in plain.learn_to_play(0, 0)[0]
    plain.close()
