"""What becomes of the fast rows of playout cap randomization behind self-play: ReplayStore splits only the rows that train,
generate_games writes only those, a Coach generation reports both kinds.  The fast rows are told by bit 0 of "pad" alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIMS, FAST, P, SEED = 40, 6, 0.25, 77
_rows = {}


def rows_with_a_cap():
    """(engine, packed rows on the device, the same on the host) of 32 3x3 games under the cap, played once"""
    if not _rows:
        import torch
        from dotsboxesaz_amd.engine import Engine
        from dotsboxesaz_amd.self_play import collect_rows_device
        e = Engine(3, 3, 16, mcts_num_read=SIMS, evaluator="formula", seed=SEED, playout_cap=(P, FAST))
        dev = collect_rows_device(e, 32, 0)
        _rows.update(e=e, dev=dev, host=dev.cpu().numpy().copy(), torch=torch)
    return _rows["e"], _rows["dev"], _rows["host"]


def old_split(n, train_split):
    """add_generation before there was a cap: the draws and the two lists"""
    locs = np.random.choice(n, size=int(round(train_split * n)), replace=False)
    mask = np.ones(n, dtype=bool)
    mask[locs] = False
    return locs.astype(np.int32), np.nonzero(mask)[0].astype(np.int32)


@pytest.mark.parametrize("avg", [False, True])
def test_store_drops_the_fast_rows(avg):
    import torch
    from dotsboxesaz_amd import train_data as TD
    e, dev, host = rows_with_a_cap()
    fast = (np.ascontiguousarray(host[:, 26:28]).view("<i2").ravel() & 1) != 0
    full_idx = np.nonzero(~fast)[0]
    assert 0 < len(full_idx) < len(host) / 2
    np.random.seed(5)
    store = TD.ReplayStore(e)
    store.add_generation(0, dev, train_split=0.8, fast_rows="drop")
    ch = store.chunks[0]
    ds = store.dataset(train=True, pos_average=avg, slot=2)
    got = e.dataset_fetch()
    # the same draws over the full rows alone, then the dataset that dataset_add_rows builds from the numpy-filtered rows
    np.random.seed(5)
    tr, va = old_split(len(full_idx), 0.8)
    assert np.array_equal(ch["train_locs"], full_idx[tr]) and np.array_equal(ch["val_locs"], full_idx[va]) and ch["n_fast"] == int(fast.sum())
    assert not fast[ch["train_locs"]].any() and not fast[ch["val_locs"]].any()
    take = np.random.choice(len(tr), size=len(tr), replace=False)
    filtered = torch.from_numpy(host[full_idx]).cuda()
    e.dataset_select(3)
    e.dataset_begin()
    e.dataset_add_rows(filtered, tr[take])
    n = e.dataset_finish(avg)
    want = e.dataset_fetch()
    assert n == len(ds) and (avg or n == len(tr))
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_store_keep_and_unmarked_rows_are_todays_split():
    from dotsboxesaz_amd import train_data as TD
    e, dev, host = rows_with_a_cap()
    np.random.seed(9)
    want = old_split(len(host), 0.9)
    for kw in (dict(fast_rows="keep"),):
        np.random.seed(9)
        store = TD.ReplayStore(e)
        store.add_generation(0, dev, **kw)
        assert np.array_equal(store.chunks[0]["train_locs"], want[0]) and np.array_equal(store.chunks[0]["val_locs"], want[1])
        assert store.chunks[0]["n_fast"] == 0
    # rows without a marked one (pad = 0: every row made without a cap) take the old path under the default, with the old draws
    clean = dev.clone()
    clean[:, 26:28] = 0
    np.random.seed(9)
    store = TD.ReplayStore(e)
    store.add_generation(0, clean)
    assert np.array_equal(store.chunks[0]["train_locs"], want[0]) and np.array_equal(store.chunks[0]["val_locs"], want[1])
    with pytest.raises(ValueError):
        store.add_generation(1, clean, fast_rows="value_only")


def params_3x3(tmp_path, cap):
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd import train as T
    params = dnn.resnet_params(3, 3, 32, 2, 4, 8)
    params["nn"]["model_class"] = dnn.ResNetZero
    params["nn"]["chkpts_filename"] = str(tmp_path / "model_gen{}.pt")
    params["nn"]["train_params"] = {"nb_epochs": 1, "train_batch_size": 64, "val_batch_size": 32, "lr": 1e-2,
                                    "lr_scheduler": T.GenerationLrScheduler({0: 1e-2}), "optimizer_params": {"momentum": 0.9, "weight_decay": 1e-4},
                                    "pos_average": True, "train_split": 0.9, "max_samples_per_gen": 100000, "symmetries": None}
    params["self_play"] = {"num_games": 32, "reuse_mcts_tree": True, "noise": (0.8, 0.25),
                           "mcts": {"mcts_num_read": 24, "mcts_cpuct": (1.25, 19652), "temperature": {0: 1.0, 6: 0.02}}}
    if cap:
        params["self_play"]["playout_cap"] = {"full_prob": P, "fast_reads": FAST}
    params["elo"] = None
    return params


def test_generate_games_writes_the_full_rows_only(tmp_path):
    import torch
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd import playout_cap as PC
    from dotsboxesaz_amd import self_play as sp
    params = params_3x3(tmp_path, True)
    assert sp.engine_kwargs_from_params(params)["playout_cap"] == (P, FAST)
    assert "playout_cap" not in sp.engine_kwargs_from_params(params_3x3(tmp_path, False))
    gen = 0
    torch.manual_seed(0)
    drop = sp.generate_games(None, gen, dnn.ResNetZero, 32, params, rows=3, cols=3, n_slots=16)
    torch.manual_seed(0)
    keep = sp.generate_games(None, gen, dnn.ResNetZero, 32, params, rows=3, cols=3, n_slots=16, fast_rows="keep")
    torch.manual_seed(0)
    plain = sp.generate_games(None, gen, dnn.ResNetZero, 32, params_3x3(tmp_path, False), rows=3, cols=3, n_slots=16)
    assert list(drop.columns) == list(keep.columns) == list(plain.columns) and drop.index.names == plain.index.names  # the reference's schema
    assert list(drop.dtypes) == list(plain.dtypes)
    g, i = keep.index.get_level_values("game_idx").to_numpy(), keep.index.get_level_values("move_idx").to_numpy()
    full = PC.is_full(gen * 1000003, g, i, P)
    assert 0 < full.sum() < len(keep) and len(drop) == int(full.sum())
    assert drop.equals(keep[full])
    assert sorted(set(g)) == list(range(32))


def test_one_coach_generation_with_a_cap_in_params(tmp_path):
    import torch
    from dotsboxesaz_amd.coach import Coach
    params = params_3x3(tmp_path, True)
    torch.manual_seed(0)
    np.random.seed(0)
    coach = Coach(params, 3, 3, n_slots=16)
    log = coach.learn_to_play(0, 0)
    s = log[0]["selfplay"]
    pc = coach.engine.playout_cap()
    assert pc["full_prob"] == P and pc["fast_reads"] == FAST
    assert s["full_rows"] + s["fast_rows"] == s["rows"] == s["moves_played"] and 0 < s["full_rows"] < s["fast_rows"]
    assert (s["full_rows"], s["fast_rows"]) == (pc["full_searches"], pc["fast_searches"])
    ch = coach.store.chunks[0]
    assert len(ch["train_locs"]) + len(ch["val_locs"]) == s["full_rows"] and ch["n_fast"] == s["fast_rows"]
    assert len(ch["train_locs"]) == int(round(0.9 * s["full_rows"]))
    coach.close()
