"""Deep exact targets on packed replay rows on the GPU (dbaz_replay_exact_targets in csrc/solver.hip, DeepTables.replay_targets,
Coach(exact_targets=DeepTables(...))): the relabelled rows byte for byte against the numpy restatement (replay_targets_ref.py) in
every mode, in any row order, the roots against endgame._game_roots, the device-built geometries through the tables they solve,
the merged host route game_tail_targets, the rows through the dataset kernels, the refusals, and the generation loop.
The 4x4 formula fixture of the deep tests, pools of 1 MiB tables.  Boards with other row layouts (more ballot words, 2-byte aligned
visits, A = 256, 1x1) are in test_hip_replay_targets_boards.py, against a numpy-only reference."""
import numpy as np
import pytest

from dotsboxesaz_amd import _lib
from dotsboxesaz_amd import self_play as sp
from dotsboxesaz_amd.endgame import DeepEndgame, DeepTables, _game_roots, game_tail_targets
from dotsboxesaz_amd.solver import ILLEGAL
import endgame_ref as ER
import replay_targets_ref as RR
import targets_ref as TR
from test_hip_deep_tables import MODES

pytestmark = pytest.mark.gpu

R, C = 4, 4
F, A = 75, 50
_fixture, _plans = {}, {}


def played():
    """8 formula-evaluator 4x4 self-play games, played once and left unchanged: (packed rows uint8 [n, row_bytes] on the host,
    the same rows through unpack_rows, order: unpacked row k is packed row order[k])"""
    if not _fixture:
        from dotsboxesaz_amd.engine import Engine
        e = Engine(R, C, 8, mcts_num_read=40, evaluator="formula")
        packed = sp.collect_rows_device(e, 8, 0).cpu().numpy()  # replay_rows_dev, cloned on the device
        e.close()
        meta = RR.fields(R, C, packed)[0]
        _fixture.update(packed=packed, rows=sp.unpack_rows(packed, F, A), order=np.lexsort((meta["move_idx"], meta["game_idx"])))
    return _fixture["packed"], _fixture["rows"], _fixture["order"]


def facts_from_table(rows, cols, max_free):
    """facts_for of replay_targets_ref.plan from the single-table scorer, which the existing tests pin against endgame_ref.py:
    v = value, O = the free a with sign(margin + q[a]) == v, finished = no move has a q"""
    acts, _ = ER.board(rows, cols)
    d = DeepEndgame(rows, cols, max_free=max_free)

    def facts_for(root, xs):
        sc = d.solve(root).score(xs)
        assert sc["solved"].all()
        out = []
        for i, x in enumerate(xs):
            free = [a for a in acts if x[a] == 0]
            fin = not (sc["q"][i] != ILLEGAL).any()
            m, v = TR.margin_of(rows, cols, x), int(sc["value"][i])
            out.append(dict(finished=fin, v=v, O=[] if fin else [a for a in free if int(np.sign(m + int(sc["q"][i][a]))) == v]))
        return out
    return facts_for, d


def plan_of(max_free, packed=None, key=None):
    key = key or max_free
    if key not in _plans:
        facts_for, d = facts_from_table(R, C, max_free)
        _plans[key] = RR.plan(R, C, played()[0] if packed is None else packed, max_free, facts_for)
        d.close()
    return _plans[key]


def dev(packed):
    import torch
    return torch.as_tensor(np.ascontiguousarray(packed)).cuda()


def check_stats(got, want, max_free):
    for k in RR.STATS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert len(got["by_free"]) == max_free + 1 and np.array_equal(got["by_free"], want["by_free"])


# ---------------------------------------------------------------- 1. against the restatement, byte for byte
@pytest.mark.parametrize("max_free", [16, 20])
def test_relabelled_rows_equal_the_restatement_byte_for_byte(max_free):
    packed, rows, _ = played()
    p = plan_of(max_free)
    left = p["n_free"]
    assert len(set(rows["game_idx"].tolist())) == 8 and len(p["roots"]) == 8 and (left > max_free).any()
    t = DeepTables(R, C, max_free=max_free, n_tables=3)  # chunks of 3, 3 and 2
    for pi_mode, z_mode in MODES:
        want, st = RR.apply(R, C, packed, p, pi_mode, z_mode, n_tables=3, max_free=max_free)
        rows_dev = dev(packed)
        got = t.replay_targets(rows_dev, pi_mode, z_mode)
        out = rows_dev.cpu().numpy()
        assert np.array_equal(out, want), (pi_mode, z_mode, np.nonzero((out != want).any(axis=1))[0][:8])
        check_stats(got, st, max_free)
        assert got["chunks"] == 3 and got["relabelled"] >= 8 * 10 and got["unserved"] == 0
        assert np.array_equal(out[left > max_free], packed[left > max_free])  # the rows before a game's root
        assert t.n_solved == 2 and all(v >= 0 for v in got["kernel_ms"].values())  # the last chunk's tables stay
        assert (want != packed).any() == (pi_mode != "keep" or z_mode)
    t.close()


# ---------------------------------------------------------------- 2. any order
@pytest.mark.parametrize("max_free", [16, 20])
def test_rows_in_any_order(max_free):
    packed, _, _ = played()
    p = plan_of(max_free)
    want, st = RR.apply(R, C, packed, p, "restrict", True, n_tables=3, max_free=max_free)
    perm = np.random.RandomState(max_free).permutation(len(packed))
    t = DeepTables(R, C, max_free=max_free, n_tables=3)
    rows_dev = dev(packed[perm])
    got = t.replay_targets(rows_dev)
    assert np.array_equal(rows_dev.cpu().numpy(), want[perm])
    check_stats(got, st, max_free)
    t.close()


# ---------------------------------------------------------------- 3. the roots
@pytest.mark.parametrize("max_free", [16, 20])
def test_roots_equal_game_roots(max_free):
    packed, rows, order = played()
    left = (rows["x"][:, ER.board(R, C)[0]] == 0).sum(axis=1)
    root, table_of, _ = _game_roots(rows["game_idx"].astype(np.int64), rows["move_idx"].astype(np.int64), left, max_free)
    want = np.full(len(packed), -1, np.int32)
    want[order] = np.where(table_of >= 0, order[root[np.maximum(table_of, 0)]], -1)  # unpacked row k is packed row order[k]
    t = DeepTables(R, C, max_free=max_free, n_tables=3)
    got = t.replay_targets(dev(packed), "keep", False, return_roots=True)
    assert got["root_of"].is_cuda and str(got["root_of"].dtype) == "torch.int32"
    assert np.array_equal(got["root_of"].cpu().numpy(), want) and np.array_equal(want, plan_of(max_free)["root_of"])
    assert (want >= 0).sum() > 8 * max_free * 0.5 and (want < 0).any()
    t.close()


# ---------------------------------------------------------------- 4. the geometries built on the device
@pytest.mark.parametrize("max_free", [16, 20])
def test_device_geometry_solves_the_host_paths_tables(max_free):
    packed, _, _ = played()
    p = plan_of(max_free)
    x = RR.fields(R, C, packed)[1]
    t = DeepTables(R, C, max_free=max_free, n_tables=8)  # one chunk
    got = t.replay_targets(dev(packed), "keep", False)
    assert got["chunks"] == 1 and t.n_solved == 8
    host = DeepTables(R, C, max_free=max_free, n_tables=8).solve(x[p["roots"]])  # F descending, game_idx ascending
    assert np.array_equal(t.n_free, host.n_free) and np.array_equal(t.d0, host.d0) and (np.diff(t.n_free) <= 0).all()
    for i in range(8):
        assert np.array_equal(t.table(i), host.table(i)), i
    sc, want = t.score(x[p["roots"]], np.arange(8, dtype=np.int32)), host.score(x[p["roots"]], np.arange(8, dtype=np.int32))
    for k in ("value", "diff", "q", "n_free", "solved"):  # the root headers serve rows as the host-built ones do
        assert np.array_equal(sc[k], want[k]), k
    assert sc["solved"].all()
    t.close()
    host.close()


# ---------------------------------------------------------------- 5. against the merged host route
@pytest.mark.parametrize("max_free", [16, 20])
def test_agrees_with_game_tail_targets(max_free):
    packed, rows, order = played()
    p = plan_of(max_free)
    relabel = np.array([s == "relabel" for s in p["status"]])[order]
    t = DeepTables(R, C, max_free=max_free, n_tables=3)
    for pi_mode in ("uniform", "restrict"):
        want_pi, want_z, info = game_tail_targets(rows, rows=R, cols=C, max_free=max_free, tables=3, pi_mode=pi_mode, z_mode=True)
        assert np.array_equal(info["relabelled"], relabel)
        rows_dev = dev(packed)
        t.replay_targets(rows_dev, pi_mode, True)
        after = sp.unpack_rows(rows_dev.cpu().numpy(), F, A)
        assert np.array_equal(after["z"].astype(np.float32), want_z)
        pi = after["pi"].astype(np.float32)
        assert np.array_equal(pi != 0, want_pi != 0)
        if pi_mode == "uniform":
            assert np.array_equal(pi.view(np.uint32), want_pi.view(np.uint32))
        else:
            # one side: one correctly rounded quotient; the other: a rounded quotient divided by a float32 sum of at most max_free
            # rounded terms
            on = want_pi != 0
            rel = np.abs(pi[on].astype(np.float64) - want_pi[on]) / want_pi[on]
            print("restrict, max_free %d: largest relative difference %.3g (bound %.3g)" % (max_free, rel.max(), (max_free + 3) * 2.0 ** -24))
            assert rel.max() <= (max_free + 3) * 2.0 ** -24
    t.close()


# ---------------------------------------------------------------- 6. through the dataset kernels
@pytest.mark.parametrize("max_free", [16, 20])
def test_relabelled_rows_through_the_dataset(max_free):
    from dotsboxesaz_amd import train_data as TD
    from dotsboxesaz_amd.engine import Engine
    packed, _, _ = played()
    p = plan_of(max_free)
    rows_dev = dev(packed)
    t = DeepTables(R, C, max_free=max_free, n_tables=3)
    t.replay_targets(rows_dev)
    t.close()
    out = rows_dev.cpu().numpy()
    meta, x, vis = RR.fields(R, C, out)
    pi = (vis.astype(np.float64) / np.maximum(vis.sum(axis=1, dtype=np.int64), 1)[:, None]).astype(np.float32)
    e = Engine(R, C, 8, mcts_num_read=40, evaluator="formula")
    for avg in (False, True):
        np.random.seed(11)
        store = TD.ReplayStore(e)
        store.add_generation(0, rows_dev, train_split=0.9)
        locs = store.chunks[0]["train_locs"]
        state = np.random.get_state()
        ds = store.dataset(train=True, pos_average=avg)
        np.random.set_state(state)
        sel = locs[TD._sample_locs(len(locs), len(locs))]  # the draw ReplayDataset made: dataset row k is packed row sel[k]
        assert ds.exact_stats is None
        e.dataset_select(ds.slot)
        dx, dpi, dz = e.dataset_fetch()
        if not avg:
            assert len(ds) == len(sel) and np.array_equal(dx, x[sel])
            assert np.array_equal(dpi.view(np.uint32), pi[sel].view(np.uint32)) and np.array_equal(dz, meta["z"][sel].astype(np.float32))
            continue
        assert 0 < len(ds) <= len(sel)
        O_of = {x[r].tobytes(): p["O"][r] for r in range(len(x)) if p["status"][r] == "relabel"}  # O is a function of the position
        seen = 0
        for k in range(len(ds)):
            O = O_of.get(dx[k].tobytes())
            if O is not None:
                seen += 1
                assert not np.delete(dpi[k], O).any() and dpi[k][O].sum() > 0.999, k
        assert seen >= 8 * 5
    e.close()


# ---------------------------------------------------------------- 7. errors and edges
def test_errors_and_edges():
    import torch
    packed, _, _ = played()
    t = DeepTables(R, C, max_free=16, n_tables=3)
    twice = np.concatenate([packed, packed[17:18]])
    rows_dev = dev(twice)
    with pytest.raises(_lib.DbazError) as ei:
        t.replay_targets(rows_dev)
    assert ei.value.code == _lib.EINVAL and "game_idx" in str(ei.value) and np.array_equal(rows_dev.cpu().numpy(), twice) and t.n_solved == 0
    good = dev(packed)
    for bad in (good[:, :-8].contiguous(), good.cpu(), good[::2], good.to(torch.int16), good.reshape(-1)):
        with pytest.raises(ValueError):
            t.replay_targets(bad)
    with pytest.raises(ValueError):
        t.replay_targets(good, "sharpen")
    assert np.array_equal(good.cpu().numpy(), packed)
    none = t.replay_targets(good[:0])
    assert all(none[k] == 0 for k in RR.STATS) and not none["by_free"].any() and len(none["by_free"]) == 17
    L = _lib.load()
    ptr = lambda v: _lib.C.c_void_p(v)  # noqa: E731
    for args in ((None, 5, packed.shape[1], 2, 1), (good.data_ptr(), 5, packed.shape[1] + 8, 2, 1), (good.data_ptr(), 5, packed.shape[1], 3, 1),
                 (good.data_ptr(), 5, packed.shape[1], 2, 2), (good.data_ptr(), -1, packed.shape[1], 2, 1)):
        assert L.dbaz_replay_exact_targets(t.h, ptr(args[0]), args[1], args[2], args[3], args[4], None, None, None) == _lib.EINVAL, args
    assert np.array_equal(good.cpu().numpy(), packed)
    # a row whose x is another game's: no subset of its root's free edges
    p = plan_of(16)
    victim = next(r for r in range(len(packed)) if p["status"][r] == "relabel" and p["root_of"][r] != r)  # a row after its game's root
    donor = int(np.nonzero(p["n_free"] > 16)[0][0])  # more free edges than any root has
    foreign = packed.copy()
    foreign[victim, 28:28 + 2 * F] = packed[donor, 28:28 + 2 * F]
    q = plan_of(16, foreign, key="foreign")
    assert q["status"][victim] == "unserved"
    want, st = RR.apply(R, C, foreign, q, "restrict", True, n_tables=3, max_free=16)
    rows_dev = dev(foreign)
    got = t.replay_targets(rows_dev)
    out = rows_dev.cpu().numpy()
    assert got["unserved"] == 1 == st["unserved"] and np.array_equal(out[victim], foreign[victim]) and np.array_equal(out, want)
    t.close()
    # max_free below every row's F: nothing to do
    low = DeepTables(R, C, max_free=1, n_tables=3)
    cut = packed[plan_of(16)["n_free"] >= 2]
    rows_dev = dev(cut)
    got = low.replay_targets(rows_dev)
    assert (got["rows"], got["games"], got["roots"], got["chunks"], got["relabelled"]) == (len(cut), 8, 0, 0, 0) and low.n_solved == 0
    assert np.array_equal(rows_dev.cpu().numpy(), cut)
    low.close()


# ---------------------------------------------------------------- 8. the generation loop
def test_coach_relabels_the_packed_rows_before_the_dataset_build(tmp_path, monkeypatch):
    import torch
    from dotsboxesaz_amd import nn as dnn
    from dotsboxesaz_amd import train as T
    from dotsboxesaz_amd import train_data as TD
    from dotsboxesaz_amd.coach import Coach

    def params():
        q = dnn.resnet_params(3, 3, 32, 2, 4, 8)
        q["nn"]["model_class"] = dnn.ResNetZero
        q["nn"]["chkpts_filename"] = str(tmp_path / "model_gen{}.pt")
        q["nn"]["train_params"] = {"nb_epochs": 2, "train_batch_size": 128, "val_batch_size": 32, "lr": 1e-2,
                                   "lr_scheduler": T.GenerationLrScheduler({0: 1e-2}), "optimizer_params": {"momentum": 0.9, "weight_decay": 1e-4},
                                   "pos_average": False, "train_split": 0.8, "max_samples_per_gen": 100000, "symmetries": None}
        q["self_play"] = {"num_games": 64, "reuse_mcts_tree": True, "noise": (0.8, 0.25),
                          "mcts": {"mcts_num_read": 16, "mcts_cpuct": (1.25, 19652), "temperature": {0: 1.0, 6: 0.02}}}
        q["elo"] = None
        return q

    taken, built = [], []
    collect, dataset = sp.collect_rows_device, TD.ReplayStore.dataset

    def collecting(*a, **k):
        rows = collect(*a, **k)
        taken.append(rows.clone())
        return rows

    def building(self, *a, **k):
        built.append((k, dataset(self, *a, **k)))
        return built[-1][1]
    monkeypatch.setattr(sp, "collect_rows_device", collecting)
    monkeypatch.setattr(TD.ReplayStore, "dataset", building)

    def run(exact):
        torch.manual_seed(0)
        np.random.seed(0)
        coach = Coach(params(), 3, 3, n_slots=32, exact_targets=exact)
        log = coach.learn_to_play(0, 0)
        rows = coach.store.chunks[0]["rows"].cpu().numpy()
        coach.close()
        return log[0], rows

    pool = DeepTables(3, 3, max_free=20)
    rec, rows = run(pool)
    before = taken[0].cpu().numpy()
    assert rec["exact_targets"]["relabelled"] > 0 and rec["exact_targets"] == rec["selfplay"]["exact_targets"]
    assert rec["exact_targets"]["games"] == 64 and rec["exact_targets"]["roots"] == 64 and len(rec["exact_targets"]["by_free"]) == 21
    facts_for, d = facts_from_table(3, 3, 20)
    want, st = RR.apply(3, 3, before, RR.plan(3, 3, before, 20, facts_for), "restrict", True, n_tables=64, max_free=20)
    d.close()
    assert np.array_equal(rows, want) and (rows != before).any() and st["relabelled"] == rec["exact_targets"]["relabelled"]
    assert len(built) == 2 and all("exact" not in k and ds.exact_stats is None for k, ds in built)  # train and validation: no relabel of their own
    pool.close()
    rec2, rows2 = run(None)
    assert "exact_targets" not in rec2 and "exact_targets" not in rec2["selfplay"]
    # with the option off the stored rows are byte for byte what self-play wrote, and the games are the ones the first coach played.
    # The engine emits the rows of finished games in the order its slots happen to finish, and it leaves RowMeta.pad and the
    # bytes that pad a row to 8 as it found them in its buffer: the two runs are compared game by game and field by field
    def by_game(rows):
        meta, x, vis = RR.fields(3, 3, rows)
        order = np.lexsort((meta["move_idx"], meta["game_idx"]))
        return [meta[k][order] for k in meta.dtype.names if k != "pad"] + [x[order], vis[order]]
    assert np.array_equal(rows2, taken[1].cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(by_game(rows2), by_game(before)))
