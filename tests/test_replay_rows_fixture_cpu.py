"""What the references alone say about the rows of replay_rows_fixture.py, before any kernel sees them: the inputs of
test_hip_replay_targets_boards.py and test_hip_train_data_boards.py reach every word, half-word, sign and fallback they are meant
to reach, and a restatement with one of those mistakes built in gives another answer on them.  The host-side symmetry table
against oracle/train_ref.py on the same boards.  Runs without a GPU.

Two conditions cannot hold on the 1x1 board with max_free = 4 and are stated for the other cases only: its four edges are all
within max_free, so no row lies above it, and its roots have every edge free, so every position is a subset of them and no row is
unserved."""
import numpy as np
import pytest

from dotsboxesaz_amd import _lib
from dotsboxesaz_amd.engine import symmetry_table
from dotsboxesaz_amd.self_play import ROW_META
from oracle import train_ref as T
import endgame_ref as ER
import replay_rows_fixture as FX
import replay_targets_ref as RR

M0 = ROW_META.itemsize


# ---------------------------------------------------------------- the restatement once more, with room for one mistake
def plan_with(R, C, packed, max_free, facts_for, unsigned_game=False, unsigned_move=False, subset_test=True):
    """replay_targets_ref.plan, line for line, except where a switch says otherwise"""
    acts, _ = ER.board(R, C)
    meta, x, _ = RR.fields(R, C, packed)
    n = len(x)
    game, move = meta["game_idx"].astype(np.int64), meta["move_idx"].astype(np.int64)
    if unsigned_game:
        game = game & 0xFFFFFFFF
    if unsigned_move:
        move = move & 0xFFFF
    free = x[:, acts] == 0
    n_free = free.sum(axis=1)
    root_of = np.full(n, -1, np.int32)
    status, v, O = [None] * n, [None] * n, [None] * n
    roots = []
    for g in sorted(set(game.tolist())):
        rows = np.nonzero(game == g)[0]
        rows = rows[np.argsort(move[rows], kind="stable")]
        late = np.nonzero(n_free[rows] <= max_free)[0]
        if not len(late):
            continue
        cand = rows[late[0]:]
        root = int(cand[0])
        roots.append(root)
        root_of[cand] = root
        served = [int(r) for r in cand if not subset_test or not (free[r] & ~free[root]).any()]
        facts = facts_for(x[root], x[served]) if served else []
        for r in cand:
            status[r] = "unserved"
        for r, f in zip(served, facts):
            status[r] = "finished" if f["finished"] else "relabel"
            if not f["finished"]:
                v[r], O[r] = int(f["v"]), list(f["O"])
    roots.sort(key=lambda r: (-int(n_free[r]), int(game[r])))
    return dict(root_of=root_of, roots=np.asarray(roots, np.int64), status=status, v=v, O=O, n_free=n_free, games=len(set(game.tolist())))


def apply_with(R, C, packed, p, pi_mode, z_mode, max_free, first_word_only=False, low_halves=False, fallback=True):
    """replay_targets_ref.apply, line for line, except where a switch says otherwise"""
    pm = RR.PI_MODES[pi_mode]
    HW, F, A = FX.dims(R, C)
    out = np.array(packed, dtype=np.uint8, copy=True)
    meta, _, vis = RR.fields(R, C, packed)
    if low_halves:
        vis = vis & 0xFFFF
    st = dict.fromkeys(RR.STATS, 0)
    by_free = np.zeros(max_free + 1, np.int64)
    for r in range(len(out)):
        s = p["status"][r]
        if s in ("unserved", "finished"):
            st[s] += 1
        if s != "relabel":
            continue
        st["relabelled"] += 1
        by_free[p["n_free"][r]] += 1
        v, O = p["v"][r], [a for a in p["O"][r] if a < 64 or not first_word_only]
        st["z_changed"] += int(int(meta["z"][r]) != v)
        if z_mode:
            out[r, M0 - 3] = np.int8(v).view(np.uint8)
        if pm:
            new = np.zeros(A, np.int64)
            if pm == 2 and (int(vis[r][O].astype(np.int64).sum()) != 0 or not fallback):
                new[O] = vis[r][O]
            else:
                new[O] = 1
            out[r, M0 + 2 * F:M0 + 2 * F + 4 * A] = new.astype("<i4").view(np.uint8)
    st.update(rows=len(out), games=p["games"], roots=len(p["roots"]), chunks=-(-len(p["roots"]) // 3))
    st["by_free"] = by_free
    return out, st


def answer(R, C, max_free, plan_switches={}, apply_switches={}):
    """everything the GPU test compares, as one tuple: the rows after the call in every mode, the stats, root_of, the roots in order"""
    c = FX.relabel_case(R, C, max_free)
    p = plan_with(R, C, c["packed"], max_free, c["facts_for"], **plan_switches)
    out = []
    for pi_mode in ("keep", "uniform", "restrict"):
        rows, st = apply_with(R, C, c["packed"], p, pi_mode, True, max_free, **apply_switches)
        out += [rows.tobytes(), tuple(st[k] for k in RR.STATS), st["by_free"].tobytes()]
    return tuple(out) + (p["root_of"].tobytes(), tuple(p["roots"].tolist()))


_answers = {}


def baseline(R, C, max_free):
    if (R, C, max_free) not in _answers:
        _answers[(R, C, max_free)] = answer(R, C, max_free)
    return _answers[(R, C, max_free)]


# ---------------------------------------------------------------- the relabel fixture
@pytest.mark.parametrize("R,C,max_free", FX.RELABEL_CASES)
def test_relabel_fixture_reaches_what_it_is_for(R, C, max_free):
    c = FX.relabel_case(R, C, max_free)
    packed, p = c["packed"], c["plan"]
    HW, F, A = FX.dims(R, C)
    meta, x, vis = RR.fields(R, C, packed)
    status = np.array([str(s) for s in p["status"]])
    rel = np.nonzero(status == "relabel")[0]
    whole_game = c["E"] <= max_free  # 1x1: see the module's docstring
    assert len(rel) >= 40 and (status == "finished").sum() >= 10
    assert (status == "unserved").sum() == (0 if whole_game else 1)
    assert (c["foreign"] is None) == whole_game and (whole_game or status[c["foreign"]] == "unserved")
    assert (p["n_free"] > max_free).any() != whole_game and (p["root_of"][p["n_free"] > max_free] == -1).all()
    assert sum(len(p["O"][r]) > 1 for r in rel) >= 8
    for w in range(-(-A // 64)):
        assert sum(any(a // 64 == w for a in p["O"][r]) for r in rel) >= 8, w
    on_O = [vis[r][p["O"][r]].astype(np.int64) for r in rel]
    assert any(v.sum() == 0 for v in on_O), "no fallback row"
    assert any(v.max() >= 65536 for v in on_O), "no kept visit past 16 bits"
    # ... and one that is zeroed (on 1x1 every free edge keeps the result on most rows: not asked for there)
    assert whole_game or any((np.delete(vis[r], p["O"][r]) >= 65536).any() for r in rel)
    values = {p["v"][r] for r in rel}
    assert values == ({-1, 0, 1} if (R * C) % 2 == 0 else {-1, 1})
    # the keys: 16 games over the signed range, rows in no order, a game from below 0, a game with gaps
    games = sorted(set(meta["game_idx"].tolist()))
    assert games == sorted(FX.GAME_IDX) and {-2 ** 31, -1, 0, 65536, 2 ** 31 - 1} <= set(games) and len(p["roots"]) == 16
    order = np.lexsort((meta["move_idx"], meta["game_idx"]))
    assert not np.array_equal(order, np.arange(len(packed)))
    steps = {g: np.diff(np.sort(meta["move_idx"][meta["game_idx"] == g].astype(np.int64))) for g in games}
    assert sum((s != 1).any() for s in steps.values()) == 1 and all((s > 0).all() for s in steps.values())
    assert sum(meta["move_idx"][meta["game_idx"] == g].min() < 0 for g in games) == 1
    # the restatement's own answer: equal to the copy above, z_changed > 0, nothing but z and the visits of relabelled rows moves
    for pi_mode in ("keep", "uniform", "restrict"):
        want, st = RR.apply(R, C, packed, p, pi_mode, True, n_tables=3, max_free=max_free)
        again, st2 = apply_with(R, C, packed, plan_with(R, C, packed, max_free, c["facts_for"]), pi_mode, True, max_free)
        assert np.array_equal(want, again) and all(st[k] == st2[k] for k in RR.STATS) and np.array_equal(st["by_free"], st2["by_free"])
        assert st["z_changed"] > 0 and st["relabelled"] == len(rel)
        changed = np.nonzero((want != packed).any(axis=1))[0]
        assert set(changed.tolist()) <= set(rel.tolist())
    assert np.array_equal(plan_with(R, C, packed, max_free, c["facts_for"])["roots"], p["roots"])


MISTAKES = [
    ("O cut to the first ballot word", {}, dict(first_word_only=True), lambda R, C, mf: 2 * (R + 1) * (C + 1) > 64),
    ("visits rebuilt from their low halves", {}, dict(low_halves=True), lambda R, C, mf: True),
    ("games ordered by unsigned game_idx", dict(unsigned_game=True), {}, lambda R, C, mf: True),
    ("moves ordered by unsigned move_idx", dict(unsigned_move=True), {}, lambda R, C, mf: True),
    ("the fallback of rows with no visit on O dropped", {}, dict(fallback=False), lambda R, C, mf: True),
    ("the subset test dropped", dict(subset_test=False), {}, lambda R, C, mf: 2 * R * C + R + C > mf),
]


@pytest.mark.parametrize("name,plan_switches,apply_switches,applies", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_a_mistake_in_the_relabel_changes_the_answer_on_every_board(name, plan_switches, apply_switches, applies):
    for R, C, max_free in FX.RELABEL_CASES:
        if applies(R, C, max_free):
            assert answer(R, C, max_free, plan_switches, apply_switches) != baseline(R, C, max_free), (name, R, C, max_free)


# ---------------------------------------------------------------- the dataset fixture
def lexicographic(x):
    """the rows' distinct values in ascending lexicographic order, and each row's group"""
    keys, inv = np.unique(x, axis=0, return_inverse=True)
    return keys, np.asarray(inv).ravel()


@pytest.mark.parametrize("R,C", FX.DATASET_BOARDS)
def test_dataset_fixture_reaches_what_it_is_for(R, C):
    d = FX.dataset_case(R, C)
    HW, F, A = FX.dims(R, C)
    KW = d["KW"]
    x, n = d["x"], len(d["x"])
    keys, inv = lexicographic(x)
    counts = np.bincount(inv)
    assert 400 <= n <= 600 and 1 < len(keys) < n and counts.max() >= 5 and counts.min() >= 1 and counts.max() <= 9
    assert ((x[:, :A] == 0) | (x[:, :A] == 1)).all() and (x[:, A:] == x[:, A:A + 1]).all()
    assert (d["visits"] >= 65536).any() and d["visits"].sum(axis=1, dtype=np.int64).max() < 2 ** 31 and d["visits"].sum(axis=1).min() > 0
    assert set(d["z"].tolist()) == {-1, 0, 1}
    # the key restated: KW words that order the positions as the lexicographic comparison of x does
    kw = FX.key_words(R, C, keys)
    assert kw.shape == (len(keys), KW) and KW == -(-(A + 16) // 64)
    assert all(tuple(kw[i]) < tuple(kw[i + 1]) for i in range(len(keys) - 1))
    differ = kw[:, None, :] != kw[None, :, :]  # [P, P, KW]
    for w in range(KW):
        only = differ[:, :, w] & (differ.sum(axis=2) == 1)
        assert only.any(), "no two groups differ in key word %d only" % w
    same_edges = (keys[:, None, :A] == keys[None, :, :A]).all(axis=2)
    p2 = keys[:, A].astype(np.int64)
    base = int(np.nonzero((keys == d["positions"][0]).all(axis=1))[0][0])
    assert (same_edges & (p2[:, None] < 0) & (p2[None, :] > 0)).any() and {-32768, -1, 0, 1, 32767} <= set(p2[same_edges[base]].tolist())
    # staging: two calls, the first through a selection, ten rows in both, then a permutation
    staged = np.concatenate([d["rows_a"][d["sel"]], d["rows_b"]])
    assert np.array_equal(staged, d["staged"]) and staged.shape == (n, d["row_bytes"]) and d["row_bytes"] == (28 + 2 * F + 4 * A + 7) // 8 * 8
    assert len(set(d["sel"].tolist())) == len(d["sel"]) < len(d["rows_a"]) and not np.array_equal(np.sort(d["sel"]), d["sel"])
    assert sorted(d["order"].tolist()) == list(range(n)) and not np.array_equal(d["order"], np.arange(n))
    _, sx, sv = RR.fields(R, C, staged)
    assert np.array_equal(sx[d["order"]], x) and np.array_equal(sv[d["order"]], d["visits"])
    n1 = len(d["sel"])
    both = {r.tobytes() for r in staged[:n1, M0:M0 + 2 * F + 4 * A]} & {r.tobytes() for r in staged[n1:, M0:M0 + 2 * F + 4 * A]}
    assert len(both) == 10


def test_a_mistake_in_the_dataset_build_changes_the_answer():
    reversed_differs = 0
    for R, C in FX.DATASET_BOARDS:
        d = FX.dataset_case(R, C)
        HW, F, A = FX.dims(R, C)
        x, visits, z = d["x"], d["visits"], d["z"]
        f, pi, v = T.assemble_dataset(x, visits, z, True)
        # keys cut to their first KW - 1 words: groups merge
        if d["KW"] >= 2:
            assert len(np.unique(FX.key_words(R, C, x)[:, :d["KW"] - 1], axis=0)) < len(f), (R, C)
        # plane 2 compared as unsigned: the groups come in another order
        u = x.astype(np.int64)
        u[:, A:] &= 0xFFFF
        assert not np.array_equal(lexicographic(u)[0].astype(np.uint16).view(np.int16), f), (R, C)
        # a group's rows summed in reverse order
        f2, pi2, v2 = T.assemble_dataset(x[::-1], visits[::-1], z[::-1], True)
        assert np.array_equal(f2, f)
        reversed_differs += int((pi2.view(np.uint32) != pi.view(np.uint32)).any() or (v2.view(np.uint32) != v.view(np.uint32)).any())
    assert reversed_differs >= 1


def test_big_dataset_case_takes_a_second_round():
    packed, x, visits, z = FX.dataset_big_case()
    assert len(packed) == 40000 > 256 * 32 * 4 and packed.shape[1] == 88
    keys, inv = lexicographic(x)
    assert 1 < len(keys) < 40000 // 8 and (visits >= 65536).any() and visits.sum(axis=1, dtype=np.int64).max() < 2 ** 31


# ---------------------------------------------------------------- the symmetry table, a host call
@pytest.mark.parametrize("R,C", FX.DATASET_BOARDS)
def test_host_symmetry_table_equals_the_oracle(R, C):
    A = 2 * (R + 1) * (C + 1)
    for sym in range(8 if R == C else 4):
        got = symmetry_table(R, C, sym)
        assert got.dtype == np.int32 and np.array_equal(got, T.symmetry_lut(R + 1, C + 1, sym)), sym
        assert sorted(got.tolist()) == list(range(A))
    if R != C:
        for sym in range(4, 8):
            with pytest.raises(_lib.DbazError):
                symmetry_table(R, C, sym)
