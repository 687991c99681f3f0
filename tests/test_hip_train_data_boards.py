"""The dataset build and batch path (dbaz_dataset_* / dbaz_symmetry_apply in csrc/replay.hip) on every layout the kernels tell
apart: one to five key words, the 16 key bits of plane 2 inside a word, filling one exactly, straddling two or alone in the last,
one to four pi values per lane, x rows padded by 0 to 3 shorts, visits 4-byte and 2-byte aligned, square boards and not.  The rows
are replay_rows_fixture.dataset_case's, staged in two calls (one through a selection) and reordered at dataset_finish;
test_replay_rows_fixture_cpu.py says what they reach.  Against oracle/train_ref.py, bit for bit: integer and permutation work,
and float64 Kahan means cast to float32."""
import numpy as np
import pytest

from oracle import train_ref as T
import replay_rows_fixture as FX

pytestmark = pytest.mark.gpu


def engine(R, C):
    from dotsboxesaz_amd.engine import Engine
    return Engine(R, C, 4, evaluator="formula")


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_dataset(e, want, m):
    f, pi, z = want
    x_d, pi_d, z_d = e.dataset_fetch()
    assert m == len(f) == len(x_d)
    assert np.array_equal(x_d, f) and same_bits(pi_d, pi) and same_bits(z_d, z)


def stage_two_calls(e, d, avg):
    e.dataset_begin()
    e.dataset_add_rows(dev(d["rows_a"]), d["sel"])
    e.dataset_add_rows(dev(d["rows_b"]))
    return e.dataset_finish(avg, order=d["order"])


@pytest.mark.parametrize("R,C", FX.DATASET_BOARDS)
def test_dataset_equals_the_oracle(R, C):
    d = FX.dataset_case(R, C)
    e = engine(R, C)
    assert e.row_bytes == d["row_bytes"] == d["rows_a"].shape[1]
    for avg in (False, True):
        want = T.assemble_dataset(d["x"], d["visits"], d["z"], avg)
        m = stage_two_calls(e, d, avg)
        check_dataset(e, want, m)
        if avg:  # groups in ascending lexicographic order of x
            assert 1 < m < len(d["x"])
            diff = np.diff(e.dataset_fetch()[0].astype(np.int32), axis=0)
            assert (diff[np.arange(m - 1), (diff != 0).argmax(axis=1)] > 0).all()
    # the same rows in one call, no selection, no order: the same groups, each mean taken in staging order
    sx, sv, sz = d["staged_fields"]
    e.dataset_begin()
    e.dataset_add_rows(dev(d["staged"]))
    m = e.dataset_finish(True)
    check_dataset(e, T.assemble_dataset(sx, sv, sz, True), m)
    e.close()


@pytest.mark.parametrize("R,C", FX.DATASET_BOARDS)
def test_batches_under_every_symmetry(R, C):
    from dotsboxesaz_amd._lib import DbazError
    d = FX.dataset_case(R, C)
    e = engine(R, C)
    f, pi, z = T.assemble_dataset(d["x"], d["visits"], d["z"], True)
    m = stage_two_calls(e, d, True)
    check_dataset(e, (f, pi, z), m)
    idx = np.random.RandomState(R * 16 + C).randint(0, m, size=1031)  # more indices than rows: repeats
    boards = f[idx].astype(np.float32).reshape(-1, 3, R + 1, C + 1)

    def check_batch(sym):
        b, p, zz = e.dataset_batch(idx, sym)
        want_b, want_p = T.apply_symmetry(boards, pi[idx], sym)
        assert same_bits(b.cpu().numpy(), np.ascontiguousarray(want_b)) and same_bits(p.cpu().numpy(), np.ascontiguousarray(want_p)), sym
        assert same_bits(zz.cpu().numpy().ravel(), z[idx])
        return b, p
    b0, p0 = check_batch(0)
    for sym in range(1, 8 if R == C else 4):
        b, p = check_batch(sym)
        b2, p2 = e.symmetry_apply(sym, b0, p0)  # the caller-tensor kernel on the untransformed batch
        assert np.array_equal(b2.cpu().numpy(), b.cpu().numpy()) and np.array_equal(p2.cpu().numpy(), p.cpu().numpy()), sym
    if R != C:
        for sym in range(4, 8):
            with pytest.raises(DbazError):
                e.dataset_batch(idx, sym)
            with pytest.raises(DbazError):
                e.symmetry_apply(sym, b0, p0)
            check_batch(sym - 4)  # the next legal batch is still right
    e.close()


@pytest.mark.parametrize("R,C", FX.DATASET_BOARDS)
def test_rows_that_are_no_feature_rows_are_refused(R, C):
    """A row whose plane 2 is not constant (its last value, in the x row's last, padded unit) and a row with a 2 on the last
    edge-plane slot, each among good rows: the call is refused and the rows staged before stay as they were."""
    from dotsboxesaz_amd._lib import DbazError
    import replay_targets_ref as RR
    d = FX.dataset_case(R, C)
    HW, F, A = FX.dims(R, C)
    sx, sv, sz = d["staged_fields"]
    e = engine(R, C)
    e.dataset_begin()
    e.dataset_add_rows(dev(d["staged"][:50]))
    for at, to in ((F - 1, lambda v: v ^ 1), (A - 1, lambda v: 2)):
        bad_x = sx[50:55].copy()
        bad_x[3, at] = to(bad_x[3, at])
        with pytest.raises(DbazError):
            e.dataset_add_rows(dev(RR.pack(R, C, 0, 0, bad_x, sv[50:55], sz[50:55])))
    e.dataset_add_rows(dev(d["staged"]), np.arange(50, 60))
    assert e.dataset_finish(False) == 60
    check_dataset(e, T.assemble_dataset(sx[:60], sv[:60], sz[:60], False), 60)
    e.close()


def test_40000_rows_take_the_block_uniform_loops_round_again():
    """1x1, 88 bytes a row: k_ds_stage and k_make_batch take 32 768 rows a round, so 40 000 staged rows and a batch of 40 000
    indices go round twice, the second time with idle waves.  Everything is compared with the oracle."""
    packed, x, visits, z = FX.dataset_big_case()
    e = engine(1, 1)
    rows = dev(packed)
    e.dataset_begin()
    e.dataset_add_rows(rows)
    m = e.dataset_finish(False)
    f, pi, v = T.assemble_dataset(x, visits, z, False)
    check_dataset(e, (f, pi, v), m)
    idx = np.random.RandomState(3).randint(0, m, size=40000)
    b, p, zz = e.dataset_batch(idx, 3)
    want_b, want_p = T.apply_symmetry(f[idx].astype(np.float32).reshape(-1, 3, 2, 2), pi[idx], 3)
    assert same_bits(b.cpu().numpy(), np.ascontiguousarray(want_b)) and same_bits(p.cpu().numpy(), np.ascontiguousarray(want_p))
    assert same_bits(zz.cpu().numpy().ravel(), v[idx])
    e.dataset_begin()
    e.dataset_add_rows(rows)
    m = e.dataset_finish(True)
    check_dataset(e, T.assemble_dataset(x, visits, z, True), m)
    assert 1 < m < 40000
    e.close()
