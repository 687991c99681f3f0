"""Deep exact targets on packed replay rows (dbaz_replay_exact_targets in csrc/solver.hip) on every row layout: one, two, three and
four ballot words with the last one partial or full, visits 4-byte and 2-byte aligned, square and not, the flagship 6x6 and the
layered solve above 16 free edges, down to the 1x1 board.  The rows are replay_rows_fixture.relabel_case's -- game_idx over the
whole signed range, move_idx below 0 and with gaps, visits past 16 bits, rows with no visit on a free edge, a row its root does not
serve, in a random order -- and test_replay_rows_fixture_cpu.py says what they reach.  The reference is numpy alone:
replay_targets_ref.py over targets_ref.solve_rows, and the numpy recurrence for the tables.  Integers and bytes: no tolerances."""
import numpy as np
import pytest

from dotsboxesaz_amd.endgame import DeepTables
import replay_rows_fixture as FX
import replay_targets_ref as RR
from test_hip_deep_endgame import ref_table
from test_hip_deep_tables import MODES
from test_hip_replay_targets import check_stats, dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,C,max_free", FX.RELABEL_CASES)
def test_relabelled_rows_equal_the_restatement_in_every_mode(R, C, max_free):
    c = FX.relabel_case(R, C, max_free)
    packed, p = c["packed"], c["plan"]
    t = DeepTables(R, C, max_free=max_free, n_tables=3)  # 16 roots: six chunks, the last of one
    for pi_mode, z_mode in MODES:
        want, st = RR.apply(R, C, packed, p, pi_mode, z_mode, n_tables=3, max_free=max_free)
        rows_dev = dev(packed)
        got = t.replay_targets(rows_dev, pi_mode, z_mode, return_roots=True)
        out = rows_dev.cpu().numpy()
        assert np.array_equal(out, want), (pi_mode, z_mode, np.nonzero((out != want).any(axis=1))[0][:8])  # whole rows: meta and padding too
        check_stats(got, st, max_free)
        assert (got["roots"], got["chunks"], got["games"]) == (16, 6, 16)
        assert np.array_equal(got["root_of"].cpu().numpy(), p["root_of"]), (pi_mode, z_mode)
        assert (want != packed).any() == (pi_mode != "keep" or z_mode)
    t.close()


@pytest.mark.parametrize("R,C,max_free", FX.RELABEL_CASES)
def test_device_built_roots_solve_the_numpy_tables(R, C, max_free):
    """One chunk of all 16 roots, then every root's table against the numpy recurrence on the root's row: k_replay_roots' compact
    edges and box neighbours for action slots in every ballot word, without going through the relabel.  (A numpy table of 18
    free edges takes a twentieth of a second: all 16 roots in every case.)"""
    c = FX.relabel_case(R, C, max_free)
    packed, p = c["packed"], c["plan"]
    x = RR.fields(R, C, packed)[1]
    t = DeepTables(R, C, max_free=max_free, n_tables=16)
    rows_dev = dev(packed)
    got = t.replay_targets(rows_dev, "keep", False)
    assert got["chunks"] == 1 and t.n_solved == 16 and np.array_equal(rows_dev.cpu().numpy(), packed)
    assert (np.diff(t.n_free) <= 0).all() and np.array_equal(t.n_free, p["n_free"][p["roots"]])  # the plan's order
    for i in range(16):
        want = ref_table(R, C, x[p["roots"][i]])
        assert np.array_equal(t.table(i), want) and t.d0[i] == want[0], i
    t.close()


@pytest.mark.parametrize("R,C,max_free", FX.RELABEL_CASES)
def test_relabelled_rows_relabel_to_themselves(R, C, max_free):
    c = FX.relabel_case(R, C, max_free)
    t = DeepTables(R, C, max_free=max_free, n_tables=3)
    rows_dev = dev(c["packed"])
    first = t.replay_targets(rows_dev, "restrict", True)
    once = rows_dev.cpu().numpy()
    second = t.replay_targets(rows_dev, "restrict", True)
    assert np.array_equal(rows_dev.cpu().numpy(), once) and (once != c["packed"]).any()
    for k in RR.STATS:
        assert second[k] == (0 if k == "z_changed" else first[k]), k
    assert first["z_changed"] > 0 and np.array_equal(second["by_free"], first["by_free"])
    t.close()
