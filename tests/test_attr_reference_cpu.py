"""CPU: the Python restatement of the pathline loop with its attribute channel (tests/pathline_attr_reference.py)
is pinned to the CPU oracle bit for bit, and covers the cases the GPU attribute tests rely on; the new C ABI
entries exist and check their arguments.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pathline_attr_reference as R

K = R.DURATION // R.RECORD_T
RI = R.RECORD_T // R.DELTA_T


@pytest.fixture(scope="module")
def derived(oracle_lib, small_case):
    mesh, s0, s1 = small_case
    return mesh, oracle_lib.preprocess(mesh, s0), oracle_lib.preprocess(mesh, s1)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_restatement_equals_oracle(oracle_lib, derived, euler, backward):
    mesh, r0, r1 = derived
    ref = R.run_shared(oracle_lib, mesh, r0, r1, euler, backward)
    orc = oracle_lib.run(mesh, r0, r1, ref["seeds"], depths=ref["depths"], delta_t=R.DELTA_T, duration=R.DURATION,
                         record_t=R.RECORD_T, euler=euler, backward=backward, cells=ref["cells"], n_threads=1)
    # the restatement is the oracle's loop: every observable the oracle has, bit for bit
    assert np.array_equal(ref["rec_pos"], orc["rec_pos"])
    assert np.array_equal(ref["rec_vel"], orc["rec_vel"])
    assert np.array_equal(ref["death"], orc["death"])
    assert np.array_equal(ref["final_depth"], orc["final_depth"])
    # coverage the GPU tests rely on
    death = ref["death"]
    alive = death < 0
    print(f"euler={euler} backward={backward}: alive {int(alive.sum())}, dead at 0 {int((death == 0).sum())}, "
          f"dead at 1..{RI - 1} {int(((death >= 1) & (death < RI)).sum())}, dead later {int((death >= RI).sum())}, "
          f"changing cell {int((ref['cell_changes'] > 0).sum())}, "
          f"live depth-0 {int((alive & (ref['depths'] == 0)).sum())}")
    if euler:
        assert int((ref["cell_changes"] > 0).sum()) >= 20
    else:
        assert int(alive.sum()) >= 20
        assert int(((death >= 1) & (death < RI)).sum()) >= 1  # before the first record: the slot-0 pre-write
        assert int((death >= RI).sum()) >= 10
    assert int((alive & (ref["depths"] == 0)).sum()) >= 1
    # the sampled temperature is not the velocity x that quirk Q9 puts in its place
    assert ref["names"] == ["salinity", "temperature"]
    t = ref["rec_attr"][:, :, ref["names"].index("temperature")]
    assert alive.any() and np.all(t[alive] != ref["rec_vel"][alive, :, 0])


def test_attr_lines_cleanup_matches_oracle_fields(oracle_lib, derived):
    """attr_lines goes through the oracle's own assembly: its points are the oracle's lines'."""
    mesh, r0, r1 = derived
    ref = R.run_shared(oracle_lib, mesh, r0, r1, True, False)
    lines = R.attr_lines(oracle_lib, ref["seeds"], ref, K)
    assert lines.shape == (2, R.N_SEEDS, K + 1)
    dead0 = ref["death"] == 0
    assert dead0.any() and np.all(lines[:, dead0, :] == 0.0)  # never sampled: the slab's zeros
    assert np.all(lines[:, ref["death"] < 0, K] == 0.0)        # the appended entry


def test_new_symbols_resolve(engine_lib):
    for name in ("mops_traj_sample_attrs", "mops_traj_advance_sampled", "mops_traj_finalize_attrs",
                 "mops_run_pathline_attrs"):
        assert hasattr(engine_lib, name), name


def test_sample_attrs_null_handles(engine_lib):
    from mops_amd import _lib
    st = engine_lib.mops_traj_sample_attrs(None, None, None, None, None, 0, 1, None, None, None, 0, None)
    assert st == _lib.MOPS_ERR_INVALID
    assert engine_lib.mops_last_error().decode()
    cfg = _lib.TrajCfg(60, 3600, 600, 0, 1)
    st = engine_lib.mops_traj_advance_sampled(None, None, None, C.byref(cfg), None, 0, 1, None, 0, 1, None, None, None,
                                              0, None)
    assert st == _lib.MOPS_ERR_INVALID
    st = engine_lib.mops_run_pathline_attrs(None, None, None, C.byref(cfg), 0, None, None, C.c_float(0), None, None,
                                            None, None, None, None, None, None, None, 1, None, None, None, None)
    assert st == _lib.MOPS_ERR_INVALID
    st = engine_lib.mops_traj_finalize_attrs(1, 0, None, None, 0, 1, None, 0, None, None, None)
    assert st == _lib.MOPS_ERR_INVALID
