"""CPU: the restatement of the layer step (tests/layer_reference.py) is pinned to the CPU oracle bit for bit, its
``relocate`` switch covers what the GPU tests of the layer mode rely on, and the new names exist.  No GPU.

The pin.  With fields whose vertex zTop column is exactly 0, -100, -200, ... at every vertex and whose w is zero, a
depth-0 run of the oracle brackets layer 1 with t == 1.0 exactly: its velocity is v_level0 * 1 + v_level1 * 0 and its
vertical update moves nothing -- a layer-0 run.  So the oracle at depth 0 on such fields, with layer k's velocities
moved to level 0 (and other, non-zero, velocities on the levels below), must equal the restatement at layer k on the
original fields.  Particles the restatement kills by its zero-velocity rule are left out (the pathline oracle has
no such rule), and nothing else."""
import os
import re

import numpy as np
import pytest

import layer_reference as LR
import pathline_attr_reference as R
import rk4_relocate_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEFT_OUT = 16  # of the 96 shared seeds (8 of them lie on land)


@pytest.fixture(scope="module")
def derived(oracle_lib, small_case):
    mesh, s0, s1 = small_case
    return mesh, oracle_lib.preprocess(mesh, s0), oracle_lib.preprocess(mesh, s1)


def pinned_field(O, mesh, d, k):
    """``d`` with the exact flat column, w = 0, layer k's velocities at level 0 and (1, 2, 3) m/s -- never zero
    under weights that sum to one -- on the levels below."""
    V, L = mesh.nVertices, mesh.nVertLevels
    zt = np.tile(0.0 - 100.0 * np.arange(L, dtype=np.float64), (V, 1))
    vel = np.empty((V, L, 3))
    vel[:, 1:, :] = np.array([1.0, 2.0, 3.0])
    vel[:, 0, :] = np.asarray(d.vertex_vel).reshape(V, L, 3)[:, k, :]
    return O.Derived(zt.reshape(-1), vel.reshape(-1), np.zeros(V * (L + 1)))


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
@pytest.mark.parametrize("pathline", [False, True], ids=["streamline", "pathline"])
@pytest.mark.parametrize("k", [0, 4, -1], ids=["k0", "k4", "kLast"])
def test_pinned_to_oracle(oracle_lib, derived, k, pathline, euler, backward):
    O = oracle_lib
    mesh, r0, r1 = derived
    k = k % mesh.nVertLevels
    seeds, _ = R.shared_seeds()
    depths = np.zeros(len(seeds), dtype=np.float32)
    ref = LR.run_case(O, mesh, r0, r1 if pathline else None, seeds, depths, k, euler=euler, backward=backward)
    orc = O.run(mesh, pinned_field(O, mesh, r0, k), pinned_field(O, mesh, r1, k) if pathline else None, seeds,
                depths=depths, delta_t=R.DELTA_T, duration=R.DURATION, record_t=R.RECORD_T, euler=euler,
                backward=backward, cells=ref["cells"], n_threads=1)
    keep = ~ref["zero_killed"]
    print(f"k={k} pathline={pathline} euler={euler} backward={backward}: left out {int((~keep).sum())}, alive "
          f"{int((ref['death'] < 0).sum())}, dead at 0 {int((ref['death'] == 0).sum())}, dead later "
          f"{int((ref['death'] > 0).sum())}")
    assert int((~keep).sum()) <= MAX_LEFT_OUT
    assert int((ref["death"][keep] < 0).sum()) >= 20  # (the comparison is not of dead particles only)
    assert np.array_equal(ref["rec_pos"][keep], orc["rec_pos"][keep])
    assert np.array_equal(ref["rec_vel"][keep], orc["rec_vel"][keep])
    assert np.array_equal(ref["death"][keep], orc["death"][keep])
    assert np.array_equal(ref["final_pos"][keep], orc["final_pos"].reshape(-1, 3)[keep])
    assert np.array_equal(ref["final_depth"][keep], orc["final_depth"][keep])
    assert np.array_equal(ref["final_depth"], depths)  # w = 0: the depth never moves


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("pathline", [False, True], ids=["streamline", "pathline"])
def test_relocation(oracle_lib, derived, pathline, backward):
    O = oracle_lib
    mesh, r0, r1 = derived
    back = r1 if pathline else None
    k = 4
    plain = LR.run_shared(O, mesh, r0, back, k, euler=False, backward=backward, relocate=False)
    rel = LR.run_shared(O, mesh, r0, back, k, euler=False, backward=backward, relocate=True)
    eul = LR.run_shared(O, mesh, r0, back, k, euler=True, backward=backward)
    assert not plain["relocations"].any()
    alive, alive_plain, alive_euler = rel["death"] < 0, plain["death"] < 0, eul["death"] < 0
    n_reloc = int(rel["relocations"].sum())
    print(f"pathline={pathline} backward={backward}: alive {int(alive.sum())} (plain {int(alive_plain.sum())}, euler "
          f"{int(alive_euler.sum())}), stage relocations on the shared seeds {n_reloc}")
    assert np.all(alive[alive_euler])  # every particle alive under Euler is alive
    assert np.all(alive[alive_plain])
    for key in ("rec_pos", "rec_vel", "final_pos"):  # a particle whose stages never left its cell: plain RK4's bytes
        assert np.array_equal(rel[key][alive_plain], plain[key][alive_plain])
    if n_reloc < 20:  # (the shared seeds gave fewer: the pentagon seeds in addition)
        seeds, depths, _ = RR.pentagon_seeds(mesh)
        more = LR.run_case(O, mesh, r0, back, seeds, depths, k, euler=False, backward=backward, relocate=True)
        n_reloc += int(more["relocations"].sum())
        print(f"  with rk4_relocate_reference.pentagon_seeds: {n_reloc}")
    assert n_reloc >= 20


def test_names_in_header_binding_and_library(engine_lib):
    from mops_amd import _lib
    text = open(os.path.join(ROOT, "include", "mops_traj.h")).read()
    for name in ("mops_traj_advance_layer", "mops_field_layer_velocity"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED
        assert hasattr(engine_lib, name)
    assert engine_lib.mops_abi_version() == 4


def test_pymops_setting_default():
    from mops_amd import pyMOPS
    assert pyMOPS.TrajectorySettings().fixedLayer == -1


def test_config_default_is_depth_mode():
    from mops_amd.engine import TrajectoryConfig
    assert TrajectoryConfig().layer is None
