"""CPU: the restatement of the pathline RK4 loop with a ``relocate`` switch (tests/rk4_relocate_reference.py) is
pinned to the CPU oracle bit for bit with the switch off, and with it on covers the cases the GPU tests of
MOPS_RK4_RELOCATE rely on; the constant and the pyMOPS setting exist.  No GPU."""
import os
import re

import numpy as np
import pytest

import pathline_attr_reference as R
import rk4_relocate_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def derived(oracle_lib, small_case):
    mesh, s0, s1 = small_case
    return mesh, oracle_lib.preprocess(mesh, s0), oracle_lib.preprocess(mesh, s1)


@pytest.fixture(scope="module")
def shared(oracle_lib, derived):
    """The shared inputs under plain RK4, relocating RK4 and Euler, both directions; computed once, never modified."""
    mesh, r0, r1 = derived
    out = {}
    for backward in (False, True):
        out[("plain", backward)] = RR.run_shared(oracle_lib, mesh, r0, r1, backward=backward, relocate=False)
        out[("reloc", backward)] = RR.run_shared(oracle_lib, mesh, r0, r1, backward=backward, relocate=True)
        out[("euler", backward)] = R.run_shared(oracle_lib, mesh, r0, r1, True, backward)
    return out


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_switch_off_equals_oracle(oracle_lib, derived, shared, backward):
    mesh, r0, r1 = derived
    ref = shared[("plain", backward)]
    orc = oracle_lib.run(mesh, r0, r1, ref["seeds"], depths=ref["depths"], delta_t=R.DELTA_T, duration=R.DURATION,
                         record_t=R.RECORD_T, euler=False, backward=backward, cells=ref["cells"], n_threads=1)
    assert np.array_equal(ref["rec_pos"], orc["rec_pos"])
    assert np.array_equal(ref["rec_vel"], orc["rec_vel"])
    assert np.array_equal(ref["death"], orc["death"])
    assert np.array_equal(ref["final_depth"], orc["final_depth"])
    assert not ref["relocations"].any()


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_relocation_on_shared_inputs(shared, backward):
    plain, rel, eul = shared[("plain", backward)], shared[("reloc", backward)], shared[("euler", backward)]
    alive, alive_plain, alive_euler = rel["death"] < 0, plain["death"] < 0, eul["death"] < 0
    same = np.array([np.array_equal(rel["rec_pos"][i], plain["rec_pos"][i]) and
                     np.array_equal(rel["rec_vel"][i], plain["rec_vel"][i]) for i in range(R.N_SEEDS)])
    print(f"backward={backward}: alive {int(alive.sum())} (plain {int(alive_plain.sum())}, euler "
          f"{int(alive_euler.sum())}), dead at 0 {int((rel['death'] == 0).sum())}, dead later "
          f"{int((rel['death'] > 0).sum())}, relocations {int(rel['relocations'].sum())} (nv != 6: "
          f"{int(rel['relocations_poly'].sum())}), differing lines {int((~same).sum())}")
    assert int(alive.sum()) >= 80
    assert int(rel["relocations"].sum()) >= 50
    assert int((~same).sum()) >= 30
    assert np.all(alive[alive_euler])      # every particle alive under Euler is alive
    assert np.all(alive[alive_plain])      # ... and every one alive under plain RK4,
    assert np.all(same[alive_plain])       # with bit-identical lines
    assert np.array_equal(rel["final_pos"][alive_plain], plain["final_pos"][alive_plain])
    assert np.array_equal(rel["final_depth"][alive_plain], plain["final_depth"][alive_plain])


def test_pentagon_seeds(oracle_lib, derived):
    mesh, r0, r1 = derived
    seeds, depths, pent = RR.pentagon_seeds(mesh)
    assert len(pent) == 11 and seeds.shape == (66, 3)
    ref = RR.run_case(oracle_lib, mesh, r0, r1, seeds, depths)
    print(f"pentagon relocations {int(ref['relocations_poly'].sum())} of {int(ref['relocations'].sum())}, alive "
          f"{int((ref['death'] < 0).sum())}")
    assert int(ref["relocations_poly"].sum()) >= 10


def test_two_hop_deaths(oracle_lib, derived):
    mesh, r0, r1 = derived
    seeds, depths = R.shared_seeds()
    ref = RR.run_case(oracle_lib, mesh, r0, r1, seeds, depths, delta_t=RR.TWO_HOP_DELTA_T,
                      duration=RR.TWO_HOP_STEPS * RR.TWO_HOP_DELTA_T,
                      record_t=RR.TWO_HOP_RECORD_EVERY * RR.TWO_HOP_DELTA_T)
    late = (ref["death"] > 0) & (ref["relocations"] > 0)
    print(f"two-hop: dead after step 0 with relocations {int(late.sum())}, dead at 0 {int((ref['death'] == 0).sum())}, "
          f"alive {int((ref['death'] < 0).sum())}")
    assert int(late.sum()) >= 3


def test_constant_in_header_and_lib():
    from mops_amd import _lib
    text = open(os.path.join(ROOT, "include", "mops_traj.h")).read()
    m = re.search(r"\bMOPS_RK4_RELOCATE\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == 2
    assert _lib.MOPS_RK4_RELOCATE == 2
    assert (_lib.MOPS_RK4, _lib.MOPS_EULER) == (0, 1)


def test_pymops_setting_default():
    from mops_amd import pyMOPS
    assert pyMOPS.TrajectorySettings().relocateStages is False
