"""CPU: the restatement of the random-walk diffusion (tests/diffusion_reference.py) -- the generator's known answers,
the deviates, the pin of its three loops to the existing restatements at Kh = 0, the kick's statistics, what the
kick does to the shared seeds (so that the GPU tests compare something that exercises the walk), the keying, and the
new names.  No GPU.  Kh is in m^2/s throughout."""
import math
import os
import re

import numpy as np
import pytest

import diffusion_reference as D
import layer_reference as LR
import pathline_attr_reference as R
import rk4_relocate_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYER = 4
SEED = 2024
KH = 2e4

PHILOX_KAT = (
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


@pytest.fixture(scope="module")
def derived(oracle_lib, small_case):
    mesh, s0, s1 = small_case
    return mesh, oracle_lib.preprocess(mesh, s0), oracle_lib.preprocess(mesh, s1)


# ---- Philox and the deviates --------------------------------------------------------------------------------
def test_philox_known_answers():
    for ctr, key, want in PHILOX_KAT:
        assert " ".join("%08x" % w for w in D.philox4x32_10(ctr, key)) == want


def test_deviates():
    h = 2.0 ** -32  # 0.5 * 2^-31
    assert D.deviate(0) == h
    assert D.deviate(0x7FFFFFFF) == 1.0 - h
    assert D.deviate(0x80000000) == -(1.0 - h)
    assert D.deviate(0xFFFFFFFF) == -h
    for w in (0, 1, 0x7FFFFFFF, 0x12345678):  # symmetric: w and ~w mirror each other; never 0, inside (-1, 1)
        assert D.deviate(w) == -D.deviate(w ^ 0xFFFFFFFF)
        assert 0.0 < abs(D.deviate(w)) < 1.0


# ---- the pin at Kh = 0 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_pin_layer(oracle_lib, derived, backward):
    O = oracle_lib
    mesh, r0, r1 = derived
    for back in (None, r1):
        for euler, relocate in ((True, False), (False, False), (False, True)):
            want = LR.run_shared(O, mesh, r0, back, LAYER, euler=euler, backward=backward, relocate=relocate)
            got = D.run_shared(O, mesh, r0, back, layer=LAYER, euler=euler, backward=backward, relocate=relocate,
                               kh=0.0, seed=SEED)
            for k in ("rec_pos", "rec_vel", "final_pos", "final_depth", "death", "final_cell"):
                assert np.array_equal(got[k], want[k]), (k, back is not None, euler, relocate)
            assert int((want["death"] < 0).sum()) >= 20
            assert not got["kick_changes"].any()


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_pin_path(oracle_lib, derived, backward):
    O = oracle_lib
    mesh, r0, r1 = derived
    for euler in (True, False):
        want = R.run_shared(O, mesh, r0, r1, euler, backward, names=[])
        got = D.run_shared(O, mesh, r0, r1, euler=euler, backward=backward, kh=0.0, seed=SEED)
        for k in ("rec_pos", "rec_vel", "final_pos", "final_depth", "death"):
            assert np.array_equal(got[k], want[k]), (k, euler)
        assert int((want["death"] < 0).sum()) >= 20


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_pin_path_relocate(oracle_lib, derived, backward):
    O = oracle_lib
    mesh, r0, r1 = derived
    want = RR.run_shared(O, mesh, r0, r1, backward=backward, relocate=True)
    got = D.run_shared(O, mesh, r0, r1, euler=False, backward=backward, relocate=True, kh=0.0, seed=SEED)
    for k in ("rec_pos", "rec_vel", "final_pos", "final_depth", "death"):
        assert np.array_equal(got[k], want[k]), k
    assert int((want["death"] < 0).sum()) >= 20


# ---- kick statistics (deterministic: seed 7) -----------------------------------------------------------------
def _start(small_case):
    mesh = small_case[0]
    rad = float(np.linalg.norm(np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)[0]))
    return (4e6, 3e6, math.sqrt(rad * rad - 4e6 * 4e6 - 3e6 * 3e6)), rad


def test_kick_variance_and_radius(small_case):
    p, rad = _start(small_case)
    s, n = 1000.0, 4096
    pa = np.array(p)
    e = np.array([-p[1], p[0], 0.0]) / math.hypot(p[0], p[1])
    nn = np.cross(pa / rad, e)
    de, dn, dr = np.empty(n), np.empty(n), np.empty(n)
    for i in range(n):
        R1, R2 = D.deviates(7, i, 0, 0)
        q = np.array(D.kick(p, s, R1, R2))
        de[i], dn[i] = np.dot(q - pa, e), np.dot(q - pa, nn)
        dr[i] = np.linalg.norm(q) - np.linalg.norm(pa)
    ve, vn = float(np.var(de)) / (s * s), float(np.var(dn)) / (s * s)
    print(f"variance / s^2 along e {ve:.4f}, along n {vn:.4f}; max |radius change| {np.abs(dr).max():.3e} m")
    # 5 sigma of the variance estimator of a uniform deviate, 0.894 / sqrt(N) relative = 7% at N = 4096
    assert abs(ve * 3.0 - 1.0) < 0.07
    assert abs(vn * 3.0 - 1.0) < 0.07
    assert np.abs(dr).max() < 1e-8


def test_kick_mean_squared_displacement(small_case):
    p, rad = _start(small_case)
    s, n, m = 1000.0, 1024, 256
    pa = np.array(p)
    msd = 0.0
    for i in range(n):
        q = p
        for step in range(m):
            R1, R2 = D.deviates(7, i, step, 0)
            q = D.kick(q, s, R1, R2)
        c = float(np.dot(np.array(q), pa)) / (float(np.linalg.norm(q)) * rad)
        cr = np.linalg.norm(np.cross(np.array(q), pa)) / (float(np.linalg.norm(q)) * rad)
        msd += (rad * math.atan2(cr, c)) ** 2
    ratio = msd / n / (m * (2.0 / 3.0) * s * s)
    print(f"mean squared great-circle displacement / (256 (2/3) s^2) = {ratio:.4f}")
    assert abs(ratio - 1.0) < 0.16  # 5 sigma at 1 / sqrt(N), N = 1024


# ---- survival: the kick exercises the walk without becoming the only thing tested -----------------------------
@pytest.mark.parametrize("euler,relocate", [(True, False), (False, True)], ids=["euler", "rk4-relocate"])
def test_survival(oracle_lib, derived, euler, relocate):
    O = oracle_lib
    mesh, r0, r1 = derived
    plain = D.run_shared(O, mesh, r0, r1, layer=LAYER, euler=euler, relocate=relocate, kh=0.0)
    dif = D.run_shared(O, mesh, r0, r1, layer=LAYER, euler=euler, relocate=relocate, kh=KH, seed=SEED)
    alive, alive0 = dif["death"] < 0, plain["death"] < 0
    differ = int((dif["final_cell"] != plain["final_cell"]).sum())
    new_deaths = int((~alive & alive0).sum())
    print(f"Kh={KH:g}, s={D.kick_scale(KH, R.DELTA_T) / 1e3:.1f} km: alive {int(alive.sum())} (without diffusion "
          f"{int(alive0.sum())}), final cell differs {differ}, deaths the plain run does not have {new_deaths}, "
          f"kick-induced cell changes {int(dif['kick_changes'].sum())}")
    assert int(alive.sum()) >= 80
    assert differ >= 30
    assert new_deaths >= 1


def test_kick_moves_particles_across_pentagon_edges(oracle_lib, derived):
    O = oracle_lib
    mesh, r0, r1 = derived
    seeds, depths, _ = RR.pentagon_seeds(mesh)
    dif = D.run_case(O, mesh, r0, r1, seeds, depths, layer=LAYER, euler=True, kh=KH, seed=SEED)
    n = int(dif["kick_changes_poly"].sum())
    print(f"pentagon seeds: kick-induced cell changes {int(dif['kick_changes'].sum())}, with a pentagon on one side {n}")
    assert n >= 1


# ---- keying --------------------------------------------------------------------------------------------------
def test_keying(oracle_lib, derived):
    O = oracle_lib
    mesh, r0, r1 = derived
    seeds, depths = R.shared_seeds()
    cells = O.knn(mesh, seeds)
    kw = dict(layer=LAYER, euler=True, kh=KH, cells=cells)
    a = D.run_case(O, mesh, r0, r1, seeds, depths, seed=SEED, epoch=0, **kw)
    b = D.run_case(O, mesh, r0, r1, seeds, depths, seed=SEED + 1, epoch=0, **kw)
    c = D.run_case(O, mesh, r0, r1, seeds, depths, seed=SEED, epoch=1, **kw)
    for other in (b, c):
        live = (a["death"] != 0) & (other["death"] != 0)  # (made at least one step, so got at least one kick)
        assert int(live.sum()) >= 80
        assert np.all(np.any(a["final_pos"][live] != other["final_pos"][live], axis=1))
        moved = (a["death"] < 0) & (other["death"] < 0)
        assert np.all(np.any(a["rec_pos"][moved, 1:] != other["rec_pos"][moved, 1:], axis=(1, 2)))
    # the same particles in another seed order, each keeping its id: the same line per id
    perm = np.random.default_rng(3).permutation(len(seeds))
    d = D.run_case(O, mesh, r0, r1, seeds[perm], depths[perm], seed=SEED, epoch=0, ids=perm, layer=LAYER, euler=True,
                   kh=KH, cells=cells[perm])
    for k in ("rec_pos", "rec_vel", "final_pos", "death"):
        assert np.array_equal(d[k], a[k][perm]), k
    # ... and id_base continues a numbering
    e = D.run_case(O, mesh, r0, r1, seeds[40:], depths[40:], seed=SEED, epoch=0, id_base=40, layer=LAYER, euler=True,
                   kh=KH, cells=cells[40:])
    assert np.array_equal(e["rec_pos"], a["rec_pos"][40:])


# ---- names ---------------------------------------------------------------------------------------------------
def test_names_in_header_binding_and_library(engine_lib):
    from mops_amd import _lib
    text = open(os.path.join(ROOT, "include", "mops_traj.h")).read()
    for name in ("mops_traj_advance_diffuse", "mops_traj_advance_layer_diffuse", "mops_run_trajectories_diffuse",
                 "mops_run_trajectories_layer_diffuse", "mops_selftest_philox", "mops_diffusion_scale"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED
        assert hasattr(engine_lib, name)
    assert re.search(r"\}\s*mops_diffusion\s*;", text)
    assert engine_lib.mops_abi_version() == 4
    assert engine_lib.mops_diffusion_scale(100.0, -60) == D.kick_scale(100.0, 60) == math.sqrt(36000.0)


def test_settings_default_to_zero():
    from mops_amd.engine import TrajectoryConfig
    cfg = TrajectoryConfig()
    assert (cfg.diffusivity, cfg.seed, cfg.epoch) == (0.0, 0, 0)
    assert cfg.diffusion() is None
    from mops_amd import pyMOPS
    ts = pyMOPS.TrajectorySettings()
    assert (ts.diffusivity, ts.randomSeed, ts.randomEpoch) == (0.0, 0, 0)
    text = open(os.path.join(ROOT, "include", "mops", "MOPS.h")).read()
    for decl in ("double diffusivity = 0.0;", "unsigned long long randomSeed = 0;", "unsigned int randomEpoch = 0;"):
        assert decl in text, decl
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            TrajectoryConfig(diffusivity=bad).diffusion()
