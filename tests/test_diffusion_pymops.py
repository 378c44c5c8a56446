"""GPU: pyMOPS.TrajectorySettings.diffusivity / randomSeed / randomEpoch -- with a diffusivity MOPS_RunStreamLine (in a
layer) and MOPS_RunPathLine (in a layer and at the depths) give the restatement's lines (tests/
diffusion_reference.py); 0, the default, is today's output whatever the seed; the refusals report an error and return
an empty list."""
import numpy as np
import pytest

import diffusion_reference as D
import pathline_attr_reference as R
from test_attr_pymops import _setup

pytestmark = pytest.mark.gpu

LAYER, KH, SEED, EPOCH = 4, 2e4, 2024, 3


def _settings(M, depths, method, layer, kh=KH, relocate=False):
    cfg = M.TrajectorySettings()
    assert (cfg.diffusivity, cfg.randomSeed, cfg.randomEpoch) == (0.0, 0, 0)
    cfg.deltaT, cfg.simulationDuration, cfg.recordT, cfg.depth = R.DELTA_T, R.DURATION, R.RECORD_T, 0.0
    cfg.methodType = method
    cfg.particle_depths = list(depths)
    cfg.relocateStages = relocate
    cfg.fixedLayer = layer
    cfg.diffusivity, cfg.randomSeed, cfg.randomEpoch = kh, SEED, EPOCH
    return cfg


def _equal(got, want, keys):
    assert len(got) == R.N_SEEDS
    for i in range(R.N_SEEDS):
        for k in keys:
            assert got[i][k].tobytes() == want[k][i].tobytes(), (i, k)


def test_pymops_diffusivity(engine_lib, oracle_lib, gpu, small_case, capfd):
    from mops_amd import engine
    O = oracle_lib
    mesh, s0, s1 = small_case
    r0, r1 = O.preprocess(mesh, s0), O.preprocess(mesh, s1)
    M = _setup(mesh, (s0, s1), ((), ()))
    K4, KE = M.CalcMethodType.kRK4, M.CalcMethodType.kEuler
    seeds, depths = R.shared_seeds()
    path_keys = ("points", "velocity", "temperature", "salinity", "lastPoint")
    kw = dict(kh=KH, seed=SEED, epoch=EPOCH)
    # a pathline in a layer (Euler) and at the depths (RK4 with relocated stages), a streamline in a layer (RK4)
    ref = D.run_shared(O, mesh, r0, r1, layer=LAYER, euler=True, **kw)
    assert int((ref["death"] < 0).sum()) >= 20 and int(ref["kick_changes"].sum()) >= 30
    on = M.MOPS_RunPathLine(_settings(M, depths, KE, LAYER), seeds)
    _equal(on, D.lines(O, ref, True), path_keys)
    ref = D.run_shared(O, mesh, r0, r1, layer=None, euler=False, relocate=True, **kw)
    _equal(M.MOPS_RunPathLine(_settings(M, depths, K4, -1, relocate=True), seeds), D.lines(O, ref, True), path_keys)
    ref = D.run_shared(O, mesh, r0, None, layer=LAYER, euler=False, **kw)
    _equal(M.MOPS_RunStreamLine(_settings(M, depths, K4, LAYER), seeds), D.lines(O, ref, False), ("points", "velocity"))
    # diffusivity 0 is today's output, whatever the seed and the epoch
    dm = engine.DeviceMesh.from_mesh(mesh)
    f0, f1 = engine.DeviceField.from_snapshot(dm, s0), engine.DeviceField.from_snapshot(dm, s1)
    cfg = engine.TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=0.0,
                                  method=1, layer=LAYER)
    today = engine.run_trajectories(dm, f0, f1, cfg, seeds, depths=depths)
    off = M.MOPS_RunPathLine(_settings(M, depths, KE, LAYER, kh=0.0), seeds)
    _equal(off, today, path_keys)
    assert any(on[i]["points"].tobytes() != off[i]["points"].tobytes() for i in range(R.N_SEEDS))
    # the Error() paths: an empty list
    capfd.readouterr()
    for bad in (-1.0, float("nan"), float("inf")):
        assert M.MOPS_RunPathLine(_settings(M, depths, KE, LAYER, kh=bad), seeds) == []
        assert M.MOPS_RunStreamLine(_settings(M, depths, KE, LAYER, kh=bad), seeds) == []
    out = capfd.readouterr()
    assert "diffusivity" in out.out + out.err
    assert M.MOPS_RunStreamLine(_settings(M, depths, KE, -1), seeds) == []  # a depth-mode streamline
    out = capfd.readouterr()
    assert "fixedLayer" in out.out + out.err
    cfg = _settings(M, depths, KE, -1)
    cfg.sampleAttributes = True
    assert M.MOPS_RunPathLine(cfg, seeds) == []
    out = capfd.readouterr()
    assert "sampleAttributes" in out.out + out.err
