"""GPU: pyMOPS.TrajectorySettings.fixedLayer -- >= 0 makes MOPS_RunStreamLine / MOPS_RunPathLine advect within that
model layer (tests/layer_reference.py is the reference); -1, the default, is today's output; an out-of-range layer
and sampleAttributes with a layer report an error and return an empty list."""
import numpy as np
import pytest

import layer_reference as LR
import pathline_attr_reference as R
from test_attr_pymops import _setup

pytestmark = pytest.mark.gpu

LAYER = 4


def _settings(M, ref, method, layer, relocate=False):
    cfg = M.TrajectorySettings()
    assert cfg.fixedLayer == -1
    cfg.deltaT, cfg.simulationDuration, cfg.recordT, cfg.depth = R.DELTA_T, R.DURATION, R.RECORD_T, 0.0
    cfg.methodType = method
    cfg.particle_depths = list(ref["depths"])
    cfg.relocateStages = relocate
    cfg.fixedLayer = layer
    return cfg


def _equal(got, want, keys):
    assert len(got) == R.N_SEEDS
    for i in range(R.N_SEEDS):
        for k in keys:
            assert got[i][k].tobytes() == want[k][i].tobytes(), (i, k)


def test_pymops_fixed_layer(engine_lib, oracle_lib, gpu, small_case, capfd):
    from mops_amd import engine
    O = oracle_lib
    mesh, s0, s1 = small_case
    r0, r1 = O.preprocess(mesh, s0), O.preprocess(mesh, s1)
    M = _setup(mesh, (s0, s1), ((), ()))
    K4, KE = M.CalcMethodType.kRK4, M.CalcMethodType.kEuler
    seeds, _ = R.shared_seeds()
    path_keys = ("points", "velocity", "temperature", "salinity", "lastPoint")
    ref = None
    for method, relocate in ((KE, False), (K4, False), (K4, True)):
        kw = dict(euler=method == KE, relocate=relocate)
        ref = LR.run_shared(O, mesh, r0, r1, LAYER, **kw)
        _equal(M.MOPS_RunPathLine(_settings(M, ref, method, LAYER, relocate), seeds), LR.lines(O, ref, True), path_keys)
        ref = LR.run_shared(O, mesh, r0, None, LAYER, **kw)  # relocateStages runs for a streamline with a layer
        _equal(M.MOPS_RunStreamLine(_settings(M, ref, method, LAYER, relocate), seeds), LR.lines(O, ref, False),
               ("points", "velocity"))
    # the default is today's output
    dm = engine.DeviceMesh.from_mesh(mesh)
    f0, f1 = engine.DeviceField.from_snapshot(dm, s0), engine.DeviceField.from_snapshot(dm, s1)
    cfg = engine.TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=0.0, method=1)
    today = engine.run_trajectories(dm, f0, f1, cfg, seeds, depths=ref["depths"])
    off = M.MOPS_RunPathLine(_settings(M, ref, KE, -1), seeds)
    _equal(off, today, path_keys)
    on = M.MOPS_RunPathLine(_settings(M, ref, KE, LAYER), seeds)
    assert any(on[i]["points"].tobytes() != off[i]["points"].tobytes() for i in range(R.N_SEEDS))
    # the Error() paths: an empty list
    capfd.readouterr()
    for bad in (mesh.nVertLevels, mesh.nVertLevels + 5):
        assert M.MOPS_RunPathLine(_settings(M, ref, KE, bad), seeds) == []
        assert M.MOPS_RunStreamLine(_settings(M, ref, KE, bad), seeds) == []
    out = capfd.readouterr()
    assert "fixedLayer" in out.out + out.err
    cfg = _settings(M, ref, KE, LAYER)
    cfg.sampleAttributes = True
    assert M.MOPS_RunPathLine(cfg, seeds) == []
    out = capfd.readouterr()
    assert "sampleAttributes" in out.out + out.err
    # the depth-mode refusal of relocateStages for streamlines is unchanged
    assert M.MOPS_RunStreamLine(_settings(M, ref, K4, -1, True), seeds) == []
