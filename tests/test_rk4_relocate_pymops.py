"""GPU: pyMOPS.TrajectorySettings.relocateStages -- with kRK4, MOPS_RunPathLine runs the RK4 that locates each stage
in its own cell (tests/rk4_relocate_reference.py is the reference); off, the output is today's; with kEuler it has
no effect; MOPS_RunStreamLine with it and kRK4 reports an error and returns an empty list."""
import numpy as np
import pytest

import pathline_attr_reference as R
import rk4_relocate_reference as RR
from test_attr_pymops import _setup

pytestmark = pytest.mark.gpu

LINE_KEYS = ("points", "velocity", "temperature", "salinity", "lastPoint")


def _settings(M, ref, method, relocate):
    cfg = M.TrajectorySettings()
    assert cfg.relocateStages is False
    cfg.deltaT, cfg.simulationDuration, cfg.recordT, cfg.depth = R.DELTA_T, R.DURATION, R.RECORD_T, 0.0
    cfg.methodType = method
    cfg.particle_depths = list(ref["depths"])
    cfg.relocateStages = relocate
    return cfg


def _same(a, b):
    return len(a) == len(b) and all(a[i][k].tobytes() == b[i][k].tobytes() for i in range(len(a)) for k in LINE_KEYS)


def test_pymops_relocate_stages(engine_lib, oracle_lib, gpu, small_case, capfd):
    from mops_amd import engine
    mesh, s0, s1 = small_case
    r0, r1 = oracle_lib.preprocess(mesh, s0), oracle_lib.preprocess(mesh, s1)
    rel = RR.run_shared(oracle_lib, mesh, r0, r1, relocate=True)
    plain = RR.run_shared(oracle_lib, mesh, r0, r1, relocate=False)
    M = _setup(mesh, (s0, s1), ((), ()))
    K4, KE = M.CalcMethodType.kRK4, M.CalcMethodType.kEuler
    seeds = rel["seeds"]
    on = M.MOPS_RunPathLine(_settings(M, rel, K4, True), seeds)
    off = M.MOPS_RunPathLine(_settings(M, rel, K4, False), seeds)
    for got, ref in ((on, rel), (off, plain)):
        want = RR.lines(oracle_lib, ref)
        assert len(got) == R.N_SEEDS
        for i in range(R.N_SEEDS):
            for k in LINE_KEYS:
                assert got[i][k].tobytes() == want[k][i].tobytes(), (i, k)
    assert not _same(on, off)
    # flag off: byte-equal to the engine's plain RK4 (today's output)
    dm = engine.DeviceMesh.from_mesh(mesh)
    f0, f1 = engine.DeviceField.from_snapshot(dm, s0), engine.DeviceField.from_snapshot(dm, s1)
    cfg = engine.TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=0.0, method=0)
    today = engine.run_trajectories(dm, f0, f1, cfg, seeds, depths=rel["depths"])
    for i in range(R.N_SEEDS):
        for k in LINE_KEYS:
            assert off[i][k].tobytes() == today[k][i].tobytes(), (i, k)
    # Euler has no stages: the flag changes nothing
    assert _same(M.MOPS_RunPathLine(_settings(M, rel, KE, True), seeds),
                 M.MOPS_RunPathLine(_settings(M, rel, KE, False), seeds))
    # streamlines: Euler ignores it, kRK4 follows the reference's error convention
    assert len(M.MOPS_RunStreamLine(_settings(M, rel, KE, True), seeds)) == R.N_SEEDS
    assert len(M.MOPS_RunStreamLine(_settings(M, rel, K4, False), seeds)) == R.N_SEEDS
    capfd.readouterr()
    assert M.MOPS_RunStreamLine(_settings(M, rel, K4, True), seeds) == []
    out = capfd.readouterr()
    assert "relocateStages" in out.out + out.err
    # ... and so does the pathline with attribute sampling
    cfg = _settings(M, rel, K4, True)
    cfg.sampleAttributes = True
    assert M.MOPS_RunPathLine(cfg, seeds) == []
