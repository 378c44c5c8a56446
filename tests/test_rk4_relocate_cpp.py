"""MOPS::TrajectorySettings::relocateStages of the C++ API (include/mops/MOPS.h) through
tests/cpp/rk4_relocate_api.cpp, compiled with g++ against the engine library: with kRK4 the lines are the
restatement's (tests/rk4_relocate_reference.py); off they are today's bytes; with kEuler the flag has no effect; a
streamline with it and kRK4 returns no lines."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pathline_attr_reference as R
import rk4_relocate_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rk4_relocate_api.cpp")


def _compile(out_dir):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = os.path.join(str(out_dir), "rk4_relocate_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    return exe


def test_relocate_cpp_driver_compiles_and_links(engine_lib, tmp_path):
    """TrajectorySettings::relocateStages is declared by the header (no GPU needed to link)."""
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_relocate_cpp_equals_the_restatement(engine_lib, oracle_lib, gpu, small_case, tmp_path):
    from mops_amd import engine
    mesh, s0, s1 = small_case
    seeds, depths = R.shared_seeds()
    K = R.DURATION // R.RECORD_T
    exe = _compile(tmp_path)
    d = str(tmp_path)
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{mesh.nCells} {mesh.nVertices} {mesh.maxEdges} {mesh.nVertLevels} {len(seeds)} {R.DELTA_T} "
                f"{R.DURATION} {R.RECORD_T}\n")
    arrays = dict(nEdgesOnCell=mesh.nEdgesOnCell, verticesOnCell=mesh.verticesOnCell, cellsOnCell=mesh.cellsOnCell,
                  cellsOnVertex=mesh.cellsOnVertex, cellCoord=mesh.cellCoord, vertexCoord=mesh.vertexCoord, seeds=seeds)
    for t, s in enumerate((s0, s1)):
        arrays.update({f"layerThickness_{t}": s.layerThickness, f"bottomDepth_{t}": s.bottomDepth,
                       f"zonal_{t}": s.zonalVelocity, f"meridional_{t}": s.meridionalVelocity,
                       f"vvel_{t}": s.vertVelocityTop})
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        (a.astype(np.uint64) if a.dtype.kind in "iu" else a.astype(np.float64)).tofile(os.path.join(d, k))
    depths.astype(np.float32).tofile(os.path.join(d, "depths"))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "relocateStages" in r.stdout + r.stderr  # the refusals' Error()

    def got(name):
        return np.fromfile(os.path.join(d, name), dtype=np.float64)
    r0, r1 = oracle_lib.preprocess(mesh, s0), oracle_lib.preprocess(mesh, s1)
    want = RR.lines(oracle_lib, RR.run_shared(oracle_lib, mesh, r0, r1, relocate=True))
    assert want["points"].shape == (len(seeds), K + 1, 3)
    assert got("points_rk4_on.f64").tobytes() == want["points"].tobytes()
    assert got("velocity_rk4_on.f64").tobytes() == want["velocity"].tobytes()
    assert got("last_rk4_on.f64").tobytes() == want["lastPoint"].tobytes()
    # flag off: the engine's plain RK4 / Euler (today's output); Euler with the flag: the same bytes
    dm = engine.DeviceMesh.from_mesh(mesh)
    f0, f1 = engine.DeviceField.from_snapshot(dm, s0), engine.DeviceField.from_snapshot(dm, s1)
    for tag, method in (("rk4_off", 0), ("euler_off", 1), ("euler_on", 1)):
        cfg = engine.TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=0.0,
                                      method=method)
        today = engine.run_trajectories(dm, f0, f1, cfg, seeds, depths=depths)
        assert got(f"points_{tag}.f64").tobytes() == today["points"].tobytes(), tag
        assert got(f"velocity_{tag}.f64").tobytes() == today["velocity"].tobytes(), tag
        assert got(f"last_{tag}.f64").tobytes() == today["lastPoint"].tobytes(), tag
    assert got("points_rk4_on.f64").tobytes() != got("points_rk4_off.f64").tobytes()
    counts = [int(x) for x in open(os.path.join(d, "streamline.txt")).read().split()]
    assert counts == [len(seeds), len(seeds), 0, 0]
