"""MOPS::TrajectorySettings::fixedLayer of the C++ API (include/mops/MOPS.h) through tests/cpp/layer_api.cpp, compiled
with g++ against the engine library: with a layer the lines of MOPS_RunStreamLine / MOPS_RunPathLine are the
restatement's (tests/layer_reference.py) for kEuler, kRK4 and kRK4 with relocateStages; with -1 they are today's
bytes; a layer out of range and sampleAttributes with a layer return no lines."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import layer_reference as LR
import pathline_attr_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "layer_api.cpp")
LAYER = 4


def _compile(out_dir):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = os.path.join(str(out_dir), "layer_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    return exe


def test_layer_cpp_driver_compiles_and_links(engine_lib, tmp_path):
    """TrajectorySettings::fixedLayer is declared by the header (no GPU needed to link)."""
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_layer_cpp_equals_the_restatement(engine_lib, oracle_lib, gpu, small_case, tmp_path):
    from mops_amd import engine
    O = oracle_lib
    mesh, s0, s1 = small_case
    seeds, depths = R.shared_seeds()
    K = R.DURATION // R.RECORD_T
    exe = _compile(tmp_path)
    d = str(tmp_path)
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{mesh.nCells} {mesh.nVertices} {mesh.maxEdges} {mesh.nVertLevels} {len(seeds)} {R.DELTA_T} "
                f"{R.DURATION} {R.RECORD_T} {LAYER}\n")
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
    assert "fixedLayer" in r.stdout + r.stderr and "sampleAttributes" in r.stdout + r.stderr  # the Error() texts

    def got(name):
        return np.fromfile(os.path.join(d, name), dtype=np.float64)
    r0, r1 = O.preprocess(mesh, s0), O.preprocess(mesh, s1)
    for kind, back in (("path", r1), ("stream", None)):
        for tag, kw in (("euler", dict(euler=True)), ("rk4", dict(euler=False)),
                        ("reloc", dict(euler=False, relocate=True))):
            want = LR.lines(O, LR.run_shared(O, mesh, r0, back, LAYER, **kw), back is not None)
            assert want["points"].shape == (len(seeds), K + 1, 3)
            assert got(f"points_{kind}_{tag}.f64").tobytes() == want["points"].tobytes(), (kind, tag)
            assert got(f"velocity_{kind}_{tag}.f64").tobytes() == want["velocity"].tobytes(), (kind, tag)
            if back is not None:
                assert got(f"last_{kind}_{tag}.f64").tobytes() == want["lastPoint"].tobytes(), (kind, tag)
    # fixedLayer -1: the engine's depth-mode Euler (today's output)
    dm = engine.DeviceMesh.from_mesh(mesh)
    f0, f1 = engine.DeviceField.from_snapshot(dm, s0), engine.DeviceField.from_snapshot(dm, s1)
    cfg = engine.TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=0.0, method=1)
    today = engine.run_trajectories(dm, f0, f1, cfg, seeds, depths=depths)
    assert got("points_path_off.f64").tobytes() == today["points"].tobytes()
    assert got("velocity_path_off.f64").tobytes() == today["velocity"].tobytes()
    assert got("points_path_off.f64").tobytes() != got("points_path_euler.f64").tobytes()
    counts = [int(x) for x in open(os.path.join(d, "errors.txt")).read().split()]
    assert counts == [0, 0, 0]
