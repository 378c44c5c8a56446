"""MOPS::TrajectorySettings::diffusivity / randomSeed / randomEpoch of the C++ API (include/mops/MOPS.h) through
tests/cpp/diffusion_api.cpp, compiled with g++ against the engine library: with a diffusivity the lines of
MOPS_RunPathLine (in a layer, and at the depths with relocated RK4 stages) and of MOPS_RunStreamLine in a layer are
the restatement's (tests/diffusion_reference.py); with 0 they are today's bytes; a negative or NaN diffusivity, a
depth-mode streamline and sampleAttributes with a diffusivity return no lines."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import diffusion_reference as D
import pathline_attr_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "diffusion_api.cpp")
LAYER, KH, SEED, EPOCH = 4, 2e4, (1 << 40) + 2024, 3


def _compile(out_dir):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = os.path.join(str(out_dir), "diffusion_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    return exe


def test_diffusion_cpp_driver_compiles_and_links(engine_lib, tmp_path):
    """The three members are declared by the header (no GPU needed to link)."""
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_diffusion_cpp_equals_the_restatement(engine_lib, oracle_lib, gpu, small_case, tmp_path):
    from mops_amd import engine
    O = oracle_lib
    mesh, s0, s1 = small_case
    seeds, depths = R.shared_seeds()
    K = R.DURATION // R.RECORD_T
    exe = _compile(tmp_path)
    d = str(tmp_path)
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{mesh.nCells} {mesh.nVertices} {mesh.maxEdges} {mesh.nVertLevels} {len(seeds)} {R.DELTA_T} "
                f"{R.DURATION} {R.RECORD_T} {LAYER} {KH!r} {SEED} {EPOCH}\n")
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
    text = r.stdout + r.stderr
    assert "diffusivity" in text and "fixedLayer" in text and "sampleAttributes" in text  # the Error() texts

    def got(name):
        return np.fromfile(os.path.join(d, name), dtype=np.float64)
    r0, r1 = O.preprocess(mesh, s0), O.preprocess(mesh, s1)
    kw = dict(kh=KH, seed=SEED, epoch=EPOCH)
    for tag, back, run in (("path_layer", r1, dict(layer=LAYER, euler=True)),
                           ("path_depth", r1, dict(layer=None, euler=False, relocate=True)),
                           ("stream_layer", None, dict(layer=LAYER, euler=False))):
        ref = D.run_shared(O, mesh, r0, back, **run, **kw)
        want = D.lines(O, ref, back is not None)
        assert want["points"].shape == (len(seeds), K + 1, 3) and int((ref["death"] < 0).sum()) >= 20
        assert got(f"points_{tag}.f64").tobytes() == want["points"].tobytes(), tag
        assert got(f"velocity_{tag}.f64").tobytes() == want["velocity"].tobytes(), tag
        if back is not None:
            assert got(f"last_{tag}.f64").tobytes() == want["lastPoint"].tobytes(), tag
    # diffusivity 0: the engine's depth-mode Euler (today's output)
    dm = engine.DeviceMesh.from_mesh(mesh)
    f0, f1 = engine.DeviceField.from_snapshot(dm, s0), engine.DeviceField.from_snapshot(dm, s1)
    cfg = engine.TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=0.0, method=1)
    today = engine.run_trajectories(dm, f0, f1, cfg, seeds, depths=depths)
    assert got("points_path_off.f64").tobytes() == today["points"].tobytes()
    assert got("velocity_path_off.f64").tobytes() == today["velocity"].tobytes()
    counts = [int(x) for x in open(os.path.join(d, "errors.txt")).read().split()]
    assert counts == [0, 0, 0, 0]
