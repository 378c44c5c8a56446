"""MOPS::MOPS_RunRemapping of the C++ API (include/mops/MOPS.h) through tests/cpp/remap_api.cpp, compiled with
g++ against the engine library: its images are the Python path's bytes (engine.remap_fixed_depth)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "remap_api.cpp")


def _compile(out_dir):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = os.path.join(str(out_dir), "remap_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    return exe


def test_remap_cpp_driver_compiles_and_links(engine_lib, tmp_path):
    """ImageBuffer, VisualizationSettings and MOPS_RunRemapping are declared by the header and resolve in
    libmops_traj.so (no GPU needed to link)."""
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_remap_cpp_equals_the_python_path(engine_lib, gpu, small_case, tmp_path):
    from mops_amd import engine
    mesh, s0, _ = small_case
    w, h, lat, lon, depth = 40, 32, (-60.0, 60.0), (-170.0, 150.0), 2500.0
    names = sorted(s0.attributes)[:2]
    exe = _compile(tmp_path)
    d = str(tmp_path)
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{mesh.nCells} {mesh.nVertices} {mesh.maxEdges} {mesh.nVertLevels} {len(names)} {w} {h} "
                f"{lat[0]} {lat[1]} {lon[0]} {lon[1]} {depth}\n")
    arrays = dict(nEdgesOnCell=mesh.nEdgesOnCell, verticesOnCell=mesh.verticesOnCell, cellsOnCell=mesh.cellsOnCell,
                  cellsOnVertex=mesh.cellsOnVertex, cellCoord=mesh.cellCoord, vertexCoord=mesh.vertexCoord,
                  layerThickness=s0.layerThickness, bottomDepth=s0.bottomDepth, zonal=s0.zonalVelocity,
                  meridional=s0.meridionalVelocity, vvel=s0.vertVelocityTop)
    arrays.update({f"attr_{k}": s0.attributes[n] for k, n in enumerate(names)})
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        (a.astype(np.uint64) if a.dtype.kind in "iu" else a.astype(np.float64)).tofile(os.path.join(d, k))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    dm = engine.DeviceMesh.from_mesh(mesh)
    df = engine.DeviceField.from_snapshot(dm, s0)
    va = tuple(engine.cell_to_vertex_attr(dm, s0.attributes[n]) for n in names)
    for rule in ("reference", "bracket"):
        want = engine.remap_fixed_depth(dm, df, w, h, lat, lon, depth, n_attr=len(names), vertex_attrs=va,
                                        layer_rule=rule).cpu().numpy()
        got = np.fromfile(os.path.join(d, f"images_{rule}.f64"), dtype=np.float64)
        assert want.shape == (2, h, w, 4) and got.tobytes() == want.tobytes()
        assert np.isfinite(want[..., :3]).any() and np.isnan(want[..., :3]).any()
    n_images, sw, sh, first_x, alpha = open(os.path.join(d, "summary.txt")).read().split()
    ref0 = np.fromfile(os.path.join(d, "images_reference.f64"), dtype=np.float64).reshape(2, h, w, 4)[0]
    assert (int(n_images), int(sw), int(sh)) == (2, w, h)
    assert float(alpha) == float(w * h)                      # getChannel(3): alpha 1 on every pixel
    assert first_x == "nan" if np.isnan(ref0[0, 0, 0]) else float(first_x) == pytest.approx(ref0[0, 0, 0], abs=1e-6)
