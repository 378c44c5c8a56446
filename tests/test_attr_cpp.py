"""MOPS::TrajectorySettings::sampleAttributes of the C++ API (include/mops/MOPS.h) through
tests/cpp/pathline_attrs_api.cpp, compiled with g++ against the engine library: the lines' temperature / salinity
are the Python path's bytes (engine.run_trajectories with ``attrs``)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pathline_attr_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pathline_attrs_api.cpp")


def _compile(out_dir):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = os.path.join(str(out_dir), "pathline_attrs_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    return exe


def test_attr_cpp_driver_compiles_and_links(engine_lib, tmp_path):
    """TrajectorySettings::sampleAttributes is declared by the header and MOPS_RunPathLine resolves in
    libmops_traj.so (no GPU needed to link)."""
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_attr_cpp_equals_the_python_path(engine_lib, gpu, small_case, tmp_path):
    from mops_amd import engine
    mesh, s0, s1 = small_case
    seeds, depths = R.shared_seeds()
    K = R.DURATION // R.RECORD_T
    exe = _compile(tmp_path)
    d = str(tmp_path)
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{mesh.nCells} {mesh.nVertices} {mesh.maxEdges} {mesh.nVertLevels} {len(seeds)} {R.DELTA_T} "
                f"{R.DURATION} {R.RECORD_T} 1\n")
    arrays = dict(nEdgesOnCell=mesh.nEdgesOnCell, verticesOnCell=mesh.verticesOnCell, cellsOnCell=mesh.cellsOnCell,
                  cellsOnVertex=mesh.cellsOnVertex, cellCoord=mesh.cellCoord, vertexCoord=mesh.vertexCoord, seeds=seeds)
    for t, s in enumerate((s0, s1)):
        arrays.update({f"layerThickness_{t}": s.layerThickness, f"bottomDepth_{t}": s.bottomDepth,
                       f"zonal_{t}": s.zonalVelocity, f"meridional_{t}": s.meridionalVelocity,
                       f"vvel_{t}": s.vertVelocityTop, f"temperature_{t}": s.attributes["temperature"],
                       f"salinity_{t}": s.attributes["salinity"]})
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        (a.astype(np.uint64) if a.dtype.kind in "iu" else a.astype(np.float64)).tofile(os.path.join(d, k))
    depths.astype(np.float32).tofile(os.path.join(d, "depths"))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    dm = engine.DeviceMesh.from_mesh(mesh)
    f0, f1 = engine.DeviceField.from_snapshot(dm, s0), engine.DeviceField.from_snapshot(dm, s1)
    attrs = {k: (engine.cell_to_vertex_attr(dm, s0.attributes[k]), engine.cell_to_vertex_attr(dm, s1.attributes[k]))
             for k in ("salinity", "temperature")}
    cfg = engine.TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=0.0,
                                  method=0)
    on = engine.run_trajectories(dm, f0, f1, cfg, seeds, depths=depths, attrs=attrs)
    off = engine.run_trajectories(dm, f0, f1, cfg, seeds, depths=depths)

    def got(name):
        return np.fromfile(os.path.join(d, name), dtype=np.float64)
    for tag, want in (("on", on), ("off", off)):
        for k in ("temperature", "salinity", "points"):
            assert got(f"{k}_{tag}.f64").tobytes() == want[k].tobytes(), (k, tag)
    assert on["temperature"].shape == (len(seeds), K + 1)
    assert not np.array_equal(on["temperature"], off["temperature"]) and on["temperature"].any()
