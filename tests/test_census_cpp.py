"""MOPS::MOPS_RunEddyCensus of the C++ API (include/mops/MOPS.h) through tests/cpp/census_api.cpp, compiled with
g++ against the engine library: its table, labels and image are the engine's (engine.eddy_census handed the
threshold the C++ side formed), which tests/test_census_gpu.py holds against the restatement."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_case as CC  # noqa: E402
import eddy_case as EC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "census_api.cpp")
K_SIGMA, MIN_CELLS, FIXED_LAYER = 0.05, 4, 0.5       # FixedLayer 0.5 truncates to layer 0


def _compile(out_dir):
    assert shutil.which("g++") is not None, "the C++ front end's test needs g++ on the PATH"
    exe = os.path.join(str(out_dir), "census_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    return exe


def test_census_cpp_driver_compiles_and_links(engine_lib, tmp_path):
    """MOPS_RunEddyCensus and its settings are declared by the header and resolve in libmops_traj.so (no GPU needed
    to link)."""
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_census_cpp_equals_the_engine(engine_lib, oracle_lib, gpu, small_case, tmp_path):
    from mops_amd import engine
    mesh, s0, _ = small_case
    exe = _compile(tmp_path)
    d = str(tmp_path)
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{mesh.nCells} {mesh.nVertices} {mesh.maxEdges} {mesh.nVertLevels} {EC.WIDTH} {EC.HEIGHT} "
                f"{EC.LAT[0]} {EC.LAT[1]} {EC.LON[0]} {EC.LON[1]} {FIXED_LAYER} {K_SIGMA} {MIN_CELLS}\n")
    arrays = dict(nEdgesOnCell=mesh.nEdgesOnCell, verticesOnCell=mesh.verticesOnCell, cellsOnCell=mesh.cellsOnCell,
                  cellsOnVertex=mesh.cellsOnVertex, cellCoord=mesh.cellCoord, vertexCoord=mesh.vertexCoord,
                  layerThickness=s0.layerThickness, bottomDepth=s0.bottomDepth, zonal=s0.zonalVelocity,
                  meridional=s0.meridionalVelocity, vvel=s0.vertVelocityTop)
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        (a.astype(np.uint64) if a.dtype.kind in "iu" else a.astype(np.float64)).tofile(os.path.join(d, k))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    thr = float(np.fromfile(os.path.join(d, "threshold.f64"), dtype=np.float64)[0])
    want_thr = CC.small(oracle_lib, small_case)["thresholds"][K_SIGMA]
    assert abs(thr - want_thr) <= 1e-12 * abs(want_thr)
    dm = engine.DeviceMesh.from_mesh(mesh)
    cen = engine.eddy_census(dm, engine.DeviceField.from_snapshot(dm, s0), layer=0, threshold=thr, min_cells=MIN_CELLS)
    ref = CC.census(oracle_lib, small_case, K_SIGMA, MIN_CELLS, threshold=thr)
    E = ref["E"]
    assert E >= 2 and cen.n_eddies == E
    assert open(os.path.join(d, "summary.txt")).read().split() == [str(E), "1", "1", "1", "1"]
    labels = np.fromfile(os.path.join(d, "census_labels.i32"), dtype=np.int32)
    assert labels.tobytes() == cen.labels.cpu().numpy().tobytes() == ref["labels"].tobytes()
    ti = np.fromfile(os.path.join(d, "census_table.i32"), dtype=np.int32).reshape(E, 5)
    td = np.fromfile(os.path.join(d, "census_table.f64"), dtype=np.float64).reshape(E, 9)
    t = cen.table
    assert np.array_equal(ti[:, 0], np.arange(E))
    for j, k in enumerate(("polarity", "n_cells", "root", "core_cell")):
        assert np.array_equal(ti[:, 1 + j], t[k]), k
    for j, k in ((3, "area"), (4, "circulation"), (5, "ow_min")):       # the kernel's columns: the same bytes
        assert td[:, j].tobytes() == t[k].tobytes() == ref["table"][k].tobytes(), k
    assert np.ascontiguousarray(td[:, 6:9]).tobytes() == t["centre"].tobytes()
    # lat, lon and radius are formed by the C++ library's own libm: to rounding of the host functions
    for j, k in ((0, "lat"), (1, "lon"), (2, "radius")):
        assert np.allclose(td[:, j], t[k], rtol=1e-14, atol=1e-12), k
    image = np.fromfile(os.path.join(d, "census_image.f64"), dtype=np.float64).reshape(EC.HEIGHT, EC.WIDTH, 4)
    assert image.tobytes() == cen.image(EC.WIDTH, EC.HEIGHT, EC.LAT, EC.LON).cpu().numpy().tobytes()
