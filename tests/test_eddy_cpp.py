"""MOPS::MOPS_RunEddyMap of the C++ API (include/mops/MOPS.h) through tests/cpp/eddy_api.cpp, compiled with g++
against the engine library: its image is the restatement's (tests/eddy_case.py) and the Python path's bytes."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eddy_case as EC  # noqa: E402
import image_reference as IR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "eddy_api.cpp")


def _compile(out_dir):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = os.path.join(str(out_dir), "eddy_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    return exe


def test_eddy_cpp_driver_compiles_and_links(engine_lib, tmp_path):
    """MOPS_RunEddyMap is declared by the header and resolves in libmops_traj.so (no GPU needed to link)."""
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_eddy_cpp_equals_the_restatement(engine_lib, oracle_lib, gpu, small_case, tmp_path):
    from mops_amd import pyMOPS as M
    mesh, s0, _ = small_case
    exe = _compile(tmp_path)
    d = str(tmp_path)
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{mesh.nCells} {mesh.nVertices} {mesh.maxEdges} {mesh.nVertLevels} {EC.WIDTH} {EC.HEIGHT} "
                f"{EC.LAT[0]} {EC.LAT[1]} {EC.LON[0]} {EC.LON[1]} {EC.DEPTH}\n")
    arrays = dict(nEdgesOnCell=mesh.nEdgesOnCell, verticesOnCell=mesh.verticesOnCell, cellsOnCell=mesh.cellsOnCell,
                  cellsOnVertex=mesh.cellsOnVertex, cellCoord=mesh.cellCoord, vertexCoord=mesh.vertexCoord,
                  layerThickness=s0.layerThickness, bottomDepth=s0.bottomDepth, zonal=s0.zonalVelocity,
                  meridional=s0.meridionalVelocity, vvel=s0.vertVelocityTop)
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        (a.astype(np.uint64) if a.dtype.kind in "iu" else a.astype(np.float64)).tofile(os.path.join(d, k))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for rule in EC.RULES:
        want = EC.depth_image(oracle_lib, small_case, rule)["images"][1]
        got = np.fromfile(os.path.join(d, f"eddy_{rule}.f64"), dtype=np.float64).reshape(EC.HEIGHT, EC.WIDTH, 4)
        assert np.array_equal(got, want, equal_nan=True), rule
    ref = np.fromfile(os.path.join(d, "eddy_reference.f64"), dtype=np.float64)
    assert np.fromfile(os.path.join(d, "eddy_again.f64"), dtype=np.float64).tobytes() == ref.tobytes()
    assert open(os.path.join(d, "summary.txt")).read().split() == ["1", "0", "0"]
    img = ref.reshape(EC.HEIGHT, EC.WIDTH, 4)
    for ch in range(2):
        name = os.path.join(d, f"py_ch{ch}.png")
        assert M.SaveToPNG(img, name, ch)
        assert np.array_equal(IR.decode_png(os.path.join(d, f"eddy_ch{ch}.png")), IR.decode_png(name))
