"""MOPS::MOPS_RunLAVD of the C++ API (include/mops/MOPS.h) through tests/cpp/lavd_api.cpp, compiled with g++ against
the engine library: the image is pyMOPS.MOPS_RunLAVD's and the engine-level chain's byte for byte, a PNG written
from C++ decodes to the restated colours, and each refusal gives Error() and an empty image."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import image_reference as IR
import lavd_case as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lavd_api.cpp")
REFUSALS = 8


def _compile(out_dir):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = os.path.join(str(out_dir), "lavd_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    return exe


def test_lavd_cpp_driver_compiles_and_links(engine_lib, tmp_path):
    """MOPS_RunLAVD is declared by the header and resolves in libmops_traj.so (no GPU needed to link)."""
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_lavd_cpp_equals_pymops_and_the_engine(engine_lib, gpu, small_case, tmp_path):
    from mops_amd.engine import DeviceMesh
    from test_lavd_pymops import _pymops
    mesh, s0, s1 = small_case
    exe = _compile(tmp_path)
    d = str(tmp_path)
    W, H = LC.WIDTH, LC.HEIGHT
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{mesh.nCells} {mesh.nVertices} {mesh.maxEdges} {mesh.nVertLevels} {W} {H} {LC.LAT[0]} {LC.LAT[1]} "
                f"{LC.LON[0]} {LC.LON[1]} {LC.DEPTH} {LC.DT} {LC.GAP} {LC.RT}\n")
    arrays = dict(nEdgesOnCell=mesh.nEdgesOnCell, verticesOnCell=mesh.verticesOnCell, cellsOnCell=mesh.cellsOnCell,
                  cellsOnVertex=mesh.cellsOnVertex, cellCoord=mesh.cellCoord, vertexCoord=mesh.vertexCoord)
    for t, s in enumerate((s0, s1)):
        arrays.update({f"layerThickness_{t}": s.layerThickness, f"bottomDepth_{t}": s.bottomDepth,
                       f"zonal_{t}": s.zonalVelocity, f"meridional_{t}": s.meridionalVelocity,
                       f"vvel_{t}": s.vertVelocityTop})
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        (a.astype(np.uint64) if a.dtype.kind in "iu" else a.astype(np.float64)).tofile(os.path.join(d, k))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stderr.count("[Error]") == REFUSALS and r.stderr.count("LAVD") >= REFUSALS
    assert open(os.path.join(d, "summary.txt")).read().split() == ["0"] * REFUSALS
    got = np.fromfile(os.path.join(d, "lavd.f64")).reshape(H, W, 4)
    again = np.fromfile(os.path.join(d, "lavd_again.f64")).reshape(H, W, 4)
    assert LC.same(got, again)
    want = LC.engine_image(DeviceMesh.from_mesh(mesh), [s0, s1])
    assert LC.same(got, want)
    M = _pymops(mesh, [s0, s1])
    M.MOPS_ActiveAttribute(0, 1)
    cfg = M.VisualizationSettings()
    cfg.imageSize, cfg.LatRange, cfg.LonRange, cfg.FixedDepth = (W, H), LC.LAT, LC.LON, LC.DEPTH
    traj = M.TrajectorySettings()
    traj.deltaT, traj.simulationDuration, traj.recordT = LC.DT, LC.GAP, LC.RT
    assert LC.same(got, M.MOPS_RunLAVD(cfg, traj))
    fin = np.isfinite(got[:, :, 0])
    assert 4 * fin.sum() >= fin.size and (~fin).any()
    rgba = IR.decode_png(os.path.join(d, "lavd.png"))
    assert np.array_equal(rgba, IR.save_to_png_rgba(got[:, :, 0])[0])
    assert not rgba[~fin].any() and (rgba[fin][:, 3] == 255).all()
