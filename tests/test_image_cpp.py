"""MOPS::SaveToPNG, MOPS::VTKFileManager::SaveVTI (both overloads) and MOPS::MPASOVisualizer::VisualizeFixedLayer
of the C++ API (include/mops/MOPS.h) through tests/cpp/image_api.cpp, compiled with g++ against the engine
library: the decoded contents of its files are those of the files the Python path writes."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_reference as IR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "image_api.cpp")


def _compile(out_dir):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = os.path.join(str(out_dir), "image_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    return exe


def test_image_cpp_driver_compiles_and_links(engine_lib, tmp_path):
    """SaveToPNG, VTKFileManager and MPASOVisualizer are declared by the header and resolve in libmops_traj.so."""
    assert os.path.exists(_compile(tmp_path))


def _same_vti(a, b):
    va, vb = IR.read_vti(a), IR.read_vti(b)
    assert (va["extent"], va["origin"], va["spacing"], va["scalars"]) == (vb["extent"], vb["origin"], vb["spacing"],
                                                                          vb["scalars"])
    assert [(n, c) for n, c, _ in va["arrays"]] == [(n, c) for n, c, _ in vb["arrays"]]
    for (_, _, x), (_, _, y) in zip(va["arrays"], vb["arrays"]):
        assert np.array_equal(x, y, equal_nan=True)
    return va


@pytest.mark.gpu
def test_image_cpp_files_equal_the_python_path(engine_lib, gpu, small_case, tmp_path, monkeypatch):
    from mops_amd import engine, pyMOPS as M
    mesh, s0, _ = small_case
    w, h, lat, lon, depth, layer = 37, 23, (-75.0, 80.0), (-180.0, 175.0), 300.0, 3.7
    names = sorted(s0.attributes)[:2]
    exe = _compile(tmp_path)
    d = str(tmp_path)
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{mesh.nCells} {mesh.nVertices} {mesh.maxEdges} {mesh.nVertLevels} {len(names)} {w} {h} "
                f"{lat[0]} {lat[1]} {lon[0]} {lon[1]} {depth} {layer}\n")
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
    assert open(os.path.join(d, "summary.txt")).read().split() == ["2", "0"] and not os.path.exists(d + "/cpp_bad.png")

    # the same through Python, into py/
    dm = engine.DeviceMesh.from_mesh(mesh)
    df = engine.DeviceField.from_snapshot(dm, s0)
    va = tuple(engine.cell_to_vertex_attr(dm, s0.attributes[n]) for n in names)
    images = engine.remap_fixed_depth(dm, df, w, h, lat, lon, depth, n_attr=2, vertex_attrs=va)
    host = images.cpu().numpy()
    assert np.isfinite(host[0, ..., 0]).mean() > 0.4 and np.isnan(host[0, ..., 0]).mean() > 0.05
    os.mkdir(os.path.join(d, "py"))
    monkeypatch.chdir(os.path.join(d, "py"))
    for i in range(2):
        for ch in range(3):
            assert M.SaveToPNG(images[i], f"py_{i}_ch{ch}.png", ch)
            got = IR.decode_png(os.path.join(d, f"cpp_{i}_ch{ch}.png"))
            assert np.array_equal(got, IR.decode_png(f"py_{i}_ch{ch}.png"))
            assert np.array_equal(got, IR.save_to_png_rgba(host[i, ..., ch])[0])
    assert M.SaveToPNG(host[0], "py_alpha.png")
    assert np.array_equal(IR.decode_png(os.path.join(d, "cpp_alpha.png")), IR.decode_png("py_alpha.png"))
    cfg = M.VisualizationSettings()
    cfg.imageSize = (w, h)
    cfg.LatRange, cfg.LonRange = lat, lon
    cfg.FixedDepth = depth
    multi = M.SaveVTI([host[0], host[1]], cfg, ["E: Zonal Velocity", "N: Meridional Velocity"], "cpp")
    assert multi == "cpp_fixed_depth_300.000000.vti"
    v = _same_vti(os.path.join(d, multi), multi)
    assert len(v["arrays"]) == 6 and v["arrays"][2][0] == "attr_2"
    assert np.array_equal(v["arrays"][0][2], host[0, ::-1, :, 0], equal_nan=True)
    single = M.SaveVTI(host[0], cfg, outputName="cpp1")
    v = _same_vti(os.path.join(d, single), single)
    assert v["spacing"][2] == depth and np.array_equal(v["arrays"][0][2], host[0, ::-1, :, :3], equal_nan=True)
    # fixed layer: 3.7 -> layer 3
    want = engine.remap_fixed_layer(dm, df, w, h, lat, lon, layer).cpu().numpy()
    got = np.fromfile(os.path.join(d, "fixed_layer.f64"), dtype=np.float64).reshape(h, w, 4)
    assert got.tobytes() == want.tobytes() and np.isfinite(got[..., 0]).any() and np.isnan(got[..., 0]).any()
    assert np.array_equal(want, engine.remap_fixed_layer(dm, df, w, h, lat, lon, 3).cpu().numpy(), equal_nan=True)
    cfg.VisType = M.VisualizeType.kFixedLayer
    cfg.FixedLayer = layer
    lname = M.SaveVTI(want, cfg, outputName="cpp")
    assert lname == "cpp_fixed_layer_3.700000.vti"
    _same_vti(os.path.join(d, lname), lname)
