"""GPU: MOPS::MOPS_LatticeSeeds / MOPS::MOPS_RunFTLE through a compiled C++ driver (tests/cpp/ftle_api.cpp): the
lattice bytes, the image pyMOPS.MOPS_RunFTLE gives for the same lines byte for byte (channel 0 included: the same
kernel), the restatement's channels 1 and 2, and a PNG written from C++."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ftle_reference as F
import image_reference as IR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pathlines(gpu, engine_lib, small_case):
    return F.e2e_lines(small_case)


def test_cpp_lattice_and_ftle(pathlines, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    from mops_amd import pyMOPS as M
    lines, horizon = pathlines
    src = os.path.join(ROOT, "tests", "cpp", "ftle_api.cpp")
    exe = str(tmp_path / "ftle_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    w = F.E2E
    W, H = w["width"], w["height"]
    d = str(tmp_path)
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{W} {H} {w['lat_range'][0]} {w['lat_range'][1]} {w['lon_range'][0]} {w['lon_range'][1]} "
                f"{horizon!r}\n")
    np.stack([ln["points"][0] for ln in lines]).astype(np.float64).tofile(os.path.join(d, "first"))
    np.stack([ln["lastPoint"] for ln in lines]).astype(np.float64).tofile(os.path.join(d, "last"))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stderr.count("[Error]") == 7
    assert np.fromfile(os.path.join(d, "seeds.f64")).tobytes() == F.lattice(**w).tobytes()
    got = np.fromfile(os.path.join(d, "ftle.f64")).reshape(H, W, 4)
    cfg = M.VisualizationSettings()
    cfg.imageSize, cfg.LatRange, cfg.LonRange = (W, H), w["lat_range"], w["lon_range"]
    assert got.tobytes() == M.MOPS_RunFTLE(lines, cfg, horizon).tobytes()
    want = F.lines_image(lines, horizon, **w)
    for ch in (1, 2, 3):
        assert got[:, :, ch].tobytes() == want[:, :, ch].tobytes(), ch
    valid = ~np.isnan(got[:, :, 0])
    assert np.array_equal(valid, ~np.isnan(want[:, :, 1])) and valid.any() and (~valid).any()
    rgba = IR.decode_png(os.path.join(d, "ftle.png"))
    assert np.array_equal(rgba, IR.save_to_png_rgba(got[:, :, 0])[0])
    assert not rgba[~valid].any() and (rgba[valid][:, 3] == 255).all()
