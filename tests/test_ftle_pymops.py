"""GPU: pyMOPS.MOPS_LatticeSeeds / MOPS_RunFTLE against the numpy restatement (tests/ftle_reference.py): the lattice
bytes, channels 1 and 2 and the NaN pattern byte for byte, channel 0 within the allowance of
tests/test_ftle_gpu.py, the image through SaveToPNG / SaveVTI unchanged, and the Error() convention."""
import os

import numpy as np
import pytest

import ftle_reference as F
import image_reference as IR
from test_ftle_gpu import LOG_ULPS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pathlines(gpu, engine_lib, small_case):
    return F.e2e_lines(small_case)


def _settings(M, **w):
    cfg = M.VisualizationSettings()
    cfg.imageSize, cfg.LatRange, cfg.LonRange = (w["width"], w["height"]), w["lat_range"], w["lon_range"]
    return cfg


def test_lattice_seeds(gpu, engine_lib):
    from mops_amd import pyMOPS as M
    for w in (F.E2E, F.DEAD_5x7):
        got = M.MOPS_LatticeSeeds(_settings(M, **w))
        assert got.shape == (w["width"] * w["height"], 3) and got.tobytes() == F.lattice(**w).tobytes()
    assert M.MOPS_LatticeSeeds(None).shape == (0, 3)
    bad = _settings(M, **dict(F.E2E, width=0))
    assert M.MOPS_LatticeSeeds(bad).shape == (0, 3)


def test_run_ftle(pathlines, tmp_path, monkeypatch):
    from mops_amd import pyMOPS as M
    lines, horizon = pathlines
    cfg = _settings(M, **F.E2E)
    assert np.stack([ln["points"][0] for ln in lines]).tobytes() == M.MOPS_LatticeSeeds(cfg).tobytes()
    dead = np.array([not np.any(ln["lastPoint"]) for ln in lines])
    assert dead.any()  # land: a dead line has a zero lastPoint, and no death array is passed
    got = M.MOPS_RunFTLE(lines, cfg, horizon)
    want = F.lines_image(lines, horizon, **F.E2E)
    H, W = F.E2E["height"], F.E2E["width"]
    assert got.shape == (H, W, 4)
    for ch in (1, 2, 3):
        assert got[:, :, ch].tobytes() == want[:, :, ch].tobytes(), ch
    valid = ~np.isnan(want[:, :, 1])
    assert np.array_equal(~np.isnan(got[:, :, 0]), valid) and 2 * valid.sum() >= W * H and (~valid).any()
    assert np.isnan(got.reshape(-1, 4)[dead, 1]).all()
    assert F.ulp_distance(got[:, :, 0], np.log(got[:, :, 1]) / (2.0 * horizon)) <= LOG_ULPS
    # usable with SaveToPNG and SaveVTI unchanged
    png = str(tmp_path / "ftle.png")
    assert M.SaveToPNG(got, png, 0)
    rgba = IR.decode_png(png)
    assert np.array_equal(rgba, IR.save_to_png_rgba(got[:, :, 0])[0])
    assert not rgba[~valid].any() and (rgba[valid][:, 3] == 255).all()
    monkeypatch.chdir(tmp_path)
    assert os.path.getsize(M.SaveVTI(got, cfg, outputName="ftle")) > 0
    # bad input: Error() and an empty image
    assert M.MOPS_RunFTLE(lines, None, horizon).size == 0
    assert M.MOPS_RunFTLE(lines[:-1], cfg, horizon).size == 0
    assert M.MOPS_RunFTLE(None, cfg, horizon).size == 0
    for h in (0.0, -1.0, float("nan"), float("inf"), None):
        assert M.MOPS_RunFTLE(lines, cfg, h).size == 0, h
    without = [{k: v for k, v in ln.items() if k != "lastPoint"} for ln in lines]
    assert M.MOPS_RunFTLE(without, cfg, horizon).size == 0
