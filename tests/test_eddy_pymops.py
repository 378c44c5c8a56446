"""pyMOPS.MOPS_RunEddyMap: the vorticity / Okubo-Weiss image of the active front solution is image 1 of the
fixed-depth remapping fed the signed vertex arrays, bit for bit the restatement's (tests/eddy_case.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eddy_case as EC  # noqa: E402
from test_remap_gpu import _pymops  # noqa: E402

pytestmark = pytest.mark.gpu


def test_pymops_eddy_map(engine_lib, oracle_lib, gpu, small_case):
    mesh, s0, _ = small_case
    M = _pymops(mesh, s0, ["salinity", "temperature"])       # the solution's own attributes play no part
    cfg = M.VisualizationSettings()
    cfg.imageSize = (EC.WIDTH, EC.HEIGHT)
    cfg.LatRange, cfg.LonRange, cfg.FixedDepth = EC.LAT, EC.LON, EC.DEPTH
    assert M._app.eddy_attrs == {}
    for rule in EC.RULES:
        cfg.layerRule = rule
        img = M.MOPS_RunEddyMap(cfg)
        want = EC.depth_image(oracle_lib, small_case, rule)["images"][1]
        assert isinstance(img, np.ndarray) and img.shape == (EC.HEIGHT, EC.WIDTH, 4) and img.dtype == np.float64
        assert np.array_equal(img, want, equal_nan=True), rule
        # it overlays the velocity image: NaN on the same pixels
        vel = M.MOPS_RunRemapping(cfg)[0]
        assert np.array_equal(np.isnan(img[..., 0]), np.isnan(vel[..., 0]))
    assert list(M._app.eddy_attrs) == [0]                     # the vertex arrays were made once, for solution 0
    kept = M._app.eddy_attrs[0]
    cfg.layerRule = "reference"
    again = M.MOPS_RunEddyMap(cfg)
    assert M._app.eddy_attrs[0] is kept
    assert np.array_equal(again, EC.depth_image(oracle_lib, small_case, "reference")["images"][1], equal_nan=True)
    cfg.imageSize = (0, EC.HEIGHT)
    assert M.MOPS_RunEddyMap(cfg) == []                       # Error() and an empty list
    assert M.MOPS_RunEddyMap(None) == []
    M.MOPS_Init("gpu")
    assert M._app.eddy_attrs == {}
    cfg.imageSize = (EC.WIDTH, EC.HEIGHT)
    assert M.MOPS_RunEddyMap(cfg) == []                       # no solution
