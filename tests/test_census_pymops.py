"""pyMOPS.MOPS_RunEddyCensus: the eddies and the label image of the active front solution are the engine's
(engine.eddy_census at the clamped FixedLayer, the settings' EddyThreshold and EddyMinCells), which
tests/test_census_gpu.py holds against the restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_case as CC  # noqa: E402
import eddy_case as EC  # noqa: E402
from test_remap_gpu import _pymops  # noqa: E402

pytestmark = pytest.mark.gpu


def test_pymops_eddy_census(engine_lib, oracle_lib, gpu, small_case):
    from mops_amd import engine
    mesh, s0, _ = small_case
    M = _pymops(mesh, s0, ["salinity", "temperature"])
    cfg = M.VisualizationSettings()
    assert cfg.EddyThreshold == 0.2 and cfg.EddyMinCells == 4
    cfg.imageSize = (EC.WIDTH, EC.HEIGHT)
    cfg.LatRange, cfg.LonRange = EC.LAT, EC.LON
    for k_sigma, min_cells, fixed_layer, layer in ((0.2, 4, 0.0, 0), (0.05, 1, 0.9, 0), (0.2, 1, 3.7, 3),
                                                   (0.2, 4, 99.0, mesh.nVertLevels - 1), (0.2, 4, -2.0, 0)):
        cfg.EddyThreshold, cfg.EddyMinCells, cfg.FixedLayer = k_sigma, min_cells, fixed_layer
        eddies, image = M.MOPS_RunEddyCensus(cfg)
        cen = engine.eddy_census(M._app.mesh, M._app.front, layer=layer, k_sigma=k_sigma, min_cells=min_cells)
        assert isinstance(eddies, list) and len(eddies) == cen.n_eddies
        assert isinstance(image, np.ndarray) and image.shape == (EC.HEIGHT, EC.WIDTH, 4) and image.dtype == np.float64
        assert image.tobytes() == cen.image(EC.WIDTH, EC.HEIGHT, EC.LAT, EC.LON).cpu().numpy().tobytes()
        for e, row in enumerate(eddies):
            assert tuple(row) == M.EDDY_KEYS and row["index"] == e
            for k in ("lat", "lon", "radius", "area", "circulation", "ow_min"):
                assert np.float64(row[k]).tobytes() == cen.table[k][e].tobytes(), (k, e)
            for k in ("polarity", "n_cells", "root", "core_cell"):
                assert row[k] == int(cen.table[k][e]), (k, e)
            assert row["centre"] == tuple(cen.table["centre"][e])
        if layer == 0:      # against the restatement, at the threshold the engine used
            ref = CC.census(oracle_lib, small_case, k_sigma, min_cells, threshold=cen.threshold)
            assert len(eddies) == ref["E"] > 0
            for k in ref["table"]:
                assert cen.table[k].tobytes() == ref["table"][k].tobytes(), k
            # it overlays the fixed-layer image: NaN wherever that image is NaN
            vel = M.MOPS_RunRemappingFixedLayer(cfg)
            assert np.all(np.isnan(image[..., 0])[np.isnan(vel[..., 0])])
            assert np.all(image[..., 2] == 0.0) and np.all(image[..., 3] == 1.0)
    # refusals: Error() and ([], [])
    cfg.FixedLayer, cfg.EddyThreshold, cfg.EddyMinCells = 0.0, 0.2, 0
    assert M.MOPS_RunEddyCensus(cfg) == ([], [])
    cfg.EddyMinCells, cfg.EddyThreshold = 4, float("nan")
    assert M.MOPS_RunEddyCensus(cfg) == ([], [])
    cfg.EddyThreshold = 0.2
    cfg.imageSize = (0, EC.HEIGHT)
    assert M.MOPS_RunEddyCensus(cfg) == ([], [])
    assert M.MOPS_RunEddyCensus(None) == ([], [])
    M.MOPS_Init("gpu")
    cfg.imageSize = (EC.WIDTH, EC.HEIGHT)
    assert M.MOPS_RunEddyCensus(cfg) == ([], [])              # no solution
