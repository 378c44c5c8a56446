"""The cases the eddy-census tests share: the restatement's census of the small mesh at the two thresholds and the
synthetic class arrays of the labelling tests.

TEST INFRASTRUCTURE ONLY: the product never imports this module.  Everything here is computed on the CPU, once
per session, and never modified.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_reference as CR  # noqa: E402
import eddy_case as EC  # noqa: E402

LAYER = 0
K_SIGMAS = (0.2, 0.05)
MIN_CELLS = (1, 4, 10_000)

_CACHE = {}


def sigma(ow, layer):
    """The population standard deviation of the layer's finite Okubo-Weiss values (numpy, FP64)."""
    col = np.asarray(ow, dtype=np.float64)[:, layer]
    return float(np.std(col[np.isfinite(col)]))


def small(O, small_case):
    """eddy_case.small's dict plus area [C] and thresholds {k_sigma: threshold} of layer 0."""
    if "small" not in _CACHE:
        c = dict(EC.small(O, small_case))
        c["area"] = CR.cell_area(c["mesh"])
        s = sigma(c["g0"]["okubo_weiss"], LAYER)
        c["thresholds"] = {k: -k * s for k in K_SIGMAS}
        _CACHE["small"] = c
    return _CACHE["small"]


def census(O, small_case, k_sigma, min_cells, threshold=None):
    """The restatement's census of layer 0 of the small mesh (cached per threshold and min_cells)."""
    c = small(O, small_case)
    thr = c["thresholds"][k_sigma] if threshold is None else threshold
    key = ("census", thr, min_cells)
    if key not in _CACHE:
        _CACHE[key] = CR.census(c["mesh"], c["g0"]["vorticity"], c["g0"]["okubo_weiss"], LAYER, thr, min_cells,
                                area=c["area"])
    return _CACHE[key]


def synthetic_classes(mesh):
    """{name: int32 [C]} for the labelling tests."""
    C = int(mesh.nCells)
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    lat = np.degrees(np.arcsin(cc[:, 2] / np.linalg.norm(cc, axis=1)))
    single = np.zeros(C, dtype=np.int32)
    single[C // 3] = 1
    out = {
        "ones": np.ones(C, dtype=np.int32),
        "zeros": np.zeros(C, dtype=np.int32),
        "single": single,
        "random": np.random.default_rng(20).integers(-1, 2, C).astype(np.int32),
        "band": ((lat > -20.0) & (lat < -5.0)).astype(np.int32),
    }
    return out
