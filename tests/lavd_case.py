"""What the LAVD tests of the outer layers share: the window, the trajectory settings and the engine-level image
(PathlineChain.run(attrs=True, integrals=...) over two snapshots) that pyMOPS, the C++ API and MOPSPathline must
reproduce byte for byte.

TEST INFRASTRUCTURE ONLY: the product never imports this module.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eddy_case as EC  # noqa: E402

WIDTH, HEIGHT, LAT, LON = EC.WIDTH, EC.HEIGHT, EC.LAT, EC.LON   # 36 x 18 = 648 particles
DEPTH = 300.0
DT, RT, GAP = 600, 3600, 21600
NAME = "vorticity_deviation"


def engine_image(dm, snaps, gaps=GAP, method=1, delta_t=DT, record_t=RT, depth=DEPTH, width=WIDTH, height=HEIGHT,
                 horizon=None):
    """The LAVD image [H, W, 4] (host) of a chain over ``snaps`` on the device mesh ``dm``."""
    from mops_amd.chain import EverDead, PathlineChain, snapshot_field_factory, vorticity_deviation_factory
    from mops_amd.engine import FlowMapLattice, PathIntegral
    lat = FlowMapLattice(width, height, LAT, LON)
    chain = PathlineChain(dm, snapshot_field_factory(dm, lambda i: snaps[i]), len(snaps), gap_seconds=gaps,
                          make_attrs=vorticity_deviation_factory(dm))
    it, ever = PathIntegral(lat.n), EverDead()
    chain.run(lat.seeds, depth=depth, method=method, delta_t=delta_t, record_t=record_t, keep_lines=False, attrs=True,
              integrals={NAME: it}, on_pair=ever)
    if horizon is None:
        horizon = float(sum(chain.gaps))
    return lat.lavd(it, ever.death(), horizon=horizon).cpu().numpy()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)
                                       and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes())
