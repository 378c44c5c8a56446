"""The cases the eddy-field tests share: the restatement's arrays on the small mesh and the images, sections and
pathline samples composed from them by the existing restatements.

TEST INFRASTRUCTURE ONLY: the product never imports this module.  Everything here is computed on the CPU, once
per session, and never modified.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eddy_reference as ER  # noqa: E402
import remap_reference as RR  # noqa: E402

# the fixed-depth image of the composition tests: 36 x 18 = 648 pixels, no multiple of 64, W != H
WIDTH, HEIGHT = 36, 18
LAT, LON = (-60.0, 60.0), (-170.0, 150.0)
DEPTH = 800.0
RULES = ("reference", "bracket")
# the keys put vorticity first in std::map (sorted) order: image 1 = {vorticity, okubo_weiss, 0, 1}
KEYS = {"vorticity": "0_vorticity", "okubo_weiss": "1_okubo_weiss"}

_CACHE = {}


def small(O, small_case):
    """dict(mesh, s0, s1, d0, d1: oracle-derived fields, g0, g1: {name: [C, L]} of the restatement, v0, v1:
    {name: [V, L]} signed vertex arrays of vorticity and okubo_weiss)."""
    if "small" not in _CACHE:
        mesh, s0, s1 = small_case
        d0, d1 = O.preprocess(mesh, s0), O.preprocess(mesh, s1)
        g0, g1 = ER.velocity_gradient(mesh, d0.vertex_vel), ER.velocity_gradient(mesh, d1.vertex_vel)
        v0 = {k: ER.cell_to_vertex_signed(mesh, g0[k]) for k in KEYS}
        v1 = {k: ER.cell_to_vertex_signed(mesh, g1[k]) for k in KEYS}
        _CACHE["small"] = dict(mesh=mesh, s0=s0, s1=s1, d0=d0, d1=d1, g0=g0, g1=g1, v0=v0, v1=v1)
    return _CACHE["small"]


def derived_with_eddy(O, d, v, names=("vorticity", "okubo_weiss")):
    """The oracle's derived fields with the signed vertex arrays as their attributes."""
    return O.Derived(d.vertex_ztop, d.vertex_vel, d.vertex_w, {KEYS[k]: v[k].reshape(-1) for k in names})


def depth_cells(O, small_case):
    if "cells" not in _CACHE:
        _CACHE["cells"] = O.knn(small_case[0], RR.depth_positions(WIDTH, HEIGHT, LAT, LON))
    return _CACHE["cells"]


def depth_image(O, small_case, rule):
    """remap_reference.fixed_depth fed the signed vertex arrays: its result dict (images[1] is the eddy map)."""
    key = ("depth", rule)
    if key not in _CACHE:
        c = small(O, small_case)
        ref = RR.fixed_depth(c["mesh"], derived_with_eddy(O, c["d0"], c["v0"]), WIDTH, HEIGHT, LAT, LON, DEPTH,
                             depth_cells(O, small_case), layer_rule=rule)
        valid = ref["code"] == RR.VALID
        img = ref["images"][1]
        assert valid.sum() >= 0.4 * valid.size and (~valid).sum() >= 0.05 * valid.size
        assert (img[valid][:, 0] > 0).any() and (img[valid][:, 0] < 0).any()      # vorticity of both signs
        assert (img[valid][:, 1] > 0).any() and (img[valid][:, 1] < 0).any()      # strain- and rotation-dominated
        _CACHE[key] = ref
    return _CACHE[key]
