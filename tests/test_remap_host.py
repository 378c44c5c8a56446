"""Image remapping without a GPU: argument validation of the C ABI and of the Python wrappers, the host
cos / sin tables against the reference restatement (tests/remap_reference.py), and the restatement's own
reproduction of the reference's documented layer override."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import remap_reference as RR  # noqa: E402


def _cfg(_lib, w=8, h=4, rule=0):
    return _lib.RemapCfg(w, h, -90.0, 90.0, -180.0, 180.0, 800.0, 0.0, 0.0, 5000.0, rule)


def test_remap_invalid_arguments_need_no_device(engine_lib):
    """Bad arguments are answered with MOPS_ERR_INVALID before any device work (the reference's Error() + return,
    MPASOVisualizerKernels.cpp:240-243, :475-485): no device is needed and nothing is written."""
    from mops_amd import _lib
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below fails its argument check first
    out = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    good = _cfg(_lib)
    calls = [
        (None, fake, good), (fake, None, good), (fake, fake, None),
        (fake, fake, _cfg(_lib, w=0)), (fake, fake, _cfg(_lib, h=-3)), (fake, fake, _cfg(_lib, w=65536, h=65536)),
        (fake, fake, _cfg(_lib, rule=2)),
    ]
    for mesh, field, cfg in calls:
        ref = None if cfg is None else C.byref(cfg)
        assert engine_lib.mops_remap_fixed_depth(mesh, field, ref, 0, None, None, out, None, None, None) == \
            _lib.MOPS_ERR_INVALID
        assert b"mops_remap_fixed_depth" in engine_lib.mops_last_error()
        assert engine_lib.mops_remap_fixed_latitude(mesh, field, ref, out, None, None) == _lib.MOPS_ERR_INVALID
    # no output buffer
    assert engine_lib.mops_remap_fixed_depth(fake, fake, C.byref(good), 0, None, None, None, None, None, None) == \
        _lib.MOPS_ERR_INVALID
    assert engine_lib.mops_remap_fixed_latitude(fake, fake, C.byref(good), None, None, None) == _lib.MOPS_ERR_INVALID
    assert list(out) == [7.0] * 4
    # MOPSApp::runRemapping's image count (MOPSApp.cpp:176-185)
    assert [engine_lib.mops_remap_num_images(k) for k in range(8)] == [1, 2, 2, 2, 3, 3, 3, 4]
    bad = _cfg(_lib, w=0)
    t = np.empty(8)
    p = t.ctypes.data_as(C.c_void_p)
    assert engine_lib.mops_remap_tables(C.byref(bad), 0, p, p, p, p) == _lib.MOPS_ERR_INVALID


def test_remap_python_argument_checks():
    from mops_amd import engine
    with pytest.raises(ValueError, match="layer_rule"):
        engine._remap_cfg(8, 4, layer_rule="nearest")
    for w, h in ((0, 4), (8, -1), (65536, 65536)):
        with pytest.raises(ValueError, match="image size"):
            engine._remap_cfg(w, h)
    with pytest.raises(ValueError, match="first two attributes"):
        engine.remap_fixed_depth(None, None, 8, 4, (-90, 90), (-180, 180), 0.0, n_attr=2, vertex_attrs=())


@pytest.mark.parametrize("w,h,lat,lon", [(48, 24, (-90.0, 90.0), (-180.0, 180.0)),
                                         (40, 32, (-60.0, 60.0), (-170.0, 150.0)), (7, 3, (-33.3, 71.7), (12.5, 13.0))])
def test_remap_depth_tables_match_the_restatement(engine_lib, w, h, lat, lon):
    """The host tables hold exactly the cos / sin the reference evaluates per pixel (GeoConverter.hpp:28-32,
    :120-121), and positions formed from them in its order are its positions, bit for bit."""
    from mops_amd import engine
    rc, rs, cc, cs = engine.remap_tables(w, h, lat, lon)
    for i in range(h):
        for j in range(w):
            theta, phi = RR.pixel_latlon(w, h, lat, lon, i, j)
            assert (rc[i], rs[i], cc[j], cs[j]) == (math.cos(theta), math.sin(theta), math.cos(phi), math.sin(phi))
    r = RR.R_EARTH
    pts = np.stack([(r * rc)[:, None] * cc[None, :], (r * rc)[:, None] * cs[None, :],
                    np.broadcast_to((r * rs)[:, None], (h, w))], axis=-1).reshape(-1, 3)
    assert np.array_equal(pts, RR.depth_positions(w, h, lat, lon))


def test_remap_latitude_tables_match_the_restatement(engine_lib):
    from mops_amd import engine
    w, lon, flat = 36, (-170.0, 150.0), 20.0
    rc, rs, cc, cs = engine.remap_tables(w, 20, lon_range=lon, latitude=flat)
    assert rc.shape == (1,) and cc.shape == (w,)
    r = RR.R_EARTH
    pts = np.stack([r * rc[0] * cc, r * rc[0] * cs, np.full(w, r * rs[0])], axis=-1)
    assert np.array_equal(pts, RR.latitude_positions(w, lon, flat))
    # one column: j_step = 0 (MPASOVisualizerKernels.cpp:514)
    _, _, c1, s1 = engine.remap_tables(1, 5, lon_range=lon, latitude=flat)
    assert (c1[0], s1[0]) == (math.cos(lon[0] * (math.pi / 180.0)), math.sin(lon[0] * (math.pi / 180.0)))


def test_restatement_reproduces_the_layer_override(oracle_lib, small_case):
    """Quirk Q13: MPASOVisualizerKernels.cpp:392-394 force layer 0 for every depth at or below the column top, so
    at 800 m every valid pixel of a global image is layer 0 (1055 of them on this mesh); without those lines
    ("bracket") the same pixels land in deeper layers."""
    mesh, s0, _ = small_case
    d = oracle_lib.preprocess(mesh, s0)
    w, h, lat, lon = 48, 24, (-90.0, 90.0), (-180.0, 180.0)
    cells = oracle_lib.knn(mesh, RR.depth_positions(w, h, lat, lon))
    ref = RR.fixed_depth(mesh, d, w, h, lat, lon, 800.0, cells)
    valid = ref["code"] == RR.VALID
    assert valid.sum() == 1055 and (ref["code"] == RR.OUTSIDE).sum() == 92
    assert (ref["code"] == RR.OUT_OF_RANGE).sum() == 5
    assert np.all(ref["layer"][valid] == 0)
    assert np.all(np.isfinite(ref["images"][0][valid])) and np.all(np.isnan(ref["images"][0][~valid][:, :3]))
    assert np.all(ref["images"][0][..., 3] == 1.0)  # alpha 1 on NaN pixels too
    br = RR.fixed_depth(mesh, d, w, h, lat, lon, 800.0, cells, layer_rule="bracket")
    bvalid = br["code"] == RR.VALID
    assert bvalid.sum() > 0.4 * w * h and np.all(br["layer"][bvalid] >= 1)
    assert not np.array_equal(br["images"][0], ref["images"][0], equal_nan=True)
