"""Particle density maps without a GPU: the three C entry points are exported with matching ctypes stubs, every
invalid argument is answered with MOPS_ERR_INVALID before any device work (fake handles, as
tests/test_remap_host.py), mops_density_bytes, and the numpy restatement (tests/density_reference.py) against a
brute-force Python loop."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_reference as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _cfg(_lib, w=8, h=4, lat=(-90.0, 90.0), lon=(-180.0, 180.0)):
    return _lib.RemapCfg(w, h, lat[0], lat[1], lon[0], lon[1], 0.0, 0.0, 0.0, 0.0, 0, 0.0)


def test_symbols_stubs_and_constants(engine_lib):
    from mops_amd import _lib
    text = open(os.path.join(ROOT, "include", "mops_traj.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("mops_density_bytes", 2), ("mops_density_accumulate", 15), ("mops_density_image", 5)):
        assert name in _lib.EXPORTED and hasattr(engine_lib, name)
        m = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        stub = getattr(engine_lib, name).argtypes
        assert len(params) == n_args == len(stub), name
        for p, t in zip(params, stub):  # pointers as void*, the integers by width
            want = C.c_void_p if "*" in p else {"int64_t": C.c_int64, "int32_t": C.c_int32}[p.split()[0]]
            assert t is want, (name, p)
    assert engine_lib.mops_density_bytes.restype is C.c_int64
    m = re.search(r"MOPS_DENSITY_COUNT\s*=\s*(\d+),\s*MOPS_DENSITY_SPEED\s*=\s*(\d+),\s*MOPS_DENSITY_VALUES\s*=\s*(\d+)",
                  code)
    assert m and tuple(int(g) for g in m.groups()) == (0, 1, 2)
    assert (_lib.MOPS_DENSITY_COUNT, _lib.MOPS_DENSITY_SPEED, _lib.MOPS_DENSITY_VALUES) == (0, 1, 2)
    assert "2^39" in text  # the overflow bound is stated in the header


def test_density_bytes(engine_lib):
    f = engine_lib.mops_density_bytes
    assert f(1, 1) == 16 and f(64, 32) == 64 * 32 * 16 and f(3601, 1801) == 3601 * 1801 * 16
    assert f(46340, 46340) == 46340 * 46340 * 16        # 2 147 395 600 pixels, below 2^31
    assert f(32768, 65535) == 32768 * 65535 * 16        # 2^31 - 32768
    for w, h in ((0, 4), (4, 0), (-1, 4), (4, -7), (65536, 32768), (46341, 46341)):  # 2^31 and above
        assert f(w, h) == -1, (w, h)


def test_invalid_arguments_need_no_device(engine_lib):
    from mops_amd import _lib
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below fails its argument check first
    good = _cfg(_lib)

    def acc(cfg, n=4, k0=0, k1=3, pts=fake, kind=0, vals=None, accum=fake):
        ref = None if cfg is None else C.byref(cfg)
        return engine_lib.mops_density_accumulate(ref, n, k0, k1, pts, 24, 1, 4, None, kind, vals, 0, 0, accum, None)

    def img(cfg, accum=fake, out=fake):
        return engine_lib.mops_density_image(None if cfg is None else C.byref(cfg), accum, 1, out, None)

    bad_cfgs = [None, _cfg(_lib, w=0), _cfg(_lib, h=0), _cfg(_lib, w=-2), _cfg(_lib, w=65536, h=32768),
                _cfg(_lib, lat=(NAN, 90.0)), _cfg(_lib, lat=(-90.0, INF)), _cfg(_lib, lon=(-INF, 180.0)),
                _cfg(_lib, lon=(0.0, NAN)), _cfg(_lib, lat=(10.0, 10.0)), _cfg(_lib, lat=(20.0, 10.0)),
                _cfg(_lib, lon=(30.0, 30.0)), _cfg(_lib, lon=(30.0, -30.0)), _cfg(_lib, lon=(-180.0, 180.5)),
                _cfg(_lib, lon=(0.0, 720.0))]
    for cfg in bad_cfgs:
        assert acc(cfg) == _lib.MOPS_ERR_INVALID
        assert b"mops_density_accumulate" in engine_lib.mops_last_error()
        assert img(cfg) == _lib.MOPS_ERR_INVALID
        assert b"mops_density_image" in engine_lib.mops_last_error()
    # null pointers
    assert acc(good, pts=None) == _lib.MOPS_ERR_INVALID and acc(good, accum=None) == _lib.MOPS_ERR_INVALID
    assert img(good, accum=None) == _lib.MOPS_ERR_INVALID and img(good, out=None) == _lib.MOPS_ERR_INVALID
    # a bad kind, VALUES without values, negative counts
    for kind in (-1, 3, 7):
        assert acc(good, kind=kind) == _lib.MOPS_ERR_INVALID
    assert acc(good, kind=_lib.MOPS_DENSITY_VALUES, vals=None) == _lib.MOPS_ERR_INVALID
    assert acc(good, n=-1) == _lib.MOPS_ERR_INVALID and acc(good, k0=-1) == _lib.MOPS_ERR_INVALID
    # bad arguments win over an empty call
    assert acc(_cfg(_lib, w=0), n=0) == _lib.MOPS_ERR_INVALID and acc(good, n=0, kind=9) == _lib.MOPS_ERR_INVALID
    # nothing to do: MOPS_OK without a launch (still no device)
    assert acc(good, n=0) == _lib.MOPS_OK
    assert acc(good, k0=0, k1=0) == _lib.MOPS_OK and acc(good, k0=5, k1=3) == _lib.MOPS_OK
    assert acc(good, n=0, kind=_lib.MOPS_DENSITY_VALUES, vals=fake) == _lib.MOPS_OK


def test_python_argument_checks():
    """DensityMap refuses what the C entry refuses before it allocates anything."""
    from mops_amd import engine
    for w, h in ((0, 4), (8, -1), (65536, 32768)):
        with pytest.raises(ValueError, match="image size"):
            engine.DensityMap(w, h, (-90, 90), (-180, 180), device="cpu")
    for lat, lon in (((10, 10), (-180, 180)), ((-90, 90), (0, 361)), ((NAN, 90), (-180, 180)), ((-90, 90), (5, -5))):
        with pytest.raises(ValueError, match="range"):
            engine.DensityMap(8, 4, lat, lon, device="cpu")
    with pytest.raises(ValueError, match="value"):
        engine.DensityMap(8, 4, (-90, 90), (-180, 180), value=3, device="cpu")


def _sphere(lat_deg, lon_deg, r=6371000.0):
    la, lo = math.radians(lat_deg), math.radians(lon_deg)
    return [r * math.cos(la) * math.cos(lo), r * math.cos(la) * math.sin(lo), r * math.sin(la)]


def test_restatement_against_brute_force():
    """50 points, one on each window edge: fr == 0 (the top edge) is inside, fr == height (the bottom edge) is
    outside, likewise fc == 0 and fc == width; plus the skipped kinds of point and value."""
    W, H, lat, lon = 16, 8, (-90.0, 90.0), (0.0, 180.0)
    R = 6371000.0
    rng = np.random.default_rng(3)
    pts = [_sphere(a, b) for a, b in zip(rng.uniform(-80, 80, 38), rng.uniform(-180, 180, 38))]
    # exactly on the edges: the poles give z / r = +-1 and lat = +-90, the x axis gives lon = 0 and 180
    top, bottom, left, right = [0.0, 0.0, R], [0.0, 0.0, -R], [R, 0.0, 0.0], [-R, 0.0, 0.0]
    _, fr, fc = D.pixel_coords([top, bottom, left, right], W, H, lat, lon)
    assert fr[0] == 0.0 and fr[1] == float(H) and fc[0] == 0.0 and fc[2] == 0.0 and fc[3] == float(W)
    pts += [top, bottom, left, right]
    pts += [[NAN, 1.0, 1.0], [1.0, INF, 1.0], [1.0, 1.0, -INF], [0.0, 0.0, 0.0]]           # skipped points
    pts += [_sphere(0.5, 90.0), _sphere(10.0, 100.0), _sphere(-10.0, 170.0), _sphere(39.0, 1.0)]
    pts = np.asarray(pts)
    assert pts.shape == (50, 3)
    vals = rng.uniform(-30.0, 30.0, 50)
    vals[46] = NAN            # a non-finite value skips its point
    vals[47] = 2.0 ** 38      # and so does |v| >= 2^38
    vals[48] = -(2.0 ** 38 - 1.0)  # the largest magnitudes below the limit are kept
    vals[49] = 0.5 + 2.0 ** -25    # a tie: v * 2^24 = 8388608.5 rounds to even
    for v in (None, vals):
        want = D.brute_force(pts, W, H, lat, lon, v)
        got = D.accumulate(D.new_accum(W, H), pts, W, H, lat, lon, v)
        assert got.dtype == np.int64 and np.array_equal(got, want)
    cnt = D.accumulate(D.new_accum(W, H), pts, W, H, lat, lon)
    one = lambda p: D.accumulate(D.new_accum(W, H), [p], W, H, lat, lon)[:, :, 0]
    assert one(top).sum() == 1 and one(top)[0].sum() == 1        # fr == 0: row 0
    assert one(bottom).sum() == 0                                 # fr == height: outside
    assert one(left).sum() == 1 and one(left)[:, 0].sum() == 1    # fc == 0: column 0
    assert one(right).sum() == 0                                  # fc == width: outside
    assert 6 <= cnt[:, :, 0].sum() <= 46 and cnt[:, :, 1].sum() == 0
    val = D.accumulate(D.new_accum(W, H), pts, W, H, lat, lon, vals)
    assert val[:, :, 0].sum() == cnt[:, :, 0].sum() - 2           # points 46 and 47 left out, 48 and 49 kept
    ok, q = D.quantise([0.5 + 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, -0.5 * 2.0 ** -24])
    assert ok.all() and q.tolist() == [8388608, 2, 2, 0]


def test_restatement_image_and_wrap():
    W, H = 12, 6
    pts = np.asarray([_sphere(10.0, -170.0), _sphere(10.0, -170.0), _sphere(-50.0, 20.0)])
    a = D.accumulate(D.new_accum(W, H), pts, W, H, (-90.0, 90.0), (-180.0, 180.0), [1.5, 2.5, -4.0])
    b = D.accumulate(D.new_accum(W, H), pts, W, H, (-90.0, 90.0), (0.0, 360.0), [1.5, 2.5, -4.0])
    assert np.array_equal(b, np.roll(a, W // 2, axis=1))  # [0, 360] is [-180, 180] rolled by half the width
    img = D.image(a)
    r, c = np.argwhere(a[:, :, 0] == 2)[0]
    assert img[r, c].tolist() == [2.0, 2.0, 4.0, 1.0]
    r1, c1 = np.argwhere(a[:, :, 0] == 1)[0]
    assert img[r1, c1].tolist() == [1.0, -4.0, -4.0, 1.0]
    empty = a[:, :, 0] == 0
    assert np.isnan(img[empty][:, :3]).all() and (img[:, :, 3] == 1.0).all()
    img0 = D.image(a, nan_empty=False)
    assert (img0[empty][:, 0] == 0).all() and (img0[empty][:, 2] == 0).all() and np.isnan(img0[empty][:, 1]).all()
