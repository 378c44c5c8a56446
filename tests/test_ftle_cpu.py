"""CPU: the numpy restatement of the FTLE semantics (tests/ftle_reference.py) against facts that do not depend on
it -- exact rigid maps, a shear with a closed form, and the one-sided rule against a scalar loop written from the
header's ten steps -- plus the ABI's argument checks, which run before any device work."""
import ctypes as C
import math

import numpy as np

import ftle_reference as F

U = 2.0 ** -53  # unit roundoff of float64


def test_symbols_are_exported(engine_lib):
    from mops_amd import _lib
    for name in ("mops_flowmap_lattice", "mops_ftle_image"):
        assert name in _lib.EXPORTED and hasattr(engine_lib, name)


def test_invalid_arguments_are_refused_before_any_device_work(engine_lib):
    """MOPS_ERR_INVALID for a null pointer, a non-positive size, H*W >= 2^31, horizon <= 0 or not finite.  The
    pointers are never dereferenced (the checks come first), so this runs without a GPU."""
    from mops_amd import _lib
    from mops_amd.engine import _remap_cfg
    lib = engine_lib
    ok = _remap_cfg(4, 3, (-10.0, 10.0), (0.0, 40.0))
    p = C.c_void_p(4096)  # non-null, never read

    def ftle(cfg=ok, seeds=p, last=p, horizon=1.0, image=p):
        return lib.mops_ftle_image(None if cfg is None else C.byref(cfg), seeds, last, None, horizon, 0, image, None)

    assert ftle(cfg=None) == _lib.MOPS_ERR_INVALID
    assert ftle(seeds=None) == _lib.MOPS_ERR_INVALID
    assert ftle(last=None) == _lib.MOPS_ERR_INVALID
    assert ftle(image=None) == _lib.MOPS_ERR_INVALID
    for h in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert ftle(horizon=h) == _lib.MOPS_ERR_INVALID, h
    for w, h in ((0, 3), (4, 0), (-1, 3), (4, -2), (65536, 32768), (2 ** 31 - 1, 2)):
        bad = _lib.RemapCfg(w, h, -10.0, 10.0, 0.0, 40.0, 0.0, 0.0, 0.0, 0.0, 0, 0.0)
        assert ftle(cfg=bad) == _lib.MOPS_ERR_INVALID, (w, h)
        assert lib.mops_flowmap_lattice(C.byref(bad), p, None) == _lib.MOPS_ERR_INVALID, (w, h)
    assert lib.mops_flowmap_lattice(None, p, None) == _lib.MOPS_ERR_INVALID
    assert lib.mops_flowmap_lattice(C.byref(ok), None, None) == _lib.MOPS_ERR_INVALID
    assert b"mops_flowmap_lattice" in lib.mops_last_error()


def test_lattice_is_the_remapping_lattice(engine_lib):
    """Row 0 is max_lat, rows run south, columns east; every seed has the remapping's radius to rounding."""
    W, H, lat, lon = 6, 4, (-30.0, 50.0), (100.0, 220.0)
    s = F.lattice(W, H, lat, lon).reshape(H, W, 3)
    la, lo = F.lattice_angles(W, H, lat, lon)
    assert la[0] == math.radians(50.0) and np.all(np.diff(la) < 0) and np.all(np.diff(lo) > 0)
    assert np.allclose(s, F.sphere(la[:, None], lo[None, :]), rtol=1e-14, atol=1e-6)
    assert np.allclose(np.linalg.norm(s, axis=-1), F.RADIUS, rtol=1e-14)


def test_identity_and_exact_rigid_maps(engine_lib):
    """The identity flow map and the rigid maps (x, y, z) -> (-y, x, z) and (x, y, z) -> (x, -y, -z) -- exact in
    floating point: a permutation and sign changes -- give bit-identical images: every square and product is the
    same double, and (x*x + y*y) + z*z only swaps the operands of its first, commutative, addition.

    Bound on |lambda - 1| for a pixel whose four neighbours all exist (u = 2^-53; higher orders are covered by
    rounding every count up).  The numerator of a is the very vector e = s[i,jp] - s[i,jm] the spacing hE is the
    length of, so from the sum S = fl((ex^2 + ey^2) + ez^2) to the quotient C11 = fl(a.a):
        S = sum(e^2)(1 + t3)           three roundings per term (its product, two additions)
        hE = sqrt(S)(1 + t1)           the square root's
        a_k = e_k / hE (1 + t1)        the division's
        C11 = sum(a_k^2)(1 + t3)
    so C11 = sum(e^2)(1+t1)^2(1+t3) / (sum(e^2)(1+t3)(1+t1)^2) and |C11 - 1| <= 10u, likewise |C22 - 1| <= 10u;
    rounded up to 11u each.  Then |m - 1| <= 12u and |d| <= 12u (one addition each; the halving is exact).
    C12 is not zero in floating point: the two difference vectors are orthogonal only as far as the seeds are
    exact.  A component of s differs from the unit vector of the pixel's angles by at most 16u (cos / sin within
    one ulp, 2u, each; two products for x and y; the norm, half of a 3u sum plus its root's u; the quotient's u:
    2+2+1+1, the same 6 again through the norm, 2.5, 1 -> 15.5u), so a component of e by at most 32u + u|e| and e
    as a vector by kappa <= sqrt(3) * 32u + u|e| <= 57u.  The exact difference vectors of a lattice with equal
    angle steps are orthogonal (the east chord is normal to the meridian plane the north chord lies in); unequal
    steps by roundings of the angles add less than 8u to the cosine.  So |a.b| <= kappa(1/hE + 1/hN) + 8u and
    |C12| <= |a.b| + 4u (three roundings, |a||b| <= 1 + 11u).  q = fl(sqrt(fl(d*d + C12*C12))) <= (|d| + |C12|)(1 +
    3u), and lambda = fl(m +- q) adds u.  Total: |lambda - 1| <= 12u + (12u + 12u + 57u(1/hE + 1/hN))(1 + 3u) + u
                                                              <= u * (40 + 60 (1/hE + 1/hN)),
    with hE = 2 cos(lat_i) sin(dlon), hN = 2 sin(dlat) from the window's angles -- geometry, not the code under
    test.  A pixel with a one-sided pair is outside this bound by design: its two chords meet at an angle that
    differs from a right angle by O(spacing), so the identity's C12 is O(spacing) there; for those the rigid
    maps' bit equality is the check."""
    for W, H, lat, lon in ((9, 7, (-60.0, 66.0), (-45.0, 45.0)), (16, 8, (-80.0, 80.0), (-180.0, 180.0))):
        seeds = F.lattice(W, H, lat, lon)
        wrap = F.wrap_lon(lon)
        ident = F.ftle_image(W, H, seeds, seeds, None, 1.0, wrap)
        rot = np.stack([-seeds[:, 1], seeds[:, 0], seeds[:, 2]], axis=1)
        flip = np.stack([seeds[:, 0], -seeds[:, 1], -seeds[:, 2]], axis=1)
        for name, last in (("rot", rot), ("flip", flip)):
            assert F.ftle_image(W, H, seeds, last, None, 1.0, wrap).tobytes() == ident.tobytes(), name
        assert not np.isnan(ident[:, :, 1]).any()  # every pixel has a stencil (H, W >= 2, nothing dead)
        la, lo = F.lattice_angles(W, H, lat, lon)
        dlat = math.radians((lat[1] - lat[0]) / H)
        dlon = math.radians((lon[1] - lon[0]) / W)
        hE = 2.0 * np.cos(la) * math.sin(dlon)
        hN = 2.0 * math.sin(dlat)
        bound = U * (40.0 + 60.0 * (1.0 / hE + 1.0 / hN))[:, None] * np.ones((1, W))
        inner = np.zeros((H, W), dtype=bool)
        inner[1:-1, :] = True
        if not wrap:
            inner[:, 0] = inner[:, -1] = False
        assert inner.sum() >= (H - 2) * (W - 2)
        for ch in (1, 2):
            err = np.abs(ident[:, :, ch] - 1.0)
            print(f"{W}x{H} channel {ch}: max |lambda - 1| / bound = {np.max(err[inner] / bound[inner]):.3g}")
            assert np.all(err[inner] <= bound[inner]), ch
        assert np.all(np.abs(ident[:, :, 0][inner]) <= bound[inner])  # |log(1 + x)| / 2 <= |x| for these x


def test_shear_converges_at_second_order(engine_lib):
    """lon' = lon + k * lat at the equator row is the simple shear [[1, k], [0, 1]] in the (east, north) frame:
    lambda_max = 1 + k^2/2 + k sqrt(1 + k^2/4).  Centred differences are second order in the spacing, so halving
    it cuts the error by 4; at least 3 is demanded."""
    k = 0.5
    want = 1.0 + k * k / 2.0 + k * math.sqrt(1.0 + k * k / 4.0)
    err = []
    for n in (16, 32):  # spacing 1 degree, then half a degree; row n/2 is the equator, exactly
        lat = lon = (-8.0, 8.0)
        la, _ = F.lattice_angles(n, n, lat, lon)
        assert la[n // 2] == 0.0
        img = F.ftle_image(n, n, F.lattice(n, n, lat, lon), F.shear_last(n, n, lat, lon, k), None, 1.0, False)
        err.append(abs(img[n // 2, n // 2, 1] - want))
        assert abs(img[n // 2, n // 2, 1] * img[n // 2, n // 2, 2] - 1.0) < 1e-3  # det C = 1: area preserving
    print(f"shear: error {err[0]:.3e} at 1 degree, {err[1]:.3e} at 0.5 degree, ratio {err[0] / err[1]:.3f}")
    assert err[1] > 1e-9  # far above rounding: the ratio measures truncation
    assert err[0] / err[1] >= 3.0


def _scalar_image(W, H, seeds, last, death, horizon, wrap):
    """The header's ten steps per pixel in Python floats (IEEE double, one operation at a time), written without
    the restatement's index arrays."""
    seeds = np.asarray(seeds, dtype=np.float64).reshape(H, W, 3).tolist()
    last = np.asarray(last, dtype=np.float64).reshape(H, W, 3).tolist()

    def unit(p):
        if not all(map(math.isfinite, p)):
            return None
        x, y, z = p
        r = math.sqrt((x * x + y * y) + z * z)
        return None if r == 0.0 else (x / r, y / r, z / r)

    def point(i, j):
        if death is not None and death[i * W + j] >= 0:
            return None
        s, u = unit(seeds[i][j]), unit(last[i][j])
        return None if s is None or u is None else (s, u)

    def diff(m, p):
        h3 = [p[0][k] - m[0][k] for k in range(3)]
        h = math.sqrt((h3[0] * h3[0] + h3[1] * h3[1]) + h3[2] * h3[2])
        return None if h == 0.0 else [(p[1][k] - m[1][k]) / h for k in range(3)]

    img = np.full((H, W, 4), np.nan)
    img[:, :, 3] = 1.0
    for i in range(H):
        for j in range(W):
            c = point(i, j)
            if c is None:
                continue
            jm, jp = j - 1, j + 1
            if wrap:
                jm, jp = jm % W, jp % W
            em = point(i, jm) if 0 <= jm < W else None
            ep = point(i, jp) if 0 <= jp < W else None
            nm = point(i - 1, j) if i - 1 >= 0 else None
            np_ = point(i + 1, j) if i + 1 < H else None
            jm, jp = (jm if em else j), (jp if ep else j)
            im, ip = (i - 1 if nm else i), (i + 1 if np_ else i)
            if jm == jp or im == ip:
                continue
            a, b = diff(em or c, ep or c), diff(np_ or c, nm or c)
            if a is None or b is None:
                continue
            c11 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
            c12 = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
            c22 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
            m, d = 0.5 * (c11 + c22), 0.5 * (c11 - c22)
            q = math.sqrt(d * d + c12 * c12)
            img[i, j, 1], img[i, j, 2] = m + q, m - q
            img[i, j, 0] = float(np.log(m + q)) / (2.0 * horizon)
    return img


def test_one_sided_rule_on_the_hand_made_case(engine_lib):
    c = F.DEAD_5x7
    W, H = c["width"], c["height"]
    seeds = F.lattice(**c)
    last = F.shear_last(**c, k=0.3)
    death, about = F.dead_case_5x7()
    for wrap in (False, True):
        got = F.ftle_image(W, H, seeds, last, death, 2.5, wrap)
        want = _scalar_image(W, H, seeds, last, death.tolist(), 2.5, wrap)
        assert got.tobytes() == want.tobytes(), wrap
    got = F.ftle_image(W, H, seeds, last, death, 2.5, False)
    alive = F.ftle_image(W, H, seeds, last, None, 2.5, False)
    nan = np.isnan(got[:, :, 1])
    assert np.array_equal(nan, np.isnan(got[:, :, 0])) and np.array_equal(nan, np.isnan(got[:, :, 2]))
    assert np.all(got[:, :, 3] == 1.0)
    assert nan[about["dead_centre"]]
    assert nan[about["dead_jm_jp"]] and death.reshape(H, W)[about["dead_jm_jp"]] < 0  # alive, but no east pair
    for key in ("dead_jm", "dead_ip"):  # one-sided: still a value, and not the centred one
        assert not nan[about[key]] and got[about[key]][1] != alive[about[key]][1], key
    dead = death.reshape(H, W) >= 0
    # invalid without being dead: (4, 4) between two dead columns; (4, 6) and (0, 0), whose only east neighbour died
    expect = dead.copy()
    for ij in ((4, 4), (4, 6), (0, 0)):
        assert not dead[ij]
        expect[ij] = True
    assert np.array_equal(nan, expect)
    # a pixel none of whose stencil points died is untouched by the deaths
    far = ~(dead | np.roll(dead, 1, 0) | np.roll(dead, -1, 0) | np.roll(dead, 1, 1) | np.roll(dead, -1, 1))
    assert far.any() and got[far].tobytes() == alive[far].tobytes()
    # a zero or non-finite last point is dead without a death array
    z = last.copy()
    z[death >= 0] = 0.0
    assert F.ftle_image(W, H, seeds, z, None, 2.5, False).tobytes() == got.tobytes()
    z[death >= 0] = np.inf
    assert F.ftle_image(W, H, seeds, z, None, 2.5, False).tobytes() == got.tobytes()


def test_degenerate_shapes_are_entirely_invalid(engine_lib):
    for W, H in ((1, 1), (5, 1), (1, 5)):
        seeds = F.lattice(W, H, (-10.0, 10.0), (0.0, 40.0))
        img = F.ftle_image(W, H, seeds, seeds, None, 1.0, False)
        assert np.isnan(img[:, :, :3]).all() and np.all(img[:, :, 3] == 1.0)


def test_ever_dead_collects_a_death_in_any_pair():
    """chain.EverDead ORs death >= 0 over the pairs, in seed order (plain objects stand in for the particle set)."""
    import torch
    from mops_amd.chain import EverDead

    class _Set:
        def __init__(self, death, ids):
            self.death, self.ids = torch.tensor(death, dtype=torch.int32), torch.tensor(ids, dtype=torch.int32)

        def original(self, t):
            out = torch.empty_like(t)
            out[self.ids.long()] = t
            return out

    ever = EverDead()
    ever(0, None, _Set([-1, 5, -1, -1], [2, 0, 1, 3]))  # slot 1 holds particle 0: it died in pair 0
    ever(1, None, _Set([-1, -1, 0, -1], [0, 1, 3, 2]))  # particle 0 lives again; particle 3 dies in pair 1
    assert ever.pairs == 2 and ever.mask.tolist() == [True, False, False, True]
    assert ever.death().tolist() == [0, -1, -1, 0] and ever.death().dtype == torch.int32
    assert not hasattr(ever, "reads_records")
