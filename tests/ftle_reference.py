"""numpy restatement of "flow-map lattices and FTLE" (include/mops_traj.h).

TEST INFRASTRUCTURE ONLY (like oracle/ and tests/density_reference.py): the product never imports this module.
The lattice is formed from the engine's own host tables (``engine.remap_tables`` -> mops_remap_tables, libm cos /
sin, pinned by tests/test_remap_host.py), with the remapping kernel's expression ``r * cos(lat) * cos(lon)``; the
image is the header's ten steps in float64 numpy ufuncs, one IEEE operation each (no contraction), every dot product
summed as ``(x*x + y*y) + z*z``.  tests/test_ftle_cpu.py pins it: exact rigid maps, a shear with a closed form, and
the one-sided rule against a scalar loop written from the header independently."""
import numpy as np

RADIUS = 6371010.0  # kRemapRadius (GeoConverter.hpp:107)
NAN = float("nan")


def lattice(width, height, lat_range, lon_range):
    """Seeds [H*W, 3], row major, row 0 at lat_range[1]: (r*cos(lat))*cos(lon), (r*cos(lat))*sin(lon), r*sin(lat)."""
    from mops_amd.engine import remap_tables
    rc, rs, cc, cs = remap_tables(width, height, lat_range, lon_range)
    rcos = RADIUS * rc
    out = np.empty((height, width, 3))
    out[:, :, 0] = rcos[:, None] * cc[None, :]
    out[:, :, 1] = rcos[:, None] * cs[None, :]
    out[:, :, 2] = (RADIUS * rs)[:, None]
    return out.reshape(-1, 3)


def lattice_angles(width, height, lat_range, lon_range):
    """(lat [H], lon [W]) in radians: GeoConverter::convertPixelToLatLonToRadians, the tables' arguments."""
    i = np.arange(height, dtype=np.float64)
    j = np.arange(width, dtype=np.float64)
    lat = lat_range[1] - (i / float(height) * (lat_range[1] - lat_range[0]))
    lon = (j / float(width) * (lon_range[1] - lon_range[0])) + lon_range[0]
    return lat * (np.pi / 180.0), lon * (np.pi / 180.0)


def sphere(lat, lon, radius=RADIUS):
    """Points [..., 3] at radians lat / lon (broadcast)."""
    lat, lon = np.broadcast_arrays(lat, lon)
    return np.stack([radius * np.cos(lat) * np.cos(lon), radius * np.cos(lat) * np.sin(lon), radius * np.sin(lat)], -1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _unit(p):
    """(p / |p| component-wise, usable): usable iff p is finite and |p| != 0."""
    r = np.sqrt(_dot(p, p))
    ok = np.isfinite(p).all(axis=-1) & (r != 0.0)
    return p / r[..., None], ok


def wrap_lon(lon_range) -> bool:
    return float(lon_range[1]) - float(lon_range[0]) == 360.0


def ftle_image(width, height, seeds, last, death=None, horizon=1.0, wrap=False):
    """The image [H, W, 4] = {ftle, lambda_max, lambda_min, 1}; invalid pixels {NaN, NaN, NaN, 1}."""
    W, H = int(width), int(height)
    with np.errstate(all="ignore"):
        s, ok_s = _unit(np.asarray(seeds, dtype=np.float64).reshape(H, W, 3))
        u, ok_u = _unit(np.asarray(last, dtype=np.float64).reshape(H, W, 3))
        valid = ok_s & ok_u
        if death is not None:
            valid &= np.asarray(death).reshape(H, W) < 0
        I, J = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")

        def side(idx, step, size, wraps, rows):
            c = idx + step
            exists = np.ones_like(c, dtype=bool) if wraps else ((c >= 0) & (c < size))
            c = c % size
            v = valid[c, J] if rows else valid[I, c]
            return np.where(exists & v, c, idx)

        JM, JP = side(J, -1, W, bool(wrap), False), side(J, +1, W, bool(wrap), False)
        IM, IP = side(I, -1, H, False, True), side(I, +1, H, False, True)
        dE = s[I, JP] - s[I, JM]
        dN = s[IM, J] - s[IP, J]
        hE, hN = np.sqrt(_dot(dE, dE)), np.sqrt(_dot(dN, dN))
        ok = valid & (JM != JP) & (IM != IP) & (hE != 0.0) & (hN != 0.0)
        a = (u[I, JP] - u[I, JM]) / hE[..., None]
        b = (u[IM, J] - u[IP, J]) / hN[..., None]
        c11, c12, c22 = _dot(a, a), _dot(a, b), _dot(b, b)
        m, d = 0.5 * (c11 + c22), 0.5 * (c11 - c22)
        q = np.sqrt(d * d + c12 * c12)
        lmax, lmin = m + q, m - q
        img = np.empty((H, W, 4))
        img[:, :, 0] = np.where(ok, np.log(lmax) / (2.0 * float(horizon)), NAN)
        img[:, :, 1] = np.where(ok, lmax, NAN)
        img[:, :, 2] = np.where(ok, lmin, NAN)
        img[:, :, 3] = 1.0
    return img


def ulp_distance(a, b):
    """Largest distance in units in the last place between two float64 arrays over the entries finite in both (the
    integer distance of the ordered bit patterns), 0 for none."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    sel = np.isfinite(a) & np.isfinite(b)
    if not sel.any():
        return 0

    def key(x):
        k = x.view(np.int64).copy()
        neg = k < 0
        k[neg] = np.int64(-2 ** 63) - k[neg]  # -0.0 -> 0, more negative values -> more negative keys
        return k.astype(object)

    return int(max(abs(p - q) for p, q in zip(key(a[sel]), key(b[sel]))))


# ---- shared cases ---------------------------------------------------------------------------------------------
def shear_last(width, height, lat_range, lon_range, k=0.5, radius=RADIUS - 37.0):
    """The flow map lon' = lon + k * lat on the lattice's angles (radians), on a sphere of another radius (the
    image must not depend on |last|).  [H*W, 3]."""
    lat, lon = lattice_angles(width, height, lat_range, lon_range)
    return sphere(lat[:, None], lon[None, :] + k * lat[:, None], radius).reshape(-1, 3)


DEAD_5x7 = dict(width=7, height=5, lat_range=(-10.0, 10.0), lon_range=(20.0, 48.0))


def dead_case_5x7():
    """(seed-order death array [35], {name: (i, j)} of the pixels the patterns are about) on the 5 x 7 window:
    a dead centre; a dead j-1; dead j-1 and j+1 together; a dead i+1."""
    death = np.full((5, 7), -1, dtype=np.int32)
    death[0, 1] = 3            # 'dead_centre' (0, 1) itself (also the j-1 of (0, 2) and the i-1 of (1, 1))
    death[2, 2] = 0            # the j-1 of (2, 3) and the j+1 of (2, 1); died at step 0
    death[4, 3] = 7; death[4, 5] = 7  # both east neighbours of (4, 4)
    death[3, 6] = 11           # the i+1 of (2, 6)
    about = dict(dead_centre=(0, 1), dead_jm=(2, 3), dead_jm_jp=(4, 4), dead_ip=(2, 6))
    return death.reshape(-1), about


E2E = dict(width=24, height=16, lat_range=(-80.0, 80.0), lon_range=(-180.0, 180.0))
E2E_DEPTH = 300.0


def e2e_lines(small_case, method=1):
    """MOPS_RunPathLine's list[dict] for the E2E lattice over the shared mesh (36 steps; GPU): what the pyMOPS and
    C++ tests feed to MOPS_RunFTLE.  (lines, horizon in days)."""
    import pathline_attr_reference as R
    from mops_amd import engine
    mesh, s0, s1 = small_case
    dm = engine.DeviceMesh.from_mesh(mesh)
    f0, f1 = engine.DeviceField.from_snapshot(dm, s0), engine.DeviceField.from_snapshot(dm, s1)
    cfg = engine.TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T,
                                  depth=E2E_DEPTH, method=method)
    got = engine.run_trajectories(dm, f0, f1, cfg, lattice(**E2E))
    n = got["points"].shape[0]
    lines = [dict(lineID=i, points=got["points"][i], velocity=got["velocity"][i], temperature=got["temperature"][i],
                  salinity=got["salinity"][i], lastPoint=got["lastPoint"][i]) for i in range(n)]
    return lines, R.DURATION / 86400.0


def lines_image(lines, horizon, **window):
    """The restatement's image of lines in lattice order: points[0] -> lastPoint, no death array."""
    seeds = np.stack([ln["points"][0] for ln in lines])
    last = np.stack([ln["lastPoint"] for ln in lines])
    return ftle_image(window["width"], window["height"], seeds, last, None, horizon, wrap_lon(window["lon_range"]))
