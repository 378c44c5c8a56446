"""numpy restatement of the particle density map (include/mops_traj.h, "particle density maps").

TEST INFRASTRUCTURE ONLY (like oracle/ and tests/remap_reference.py): the product never imports this module.
Every expression is the header's, in its order, on IEEE doubles: libm ``arcsin`` / ``arctan2``, ``np.rint`` (ties
to even) for the quantisation, ``np.add.at`` on int64 for the sums.  ``brute_force`` says the same with plain
Python floats, one point at a time, and pins this module (tests/test_density_cpu.py).

The device's asin / atan2 may differ from libm's by ulps, which can move a point that lies on a pixel edge.  So
every GPU comparison first asserts ``edge_distance(...) > EDGE_GUARD`` on its input -- no valid point within 1e-6
of a pixel of an edge -- and then demands equal bytes with nothing excluded.
"""
import math

import numpy as np

COUNT, SPEED, VALUES = 0, 1, 2
Q_SCALE = float(2 ** 24)
V_LIMIT = float(2 ** 38)
EDGE_GUARD = 1e-6
RAD2DEG = 180.0 / math.pi


def pixel_coords(points, width, height, lat_range, lon_range):
    """(valid [m] bool, fr [m], fc [m]) of points [m, 3]: ``valid`` = finite coordinates and r != 0."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y + z * z)
        valid = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (r != 0.0)
        rs = np.where(valid, r, 1.0)
        xs, ys, zs = np.where(valid, x, 1.0), np.where(valid, y, 0.0), np.where(valid, z, 0.0)
        lat = np.arcsin(np.clip(zs / rs, -1.0, 1.0)) * RAD2DEG
        lon = np.arctan2(ys, xs) * RAD2DEG
        lon = lon - 360.0 * np.floor((lon - lon_range[0]) / 360.0)
        fr = (lat_range[1] - lat) / (lat_range[1] - lat_range[0]) * float(height)
        fc = (lon - lon_range[0]) / (lon_range[1] - lon_range[0]) * float(width)
    return valid, fr, fc


def quantise(values):
    """(usable [m] bool, q [m] int64): q = llrint(v * 2^24); not usable where v is not finite or |v| >= 2^38."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        ok = np.isfinite(v) & (np.abs(v) < V_LIMIT)
        q = np.rint(np.where(ok, v, 0.0) * Q_SCALE).astype(np.int64)
    return ok, q


def speed(velocity):
    v = np.asarray(velocity, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def accumulate(accum, points, width, height, lat_range, lon_range, values=None):
    """Add points [m, 3] (``values`` [m] for a SPEED / VALUES map, None for COUNT) to accum [H, W, 2] int64."""
    valid, fr, fc = pixel_coords(points, width, height, lat_range, lon_range)
    inside = valid & (fr >= 0.0) & (fr < height) & (fc >= 0.0) & (fc < width)
    q = np.zeros(len(valid), dtype=np.int64)
    if values is not None:
        ok, q = quantise(values)
        inside &= ok
    row = np.floor(fr[inside]).astype(np.int64)
    col = np.floor(fc[inside]).astype(np.int64)
    np.add.at(accum[:, :, 0], (row, col), 1)
    if values is not None:
        np.add.at(accum[:, :, 1], (row, col), q[inside])
    return accum


def new_accum(width, height):
    return np.zeros((height, width, 2), dtype=np.int64)


def records_accumulate(accum, records, n, width, height, lat_range, lon_range, kind=COUNT, attr=None, k_range=None,
                       seeds=None):
    """A record slab [K, 6, stride] (columns >= n never read), slots ``k_range`` (default all); ``attr``: the
    [K, stride] attribute row of a VALUES map; ``seeds`` [n, 3]: binned by a COUNT map only."""
    rec = np.asarray(records)
    k0, k1 = (0, rec.shape[0]) if k_range is None else k_range
    if n == 0 or k1 <= k0:
        return accum
    if seeds is not None and kind == COUNT:
        accumulate(accum, np.asarray(seeds)[:n], width, height, lat_range, lon_range)
    pts = rec[k0:k1, 0:3, :n].transpose(0, 2, 1).reshape(-1, 3)
    if kind == COUNT:
        val = None
    elif kind == SPEED:
        val = speed(rec[k0:k1, 3:6, :n].transpose(0, 2, 1).reshape(-1, 3))
    else:
        val = np.asarray(attr)[k0:k1, :n].reshape(-1)
    return accumulate(accum, pts, width, height, lat_range, lon_range, val)


def image(accum, nan_empty=True):
    """mops_density_image: [H, W, 4] float64 {count, mean, sum, 1}."""
    cnt, qs = accum[:, :, 0], accum[:, :, 1]
    img = np.empty(accum.shape[:2] + (4,))
    empty = cnt == 0
    with np.errstate(all="ignore"):
        total = qs.astype(np.float64) / Q_SCALE
        img[:, :, 0] = cnt.astype(np.float64)
        img[:, :, 1] = total / cnt.astype(np.float64)
        img[:, :, 2] = total
    img[:, :, 3] = 1.0
    img[empty, 1] = np.nan
    img[empty, 0] = np.nan if nan_empty else 0.0
    img[empty, 2] = np.nan if nan_empty else 0.0
    return img


def edge_distance(points, width, height, lat_range, lon_range):
    """The smallest distance (in pixels) of a valid point's fr or fc from an integer."""
    valid, fr, fc = pixel_coords(points, width, height, lat_range, lon_range)
    if not valid.any():
        return np.inf
    f = np.concatenate([fr[valid], fc[valid]])
    return float(np.min(np.abs(f - np.rint(f))))


def brute_force(points, width, height, lat_range, lon_range, values=None):
    """The header's rules one point at a time in Python floats (math.asin / math.atan2 are libm's)."""
    acc = [[[0, 0] for _ in range(width)] for _ in range(height)]
    for i, (x, y, z) in enumerate(np.asarray(points, dtype=np.float64).reshape(-1, 3).tolist()):
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            continue
        r = math.sqrt(x * x + y * y + z * z)
        if r == 0.0:
            continue
        lat = math.asin(max(-1.0, min(1.0, z / r))) * RAD2DEG
        lon = math.atan2(y, x) * RAD2DEG
        lon -= 360.0 * math.floor((lon - lon_range[0]) / 360.0)
        fr = (lat_range[1] - lat) / (lat_range[1] - lat_range[0]) * height
        fc = (lon - lon_range[0]) / (lon_range[1] - lon_range[0]) * width
        if not (0.0 <= fr < height and 0.0 <= fc < width):
            continue
        q = 0
        if values is not None:
            v = float(values[i])
            if not math.isfinite(v) or abs(v) >= V_LIMIT:
                continue
            q = round(v * Q_SCALE)  # Python's round: ties to even, exact on the scaled double
        cell = acc[int(math.floor(fr))][int(math.floor(fc))]
        cell[0] += 1
        cell[1] += q
    return np.asarray(acc, dtype=np.int64)
