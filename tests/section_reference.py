"""Restatement of the vertical section (mops_section_points, mops_remap_section, mops_section_transport) in
plain Python floats.

TEST INFRASTRUCTURE ONLY (like remap_reference.py, whose helpers it imports): the product never imports this
module.  The path geometry and the transport quadrature are include/mops_traj.h's expressions in their order
with ``math.sin`` / ``cos`` / ``atan2`` / ``sqrt`` (the host libm the C library calls); the pixel is
remap_reference.fixed_latitude's -- Kernel::VisualizeFixedLatitude, MPASOVisualizerKernels.cpp:545-651 -- at a
given column position, plus the across-section component and the depth-blended attributes.
"""
import math

import numpy as np

import remap_reference as RR
from remap_reference import BAD_CELL, NAN, NO_LAYER, OUT_OF_RANGE, OUTSIDE, VALID, ZERO_DENOM, _Case, enu, is_on_land, \
    wachspress

R = 6371010.0  # the remapping's radius (RR.R_EARTH: 6371010.0f is exact)
assert R == RR.R_EARTH


class Refused(ValueError):
    """What mops_section_points answers with MOPS_ERR_INVALID."""


# ---- path geometry ----------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _len(q):
    return math.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])


def waypoint_unit(lat, lon):
    theta, phi = lat * (math.pi / 180.0), lon * (math.pi / 180.0)
    ct, st, cp, sp = math.cos(theta), math.sin(theta), math.cos(phi), math.sin(phi)
    return (ct * cp, ct * sp, st)


def legs(path):
    """(unit vectors, tangents, angles, cumulative angles) of the polyline; Refused as the entry refuses."""
    path = [(float(a), float(b)) for a, b in path]
    if len(path) < 2:
        raise Refused("fewer than two waypoints")
    for lat, lon in path:
        if not (math.isfinite(lat) and math.isfinite(lon)) or abs(lat) > 90.0:
            raise Refused("invalid waypoint")
    u = [waypoint_unit(lat, lon) for lat, lon in path]
    tg, ang, cum = [], [], [0.0]
    for a, b in zip(u[:-1], u[1:]):
        d = _dot(a, b)
        q = (b[0] - d * a[0], b[1] - d * a[1], b[2] - d * a[2])
        lq = _len(q)
        g = math.atan2(lq, d)
        if not g >= 1e-12:
            raise Refused("a leg of zero length")
        if g > math.pi - 1e-9:
            raise Refused("an antipodal leg")
        tg.append((q[0] / lq, q[1] / lq, q[2] / lq))
        ang.append(g)
        cum.append(cum[-1] + g)
    return u, tg, ang, cum


def section_points(path, width):
    """mops_section_points: (points [W, 3], normals [W, 3], distance [W])."""
    width = int(width)
    u, tg, ang, cum = legs(path)
    if width < 2:
        raise Refused("fewer than two columns")
    n_leg = len(ang)
    total = cum[n_leg]
    pts, nrm, dist = np.empty((width, 3)), np.empty((width, 3)), np.empty(width)
    for j in range(width):
        if j == 0:
            leg, s, phi = 0, 0.0, 0.0
        elif j == width - 1:
            leg, s, phi = n_leg - 1, total, ang[n_leg - 1]
        else:
            s = (float(j) * total) / float(width - 1)
            leg = 0
            while leg < n_leg - 1 and s > cum[leg + 1]:
                leg += 1
            phi = s - cum[leg]
            if phi > ang[leg]:
                phi = ang[leg]
        a, t = u[leg], tg[leg]
        c, sn = math.cos(phi), math.sin(phi)
        p = (c * a[0] + sn * t[0], c * a[1] + sn * t[1], c * a[2] + sn * t[2])
        tau = (c * t[0] - sn * a[0], c * t[1] - sn * a[1], c * t[2] - sn * a[2])
        pts[j] = (R * p[0], R * p[1], R * p[2])
        nrm[j] = (p[1] * tau[2] - p[2] * tau[1], p[2] * tau[0] - p[0] * tau[2], p[0] * tau[1] - p[1] * tau[0])
        dist[j] = R * s
    return pts, nrm, dist


# ---- the pixel --------------------------------------------------------------------------------------------
def section(mesh, derived, positions, normals, height, depth_range, cells, attrs=()):
    """mops_remap_section per pixel.  ``positions`` [W, 3], ``normals`` [W, 3] or None, ``cells`` [W] the 1-NN
    cell of each column, ``attrs`` up to two vertex arrays [V*L] in the mesh's vertex order.  Returns
    dict(images [1 or 2, H, W, 4], code [H, W], layer [H, W])."""
    c = _Case(mesh, derived)
    positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    width = len(positions)
    attrs = [np.asarray(a, dtype=np.float64).reshape(c.V, c.L).tolist() for a in attrs]
    n_attr = len(attrs)
    assert n_attr <= 2
    images = np.zeros((2 if n_attr else 1, height, width, 4))
    code = np.full((height, width), -1, dtype=np.int32)
    layer_map = np.full((height, width), -1, dtype=np.int32)
    minDepth, maxDepth = float(depth_range[0]), float(depth_range[1])
    nVert = c.L
    i_step = (maxDepth - minDepth) / (height - 1) if height > 1 else 0.0
    cells = np.asarray(cells).reshape(-1)
    for jw in range(width):
        position = tuple(float(x) for x in positions[jw])
        normal = None if normals is None else tuple(float(x) for x in normals[jw])

        def nan_column(why):
            code[:, jw] = why
            images[:, :, jw] = (NAN, NAN, NAN, 1.0)

        cell = int(cells[jw])
        if cell < 0 or cell >= c.C:                     # :545
            nan_column(BAD_CELL)
            continue
        n = c.nv[cell]
        ids = c.voc[cell][:n]
        poly = [c.vc[v] for v in ids]
        if n == 0 or is_on_land(poly, position):        # :551-555
            nan_column(OUTSIDE)
            continue
        w = wachspress(position, poly)
        z, _ = c.column(ids, w)
        EPSILON = 1e-6
        for ih in range(height):
            def nan_pixel(why):
                code[ih, jw] = why
                images[:, ih, jw] = (NAN, NAN, NAN, 1.0)

            depth_plot = minDepth + ih * i_step
            DEPTH = -abs(depth_plot)
            if DEPTH > z[0] + EPSILON or DEPTH < z[nVert - 1] - EPSILON:  # :592
                nan_pixel(OUT_OF_RANGE)
                continue
            layer = -1
            for k in range(1, nVert):                   # :597-607
                z_up, z_dn = z[k - 1], z[k]
                if z_up < z_dn:
                    z_up, z_dn = z_dn, z_up
                if DEPTH <= z_up + EPSILON and DEPTH >= z_dn - EPSILON:
                    layer = k
                    break
            if layer == -1:                             # :609
                nan_pixel(NO_LAYER)
                continue
            dn, up = z[layer], z[layer - 1]
            if up < dn:
                up, dn = dn, up
            denom = up - dn
            if abs(denom) < 1e-30:                      # :621
                nan_pixel(ZERO_DENOM)
                continue
            t = (DEPTH - dn) / denom
            vel_up = c.velocity(ids, w, layer - 1)
            vel_dn = c.velocity(ids, w, layer)
            cc = 1.0 - t
            f = (cc * vel_dn[0] + t * vel_up[0], cc * vel_dn[1] + t * vel_up[1], cc * vel_dn[2] + t * vel_up[2])
            zonal, meridional = enu(position, f)
            across = 0.0 if normal is None else (f[0] * normal[0] + f[1] * normal[1]) + f[2] * normal[2]
            images[0, ih, jw] = (zonal, meridional, across, 1.0)
            if n_attr:
                vals = [0.0, 0.0]
                for q, arr in enumerate(attrs):
                    up_a = dn_a = 0.0
                    for v, vid in enumerate(ids):
                        up_a += w[v] * arr[vid][layer - 1]
                    for v, vid in enumerate(ids):
                        dn_a += w[v] * arr[vid][layer]
                    vals[q] = cc * dn_a + t * up_a
                images[1, ih, jw] = (vals[0], vals[1], 0.0, 1.0)
            code[ih, jw] = VALID
            layer_map[ih, jw] = layer
    return dict(images=images, code=code, layer=layer_map)


# ---- transport --------------------------------------------------------------------------------------------
def transport(image, distance, depth_range):
    """mops_section_transport: (Sverdrups, valid area)."""
    image = np.asarray(image, dtype=np.float64)
    H, W = image.shape[:2]
    d = [float(x) for x in distance]
    ds = [0.5 * (d[min(j + 1, W - 1)] - d[max(j - 1, 0)]) for j in range(W)]
    dz = (float(depth_range[1]) - float(depth_range[0])) / (H - 1)
    total = area = 0.0
    for i in range(H):
        dzi = 0.5 * dz if i in (0, H - 1) else dz
        for j in range(W):
            across = float(image[i, j, 2])
            if across != across:
                continue
            total += (across * ds[j]) * dzi
            area += ds[j] * dzi
    return total / 1.0e6, area
