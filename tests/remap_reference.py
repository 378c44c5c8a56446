"""Per-pixel restatement of the reference's two image remapping functions in plain Python floats.

TEST INFRASTRUCTURE ONLY (like oracle/): the product never imports this module.  Every expression is the
reference's, in its order, on IEEE doubles (Python floats; ``math.sqrt`` is correctly rounded, ``math.sin`` /
``math.cos`` are the host libm's, which the reference calls too).  Line numbers are in the reference's ``src/``:

* ``fixed_depth``     Kernel::VisualizeFixedDepth, CPU/TBB/Kernel/MPASOVisualizerKernels.cpp:238-471
* ``fixed_latitude``  Kernel::VisualizeFixedLatitude, same file :473-651
* pixel positions     Utils/GeoConverter.hpp:28-32 and :118-124
* helpers             CPU/TBB/Kernel/TBBKernel.h:21-54,128-166, Utils/Interpolation.hpp:95-165,
                      Core/MPASOField.cpp:36-81, Utils/GeoConverter.hpp:200-223

Outcome codes (per pixel, for the tests' coverage assertions): VALID, OUTSIDE (the inside test failed),
OUT_OF_RANGE (the depth range test failed), NO_LAYER (the layer search found none), BAD_CELL, ZERO_DENOM.
"""
import math

import numpy as np

VALID, OUTSIDE, OUT_OF_RANGE, NO_LAYER, BAD_CELL, ZERO_DENOM = 0, 1, 2, 3, 4, 5
R_EARTH = float(np.float32(6371010.0))  # `double r = 6371010.0f` (GeoConverter.hpp:107)
NAN = float("nan")


# ---- pixel positions --------------------------------------------------------------------------------------
def pixel_latlon(width, height, lat_range, lon_range, i, j):
    """GeoConverter::convertPixelToLatLonToRadians (:28-32): pixel (row i, column j) -> (lat, lon) radians."""
    min_lat, max_lat = lat_range
    min_lon, max_lon = lon_range
    lat = max_lat - (float(i) / float(height) * (max_lat - min_lat))
    lon = (float(j) / float(width) * (max_lon - min_lon)) + min_lon
    return lat * (math.pi / 180.0), lon * (math.pi / 180.0)


def latlon_to_xyz(theta, phi):
    """GeoConverter::convertRadianLatLonToXYZ (:118-124)."""
    r = R_EARTH
    costheta, cosphi = math.cos(theta), math.cos(phi)
    sintheta, sinphi = math.sin(theta), math.sin(phi)
    return (r * costheta * cosphi, r * costheta * sinphi, r * sintheta)


def depth_positions(width, height, lat_range, lon_range):
    """TBBKernel::SearchKDTree's positions (TBBKernel.cpp:15-28), row-major [height*width, 3]."""
    pts = np.empty((height * width, 3))
    for i in range(height):
        for j in range(width):
            pts[i * width + j] = latlon_to_xyz(*pixel_latlon(width, height, lat_range, lon_range, i, j))
    return pts


def latitude_positions(width, lon_range, fixed_lat):
    """VisualizeFixedLatitude's positions (:513-523), one per column [width, 3]."""
    min_lon, max_lon = lon_range
    j_step = (max_lon - min_lon) / (width - 1) if width > 1 else 0.0
    pts = np.empty((width, 3))
    for jw in range(width):
        lon = min_lon + jw * j_step
        pts[jw] = latlon_to_xyz(fixed_lat * (math.pi / 180.0), lon * (math.pi / 180.0))
    return pts


# ---- helpers ----------------------------------------------------------------------------------------------
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _length(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def is_in_mesh(poly, p):
    """TBBKernel::IsInMesh (TBBKernel.h:21-54) on the cell's vertex positions."""
    if not (math.isfinite(p[0]) and math.isfinite(p[1]) and math.isfinite(p[2])):
        return False
    n = len(poly)
    if n == 0:
        return False
    for k in range(n):
        if _dot(_cross(poly[k], poly[(k + 1) % n]), p) < 0.0:
            return False
    return True


def is_on_land(poly, p):
    """MPASOField::isOnOcean's return value is_land (MPASOField.cpp:36-81): sign consistency of
    dot(cross(O - A, O - B), p - A) over the cell's edges."""
    n = len(poly)
    dirs = []
    for k in range(n):
        A, B = poly[k], poly[(k + 1) % n]
        AO = (0.0 - A[0], 0.0 - A[1], 0.0 - A[2])
        BO = (0.0 - B[0], 0.0 - B[1], 0.0 - B[2])
        A_point = (p[0] - A[0], p[1] - A[1], p[2] - A[2])
        dirs.append(_dot(_cross(AO, BO), A_point))
    sign = 1.0 if dirs[0] > 0 else -1.0
    for d in dirs:
        if (1.0 if d > 0 else -1.0) != sign:
            return True
    return False


def triangle_area(a, b, c):
    """Interpolator::triangle_area (Interpolation.hpp:95-110)."""
    e1 = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
    e2 = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
    cp = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
    return math.sqrt(cp[0] * cp[0] + cp[1] * cp[1] + cp[2] * cp[2]) / 2.0


def _div(a, b):
    """IEEE double division (Python raises on a zero divisor)."""
    return float(np.float64(a) / np.float64(b))


def wachspress(p, poly):
    """Interpolator::CalcPolygonWachspress (Interpolation.hpp:137-165)."""
    N = len(poly)
    w = [0.0] * N
    sumweights = 0.0
    A_iplus1 = triangle_area(poly[N - 1], poly[0], p)
    with np.errstate(all="ignore"):
        for i in range(N):
            A_i = A_iplus1
            A_iplus1 = triangle_area(poly[i], poly[(i + 1) % N], p)
            B = triangle_area(poly[(i - 1 + N) % N], poly[i], poly[(i + 1) % N])
            w[i] = _div(B, A_i * A_iplus1)
            sumweights += w[i]
        recp = _div(1.0, sumweights)
    return [x * recp for x in w]


def enu(p, v):
    """GeoConverter::convertXYZVelocityToENU (GeoConverter.hpp:200-223)."""
    if p[0] == 0.0 and p[1] == 0.0:
        return 0.0, 0.0
    Rxy = math.sqrt(p[0] * p[0] + p[1] * p[1])
    Rxyz = math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    slon = p[1] / Rxy
    clon = p[0] / Rxy
    slat = p[2] / Rxyz
    clat = Rxy / Rxyz
    Uzon = -slon * v[0] + clon * v[1]
    Umer = -slat * (clon * v[0] + slon * v[1]) + clat * v[2]
    return Uzon, Umer


class _Case:
    """Plain-list views of a synth.Mesh and its derived vertex fields."""

    def __init__(self, mesh, derived):
        self.C, self.V, self.L, me = mesh.nCells, mesh.nVertices, mesh.nVertLevels, mesh.maxEdges
        self.nv = [int(x) for x in mesh.nEdgesOnCell]
        self.voc = (np.asarray(mesh.verticesOnCell).reshape(-1, me).astype(np.int64) - 1).tolist()
        self.vc = [tuple(r) for r in np.asarray(mesh.vertexCoord, dtype=np.float64).reshape(-1, 3).tolist()]
        self.zt = np.asarray(derived.vertex_ztop, dtype=np.float64).reshape(self.V, self.L).tolist()
        self.vel = np.asarray(derived.vertex_vel, dtype=np.float64).reshape(self.V, self.L, 3).tolist()

    def column(self, ids, w):
        """The weighted zTop column and the monotone clamp (:346-360 / :573-587); (z, clamped?)."""
        z = []
        for k in range(self.L):
            acc = 0.0
            for v, vid in enumerate(ids):
                acc += w[v] * self.zt[vid][k]
            z.append(acc)
        clamped = False
        for k in range(1, self.L):
            if z[k] > z[k - 1]:
                z[k] = z[k - 1] - 1e-9
                clamped = True
        return z, clamped

    def velocity(self, ids, w, layer):
        """TBBKernel::CalcVelocity (TBBKernel.h:128-147)."""
        x = y = z = 0.0
        for v, vid in enumerate(ids):
            vel = self.vel[vid][layer]
            x += w[v] * vel[0]
            y += w[v] * vel[1]
            z += w[v] * vel[2]
        return (x, y, z)


def fixed_depth(mesh, derived, width, height, lat_range, lon_range, depth, cells, layer_rule="reference",
                positions=None):
    """VisualizeFixedDepth over MOPSApp::runRemapping's images (MOPSApp.cpp:171-196).

    ``derived``: oracle.preprocess(...) (its ``attrs`` decide the image count and feed image 1); ``cells``: the
    1-NN cell of every pixel, row-major.  Returns dict(images [n, H, W, 4], code [H, W], layer [H, W] (-1 where
    not valid), clamped [H, W] bool, branch [H, W]: 0 both tiny, 1 top tiny, 2 bottom tiny, 3 blend, -1 n/a)."""
    c = _Case(mesh, derived)
    names = sorted(derived.attrs)                       # std::map order
    n_attr = len(names)
    n_img = 1 + (n_attr + 2) // 3 if n_attr > 0 else 1  # MOPSApp.cpp:176-185
    two = n_attr > 1                                    # bDoubleAttributes (:261)
    attrs = [np.asarray(derived.attrs[k], dtype=np.float64).reshape(c.V, c.L).tolist() for k in names[:2]] if two \
        else []
    images = np.zeros((n_img, height, width, 4))
    code = np.full((height, width), -1, dtype=np.int32)
    layer = np.full((height, width), -1, dtype=np.int32)
    clamped = np.zeros((height, width), dtype=bool)
    branch = np.full((height, width), -1, dtype=np.int32)
    DEPTH = -float(depth)                               # :251
    cells = np.asarray(cells).reshape(-1)
    L = c.L

    def set_pixel(k, i, j, val):                        # SetPixel: alpha 1.0
        images[k, i, j] = (val[0], val[1], val[2], 1.0)

    for g in range(width * height):
        i, j = g // width, g % width
        if positions is None:
            p = latlon_to_xyz(*pixel_latlon(width, height, lat_range, lon_range, i, j))
        else:
            p = tuple(float(x) for x in positions[g])

        def nan_pixel(why):
            code[i, j] = why
            set_pixel(0, i, j, (NAN, NAN, NAN))
            if two:
                set_pixel(1, i, j, (NAN, NAN, NAN))

        cell = int(cells[g])
        if cell < 0 or cell >= c.C:                     # :299
            nan_pixel(BAD_CELL)
            continue
        n = c.nv[cell]
        ids = c.voc[cell][:n]
        poly = [c.vc[v] for v in ids]
        if not is_in_mesh(poly, p):                     # :312
            nan_pixel(OUTSIDE)
            continue
        w = wachspress(p, poly)                         # :335
        if L <= 0 or L > 100:                           # :338
            nan_pixel(OUT_OF_RANGE)
            continue
        z, cl = c.column(ids, w)                        # :346-360
        z_surf, z_bot = z[0], z[L - 1]
        if z_surf < z_bot:
            z_surf, z_bot = z_bot, z_surf
        epsd = max(1e-6, 1e-8 * abs(z_surf - z_bot))
        if not (DEPTH <= z_surf + epsd and DEPTH >= z_bot - epsd):  # :370
            nan_pixel(OUT_OF_RANGE)
            continue
        local_layer = -1
        for k in range(1, L):                           # :379-391
            topI, botI = z[k - 1], z[k]
            if topI < botI:
                topI, botI = botI, topI
            if DEPTH <= topI + 1e-8 and DEPTH >= botI - 1e-8:
                local_layer = k
                break
        if layer_rule == "reference":                   # :392-394, left out by "bracket"
            if DEPTH <= z[0]:
                local_layer = 0
        if local_layer < 0:                             # :395
            nan_pixel(NO_LAYER)
            continue
        topI, botI = z[max(0, local_layer - 1)], z[local_layer]
        if topI < botI:
            topI, botI = botI, topI
        denom = topI - botI
        tparam = (DEPTH - botI) / denom if denom > 1e-12 else 0.5
        jj = min(max(local_layer - 1, 0), L - 1)
        j_bot = min(jj + 1, L - 1)
        j_top = jj
        v_top = c.velocity(ids, w, j_top)
        v_bot = c.velocity(ids, w, j_bot)
        mtop, mbot = _length(v_top), _length(v_bot)
        if mtop < 1e-12 and mbot < 1e-12:
            final, br = (0.0, 0.0, 0.0), 0
        elif mtop < 1e-12:
            final, br = v_bot, 1
        elif mbot < 1e-12:
            final, br = v_top, 2
        else:
            cc = 1.0 - tparam
            final = (cc * v_bot[0] + tparam * v_top[0], cc * v_bot[1] + tparam * v_top[1],
                     cc * v_bot[2] + tparam * v_top[2])
            br = 3
        u_east, v_north = enu(p, final)
        spd = math.sqrt(u_east * u_east + v_north * v_north)
        set_pixel(0, i, j, (u_east, v_north, spd))
        if two:                                         # :443-469
            a = []
            for arr in attrs:
                r = 0.0
                for v, vid in enumerate(ids):
                    r += w[v] * arr[vid][jj]
                a.append(r)
            set_pixel(1, i, j, (a[0], a[1], 0.0))
        code[i, j] = VALID
        layer[i, j] = local_layer
        clamped[i, j] = cl
        branch[i, j] = br
    return dict(images=images, code=code, layer=layer, clamped=clamped, branch=branch)


def fixed_latitude(mesh, derived, width, height, lon_range, fixed_lat, depth_range, cells):
    """VisualizeFixedLatitude (:473-651).  ``depth_range``: (refBottomDepth.front(), .back()); ``cells``: the
    1-NN cell of every column [width].  Returns dict(image [H, W, 4], code [H, W], layer [H, W])."""
    c = _Case(mesh, derived)
    image = np.zeros((height, width, 4))
    code = np.full((height, width), -1, dtype=np.int32)
    layer_map = np.full((height, width), -1, dtype=np.int32)
    minDepth, maxDepth = float(depth_range[0]), float(depth_range[1])
    min_lon, max_lon = lon_range
    nVert = c.L
    i_step = (maxDepth - minDepth) / (height - 1) if height > 1 else 0.0
    j_step = (max_lon - min_lon) / (width - 1) if width > 1 else 0.0
    cells = np.asarray(cells).reshape(-1)
    for gid in range(width * height):
        ih, jw = gid // width, gid % width

        def nan_pixel(why):
            code[ih, jw] = why
            image[ih, jw] = (NAN, NAN, NAN, 1.0)

        depth_plot = minDepth + ih * i_step
        DEPTH = -abs(depth_plot)
        lon = min_lon + jw * j_step
        position = latlon_to_xyz(fixed_lat * (math.pi / 180.0), lon * (math.pi / 180.0))
        cell = int(cells[jw])
        if cell < 0 or cell >= c.C:                     # :545
            nan_pixel(BAD_CELL)
            continue
        n = c.nv[cell]
        ids = c.voc[cell][:n]
        poly = [c.vc[v] for v in ids]
        if is_on_land(poly, position) or n == 0:        # :551-555
            nan_pixel(OUTSIDE)
            continue
        w = wachspress(position, poly)
        z, _ = c.column(ids, w)
        EPSILON = 1e-6
        if DEPTH > z[0] + EPSILON or DEPTH < z[nVert - 1] - EPSILON:  # :592
            nan_pixel(OUT_OF_RANGE)
            continue
        layer = -1
        for k in range(1, nVert):                       # :597-607
            z_up, z_dn = z[k - 1], z[k]
            if z_up < z_dn:
                z_up, z_dn = z_dn, z_up
            if DEPTH <= z_up + EPSILON and DEPTH >= z_dn - EPSILON:
                layer = k
                break
        if layer == -1:                                 # :609
            nan_pixel(NO_LAYER)
            continue
        dn, up = z[layer], z[layer - 1]
        if up < dn:
            up, dn = dn, up
        denom = up - dn
        if abs(denom) < 1e-30:                          # :621
            nan_pixel(ZERO_DENOM)
            continue
        t = (DEPTH - dn) / denom
        vel_up = c.velocity(ids, w, layer - 1)
        vel_dn = c.velocity(ids, w, layer)
        cc = 1.0 - t
        final = (cc * vel_dn[0] + t * vel_up[0], cc * vel_dn[1] + t * vel_up[1], cc * vel_dn[2] + t * vel_up[2])
        zonal, meridional = enu(position, final)
        image[ih, jw] = (zonal, meridional, 0.0, 1.0)
        code[ih, jw] = VALID
        layer_map[ih, jw] = layer
    return dict(image=image, code=code, layer=layer_map)
