"""Restatements of the reference's image colouring and fixed-layer remapping, and minimal readers for the two
image file formats the engine writes.

TEST INFRASTRUCTURE ONLY (like oracle/ and remap_reference.py): the product never imports this module.
Line numbers are in the reference's ``src/``:

* ``save_to_png_rgba``  MOPS::SaveToPNG, Common/ImageBuffer.hpp:91-136, with tinycolormap's CalcLerp
                        (Utils/tinycolormap.hpp:162-171): float32 for min / max / norm, float64 for the lerp and
                        the truncation to bytes.  numpy evaluates every operation separately (no FMA contraction).
* ``fixed_layer``       Kernel::VisualizeFixedLayer, CPU/TBB/Kernel/MPASOVisualizerKernels.cpp:141-236, on the
                        helpers of remap_reference.py.
* ``decode_png``        PNG (ISO/IEC 15948): 8-bit RGBA, non-interlaced, all five filter types, CRCs verified.
* ``read_vti``          the VTK XML ImageData layout of mops_write_images_vti / mops_write_image_vti.

The Viridis table is parsed from include/mops_viridis.h (generated from matplotlib's published samples).
"""
import os
import re
import struct
import zlib

import numpy as np

import remap_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max


def viridis_table():
    """The 256 x 3 float64 table of include/mops_viridis.h."""
    src = open(os.path.join(ROOT, "include", "mops_viridis.h")).read()
    rows = re.findall(r"^\s*\{([^{}]+)\},?\s*$", src, flags=re.M)
    t = np.array([[float(v) for v in r.split(",")] for r in rows], dtype=np.float64)
    assert t.shape == (256, 3), t.shape
    return t


_TABLE = None


def save_to_png_rgba(channel):
    """SaveToPNG's pixels for one channel [H, W] float64 -> (rgba [H, W, 4] uint8, (min, max) float32)."""
    global _TABLE
    if _TABLE is None:
        _TABLE = viridis_table()
    T = _TABLE
    ch = np.asarray(channel, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = ch.astype(np.float32)                       # :105 static_cast<float>
        ok = ~np.isnan(f)                               # :106
        mn, mx = np.float32(FLT_MAX), np.float32(-FLT_MAX)  # :101-102
        if ok.any():
            mn = np.float32(min(mn, f[ok].min()))       # :107-108
            mx = np.float32(max(mx, f[ok].max()))
        if mn >= mx:                                    # :111
            mx = np.float32(mn + np.float32(1e-5))
        norm = (f - mn) / np.float32(mx - mn)           # :125, float32 throughout
        assert norm.dtype == np.float32
        x = norm.astype(np.float64)                     # GetColor(double x)
        cl = np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))  # Clamp01 (tinycolormap.hpp:155-158)
        cl = np.where(np.isnan(cl), 0.0, cl)            # undefined in the reference; the engine: entry 0
        a = cl * 255.0                                  # :165  (N - 1 = 255)
        i = np.floor(a)
        t = a - i
        i0 = i.astype(np.int64)
        i1 = np.ceil(a).astype(np.int64)
        c = (1.0 - t)[..., None] * T[i0] + t[..., None] * T[i1]  # :171
        rgb = (c * 255.0).astype(np.uint8)              # :127-129: truncation
    rgba = np.zeros(ch.shape + (4,), dtype=np.uint8)
    rgba[..., :3] = rgb
    rgba[..., 3] = 255
    rgba[~ok] = 0                                       # :118-123
    return rgba, (mn, mx)


# ---- fixed layer ------------------------------------------------------------------------------------------
def clamp_layer(layer, total_layers):
    """ClampLayer (:14-26) of the double FixedLayer converted to int (:166, truncation toward zero)."""
    layer = int(layer)
    if total_layers <= 0 or layer < 0:
        return 0
    return total_layers - 1 if layer >= total_layers else layer


def fixed_layer(mesh, derived, width, height, lat_range, lon_range, layer, cells):
    """VisualizeFixedLayer (:141-236).  ``cells``: the 1-NN cell of every pixel, row-major.  Returns
    dict(image [H, W, 4], code [H, W]: RR.VALID / RR.OUTSIDE / RR.BAD_CELL, layer: the clamped layer)."""
    c = RR._Case(mesh, derived)
    image = np.zeros((height, width, 4))
    code = np.full((height, width), -1, dtype=np.int32)
    total_layers = max(1, c.L)                          # :165
    fl = clamp_layer(layer, total_layers)               # :166
    cells = np.asarray(cells).reshape(-1)
    for g in range(width * height):
        i, j = g // width, g % width
        p = RR.latlon_to_xyz(*RR.pixel_latlon(width, height, lat_range, lon_range, i, j))  # :184-188
        cell = int(cells[g])
        if cell < 0 or cell >= c.C:                     # :191
            image[i, j] = (RR.NAN, RR.NAN, RR.NAN, 1.0)
            code[i, j] = RR.BAD_CELL
            continue
        n = c.nv[cell]
        if n <= 0 or n > 20:                            # :197
            image[i, j] = (RR.NAN, RR.NAN, RR.NAN, 1.0)
            code[i, j] = RR.BAD_CELL
            continue
        ids = c.voc[cell][:n]
        poly = [c.vc[v] for v in ids]
        if not RR.is_in_mesh(poly, p):                  # :206
            image[i, j] = (RR.NAN, RR.NAN, RR.NAN, 1.0)
            code[i, j] = RR.OUTSIDE
            continue
        w = RR.wachspress(p, poly)                      # :219
        vel = c.velocity(ids, w, fl)                    # :222-228 CalcVelocity
        zonal, meridional = RR.enu(p, vel)              # :232
        image[i, j] = (zonal, meridional, 0.0, 1.0)     # :234
        code[i, j] = RR.VALID
    return dict(image=image, code=code, layer=fl)


# ---- PNG --------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def decode_png(data):
    """An 8-bit RGBA non-interlaced PNG (bytes or a path) -> [H, W, 4] uint8.  Every chunk's CRC is checked."""
    if not isinstance(data, (bytes, bytearray)):
        with open(data, "rb") as f:
            data = f.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    pos, idat, ihdr, ended = 8, [], None, False
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert zlib.crc32(typ + body) & 0xFFFFFFFF == crc, f"bad CRC in {typ!r}"
        pos += 12 + n
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat.append(body)
        elif typ == b"IEND":
            ended = True
            break
    assert ihdr is not None and ended and pos == len(data)
    w, h, depth, ctype, comp, filt, interlace = ihdr
    assert (depth, ctype, comp, filt, interlace) == (8, 6, 0, 0, 0), ihdr
    raw = zlib.decompress(b"".join(idat))
    stride, bpp = w * 4, 4
    assert len(raw) == h * (1 + stride)
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.int64)
    for r in range(h):
        ft = raw[r * (1 + stride)]
        line = np.frombuffer(raw, dtype=np.uint8, count=stride, offset=r * (1 + stride) + 1).astype(np.int64)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):  # serial in x: Sub, Average, Paeth
            cur = np.zeros(stride, dtype=np.int64)
            lst, pv = line.tolist(), prev.tolist()
            res = [0] * stride
            for k in range(stride):
                a = res[k - bpp] if k >= bpp else 0
                b = pv[k]
                cc = pv[k - bpp] if k >= bpp else 0
                pred = a if ft == 1 else ((a + b) >> 1 if ft == 3 else _paeth(a, b, cc))
                res[k] = (lst[k] + pred) & 255
            cur = np.array(res, dtype=np.int64)
        else:
            raise AssertionError(f"bad filter type {ft}")
        out[r] = cur
        prev = cur
    return out.reshape(h, w, 4)


# ---- VTI --------------------------------------------------------------------------------------------------
def read_vti(path):
    """dict(extent (6 ints), origin, spacing (3 floats), arrays: [(name, n_components, float64 [H, W(, 3)])],
    scalars: the PointData Scalars attribute or None) of an appended-raw VTK XML ImageData file with UInt64 block
    headers.  Rows are the file's (VTK's) rows: no flip is undone."""
    with open(path, "rb") as f:
        data = f.read()
    mark = data.index(b"<AppendedData encoding=\"raw\">")
    start = data.index(b"_", mark) + 1
    head = data[:mark].decode()
    assert 'type="ImageData"' in head and 'byte_order="LittleEndian"' in head and 'header_type="UInt64"' in head
    m = re.search(r'<ImageData WholeExtent="([^"]*)" Origin="([^"]*)" Spacing="([^"]*)"', head)
    extent = [int(v) for v in m.group(1).split()]
    origin = [float(v) for v in m.group(2).split()]
    spacing = [float(v) for v in m.group(3).split()]
    assert re.search(r'<Piece Extent="([^"]*)"', head).group(1) == m.group(1)
    w, h = extent[1] - extent[0] + 1, extent[3] - extent[2] + 1
    sc = re.search(r'<PointData Scalars="([^"]*)"', head)
    arrays = []
    for tag in re.findall(r"<DataArray ([^>]*)/>", head):
        at = dict(re.findall(r'(\w+)="([^"]*)"', tag))
        assert at["type"] == "Float64" and at["format"] == "appended"
        nc = int(at.get("NumberOfComponents", "1"))
        off = start + int(at["offset"])
        (nbytes,) = struct.unpack("<Q", data[off:off + 8])
        assert nbytes == w * h * nc * 8
        a = np.frombuffer(data, dtype="<f8", count=w * h * nc, offset=off + 8)
        name = at["Name"].replace("&lt;", "<").replace("&gt;", ">").replace("&quot;", '"').replace("&amp;", "&")
        arrays.append((name, nc, a.reshape((h, w) if nc == 1 else (h, w, nc)).copy()))
    assert data[start + sum(8 + a.size * 8 for _, _, a in arrays):].strip().startswith(b"</AppendedData>")
    return dict(extent=extent, origin=origin, spacing=spacing, arrays=arrays, scalars=sc.group(1) if sc else None)
