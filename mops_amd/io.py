"""Trajectory and image output formats (include/mops_io.h), Python side.

Images are [H, W, 4] float64 (``engine.remap_*``): ``save_image_png`` colours one channel on the GPU and
writes the RGBA bytes as a PNG, ``save_images_vti`` / ``save_image_vti`` store the doubles as VTK ImageData.

``lines`` is the dict the engine returns (``run_trajectories``,
``ParticleSet.finalize``, ``PathlineChain.run``): points/velocity [n, P, 3],
temperature/salinity [n, P], as numpy arrays or device tensors.  The
xyz -> (lat, lon, r, |v|) conversion runs on the GPU (``lines_geo``); the
writers stream to disk in native code.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _host(a):
    if a is None:
        return None
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def lines_geo(points, velocity=None, stream=None):
    """Device {lat_deg, lon_deg, r, |v|} per point (mops_lines_geo) -> torch [n, P, 4]."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    p = torch.as_tensor(points, dtype=torch.float64, device=dev).contiguous()
    v = None if velocity is None else torch.as_tensor(velocity, dtype=torch.float64, device=dev).contiguous()
    n, P = int(p.shape[0]), int(p.shape[1])
    out = torch.empty((n, P, 4), dtype=torch.float64, device=dev)
    h = C.c_void_p(0 if stream is None else int(getattr(stream, "cuda_stream", stream)))
    L.check(L.load().mops_lines_geo(n, P, C.c_void_p(p.data_ptr()), None if v is None else C.c_void_p(v.data_ptr()),
                                    C.c_void_p(out.data_ptr()), h), "mops_lines_geo")
    return out


def save_trajectory_lines_vtp(path: str, lines: dict, binary: bool = True, geo=None):
    """VTKFileManager::SaveTrajectoryLinesAsVTP (VTKFileManager.hpp:315-417)."""
    pts = lines["points"]
    n, P = int(pts.shape[0]), int(pts.shape[1])
    g = _host(geo if geo is not None else lines_geo(pts, lines.get("velocity")))
    t, s = _host(lines.get("temperature")), _host(lines.get("salinity"))
    L.check(L.load().mops_write_lines_vtp(path.encode(), n, P, _ptr(g), _ptr(t), _ptr(s), 1 if binary else 0),
            "mops_write_lines_vtp")


def save_trajectory_lines_txt(path: str, lines: dict):
    """The CLI's text dump (CLI/main.cpp:239-262)."""
    p, v = _host(lines["points"]), _host(lines["velocity"])
    L.check(L.load().mops_write_lines_txt(path.encode(), p.shape[0], p.shape[1], _ptr(p), _ptr(v)),
            "mops_write_lines_txt")


def export_pathlines_to_binary(lines: dict, path: str, include_velocity: bool = False,
                               include_scalars: bool = False, geo=None):
    """tutorial/export_pathline_binary.py:export_pathlines_to_binary (+ .meta.json)."""
    pts = lines["points"]
    n, P = int(pts.shape[0]), int(pts.shape[1])
    g = _host(geo if geo is not None else lines_geo(pts, lines.get("velocity")))
    v = _host(lines.get("velocity")) if include_velocity else None
    t = _host(lines.get("temperature")) if include_scalars else None
    s = _host(lines.get("salinity")) if include_scalars else None
    L.check(L.load().mops_write_pathline_binary(path.encode(), n, P, _ptr(g), _ptr(v), _ptr(t), _ptr(s),
                                                int(include_velocity), int(include_scalars)),
            "mops_write_pathline_binary")


# ---- images ------------------------------------------------------------------------------------------------

def write_png_rgba8(path: str, rgba):
    """An [H, W, 4] uint8 array (numpy or tensor) as an 8-bit RGBA PNG (mops_write_png_rgba8)."""
    if hasattr(rgba, "detach"):
        rgba = rgba.detach().cpu().numpy()
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("write_png_rgba8: expected an [H, W, 4] uint8 array")
    L.check(L.load().mops_write_png_rgba8(str(path).encode(), a.shape[1], a.shape[0], _ptr(a)),
            "mops_write_png_rgba8")


def save_image_png(path: str, image, channel: int = 3):
    """MOPS::SaveToPNG (ImageBuffer.hpp:91-136): channel ``channel`` of an [H, W, 4] float64 image through
    the Viridis map into a PNG.  A CUDA tensor is coloured where it lies and only its RGBA bytes come to the
    host; a numpy array goes through the engine's host entry (upload, same kernels).  False where the
    reference returns false (a channel outside 0..3, an empty image)."""
    channel = int(channel)
    if channel < 0 or channel > 3:
        return False
    if hasattr(image, "is_cuda") and image.is_cuda:
        from . import engine
        if image.numel() == 0:
            return False
        rgba = engine.colormap_rgba(image.contiguous(), channels=(channel,))[0].cpu().numpy()
    else:
        img = _host(image)
        if img.ndim != 3 or img.shape[2] != 4:
            raise ValueError("save_image_png: expected an [H, W, 4] image")
        if img.size == 0:
            return False
        rgba = np.empty(img.shape, dtype=np.uint8)
        L.check(L.load().mops_colormap_image(_ptr(img), img.shape[1], img.shape[0], 1 << channel, _ptr(rgba), None,
                                             None), "mops_colormap_image")
    write_png_rgba8(path, rgba)
    return True


def _vec3(v, name):
    a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    if a.size != 3:
        raise ValueError(f"{name}: expected 3 values")
    return a


def save_images_vti(path: str, images, origin, spacing, names=()):
    """VTKFileManager::SaveVTI, image-list overload (VTKFileManager.hpp:80-138), to ``path`` as given:
    ``images`` [n, H, W, 4] (or a list of [H, W, 4]) -> 3 n one-component Float64 arrays, named from ``names``
    then "attr_<i>"; VTK row i is image row H - 1 - i (mops_write_images_vti)."""
    if isinstance(images, (list, tuple)):
        images = np.stack([_host(a) for a in images])
    img = _host(images)
    if img.ndim != 4 or img.shape[3] != 4 or img.size == 0:
        raise ValueError("save_images_vti: expected images [n, H, W, 4]")
    o, s = _vec3(origin, "origin"), _vec3(spacing, "spacing")
    enc = [str(n).encode() for n in names]
    arr = (C.c_char_p * len(enc))(*enc) if enc else None
    L.check(L.load().mops_write_images_vti(str(path).encode(), img.shape[0], img.shape[2], img.shape[1], _ptr(img),
                                           _ptr(o), _ptr(s), arr, len(enc)), "mops_write_images_vti")


def save_image_vti(path: str, image, origin, spacing):
    """VTKFileManager::SaveVTI, single-image overload (:25-78): one 3-component array "ImageScalars"."""
    img = _host(image)
    if img.ndim != 3 or img.shape[2] != 4 or img.size == 0:
        raise ValueError("save_image_vti: expected an image [H, W, 4]")
    o, s = _vec3(origin, "origin"), _vec3(spacing, "spacing")
    L.check(L.load().mops_write_image_vti(str(path).encode(), img.shape[1], img.shape[0], _ptr(img), _ptr(o),
                                          _ptr(s)), "mops_write_image_vti")
