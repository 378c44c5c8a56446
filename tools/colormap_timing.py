"""Times the colour pass on one 3601 x 1801 remapped image (profiles/r10/).

    python tools/colormap_timing.py [out.json]
    rocprofv3 --kernel-trace --stats -- python tools/colormap_timing.py      (per-kernel times)

Host-clock times of engine.colormap_rgba (three planes, one plane; 3 warm-up + 10 timed calls, each
synchronised), of the device-to-host copies of the RGBA planes and of the double image, of one stored-block PNG
write, and of the numpy restatement (tests/image_reference.py) of the same three channels on the host.
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_reference as IR  # noqa: E402
from mops_amd import engine, io as mio, synth  # noqa: E402


def _median(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}


def main():
    torch.cuda.set_device(0)
    mesh = synth.make_mesh(16, n_levels=10)
    dm = engine.DeviceMesh.from_mesh(mesh)
    df = engine.DeviceField.from_snapshot(dm, synth.make_snapshot(mesh))
    W, H = 3601, 1801
    img = engine.remap_fixed_depth(dm, df, W, H, (-90.0, 90.0), (-180.0, 180.0), 800.0)[0]
    res = {"width": W, "height": H, "nan_fraction": float(torch.isnan(img[..., 0]).float().mean())}
    for name, ch in (("three_channels", (0, 1, 2)), ("one_channel", (0,))):
        ts = []
        for _ in range(13):
            torch.cuda.synchronize()
            t = time.perf_counter()
            engine.colormap_rgba(img, channels=ch)
            ts.append((time.perf_counter() - t) * 1e3)
        res[name + "_call_ms"] = _median(ts[3:])
    out = engine.colormap_rgba(img, channels=(0, 1, 2))
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        host = out.cpu()
        ts.append((time.perf_counter() - t) * 1e3)
    res["d2h_three_planes_ms"] = _median(ts)["median"]
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        hd = img.cpu()
        ts.append((time.perf_counter() - t) * 1e3)
    res["d2h_one_double_image_ms"] = _median(ts)["median"]
    hn, hd = host.numpy(), hd.numpy()
    with tempfile.TemporaryDirectory() as d:
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            mio.write_png_rgba8(os.path.join(d, "plane.png"), hn[0])
            ts.append((time.perf_counter() - t) * 1e3)
    res["png_write_one_plane_ms"] = _median(ts)["median"]
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        refs = [IR.save_to_png_rgba(hd[..., c])[0] for c in range(3)]
        ts.append((time.perf_counter() - t) * 1e3)
    res["numpy_restatement_three_channels_ms"] = _median(ts)["median"]
    res["equal"] = bool(all(np.array_equal(hn[c], refs[c]) for c in range(3)))
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
