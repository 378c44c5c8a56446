#!/usr/bin/env python3
"""What a vertical section (mops_remap_section) costs beside the existing fixed-latitude
curtain (mops_remap_fixed_latitude) at the same width x height: a 3601 x 200 image on the bench's EC30to60-class
mesh (config 3: 235 567 cells, 60 levels, one device-generated snapshot from mops_amd.synth_device), the curtain
along the equator over 360 degrees and the section along the same circle as three great-circle legs, so that
both cut the same water and land.

    python tools/section_timing.py [--rounds 5] [--out profiles/r19/section_timing.json]

Protocol: each call whole -- scratch allocation, the columns' upload or formation, the locate of `width` points,
the evaluation kernel, the stream synchronisation -- between HIP events on torch's current stream, into
preallocated images (the ctypes entries, not the engine wrappers, so no tensor is allocated inside the events).
One warm-up round, then `rounds` rounds in which the three calls alternate their order; the median and the
minimum to maximum over the rounds.  Variants: the curtain (velocity only: it has no attributes), the section
with velocity only, the section with two vertex attributes.  The yardstick is the curtain in the same session on
the same device; its own min-to-max spread is the margin."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATH = [(0.0, -180.0), (0.0, -60.0), (0.0, 60.0), (0.0, 180.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--freq", type=int, default=158)
    ap.add_argument("--levels", type=int, default=60)
    ap.add_argument("--width", type=int, default=3601)
    ap.add_argument("--height", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build_engine()
    g.build_synth()
    import bench
    from mops_amd import _lib as L
    from mops_amd import engine, synth
    from mops_amd.synth_device import DeviceSnapshotSource

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lib = L.load()
    mesh = synth.make_mesh(args.freq, n_levels=args.levels)
    dm = engine.DeviceMesh.from_mesh(mesh)
    snap = DeviceSnapshotSource(mesh, dev).make(timestep=0, phase=0.0)
    torch.cuda.synchronize()
    df = engine.DeviceField.from_device_snapshot(dm, snap, timestep=0)
    del snap
    W, H, nl = args.width, args.height, mesh.nVertLevels
    drange = (float(mesh.refBottomDepth[0]), float(mesh.refBottomDepth[-1]))
    level = np.arange(nl, dtype=np.float64) / nl
    lat_cell = np.asarray(mesh.lat_cell, dtype=np.float64)
    temp = (25.0 * np.cos(lat_cell)[:, None]) * (1.0 - 0.8 * level[None, :])
    salt = 34.0 + 1.5 * level[None, :] + 0.5 * np.sin(lat_cell)[:, None]
    va = [engine.cell_to_vertex_attr(dm, a) for a in (salt, temp)]
    pts, nrm, dist = engine.section_points(PATH, W)
    cfg = engine._remap_cfg(W, H, lon_range=(-180.0, 180.0), latitude=0.0, depth_range=drange)
    curtain = torch.empty((H, W, 4), dtype=torch.float64, device=dev)
    sect = torch.empty((2, H, W, 4), dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def section(n_attr):
        return lambda: L.check(lib.mops_remap_section(
            dm.handle, df.handle, W, H, drange[0], drange[1], hp(pts), hp(nrm), n_attr, p(va[0]) if n_attr else None,
            p(va[1]) if n_attr > 1 else None, p(sect[0]), p(sect[1]) if n_attr else None, None, stream),
            "mops_remap_section")

    calls = dict(
        curtain=lambda: L.check(lib.mops_remap_fixed_latitude(dm.handle, df.handle, C.byref(cfg), p(curtain), None,
                                                              stream), "mops_remap_fixed_latitude"),
        section_velocity=section(0), section_two_attrs=section(2))
    names = list(calls)
    ms = {k: [] for k in names}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for rnd in range(args.rounds + 1):
        order = names[rnd % 3:] + names[:rnd % 3]
        for name in order:
            t = timed(calls[name])
            if rnd > 0:
                ms[name].append(t)
            print(f"round {rnd} {name}: {t:.3f} ms", flush=True)
    valid_c = int((~torch.isnan(curtain[:, :, 0])).sum().item())
    valid_s = int((~torch.isnan(sect[0, :, :, 0])).sum().item())
    sv, area = engine.section_transport(sect[0], dist, drange)
    result = dict(build_id=bench.engine_build_id(), device=torch.cuda.get_device_name(0), cells=int(mesh.nCells),
                  levels=int(nl), image=[W, H], depth_range=list(drange), path=PATH, rounds=args.rounds,
                  valid_pixels=dict(curtain=valid_c, section=valid_s), path_km=float(dist[-1] / 1e3),
                  transport_sv=sv, valid_area_m2=area, calls={})
    med_c = statistics.median(ms["curtain"])
    for name in names:
        med = statistics.median(ms[name])
        result["calls"][name] = dict(ms_median=med, ms_min=min(ms[name]), ms_max=max(ms[name]),
                                     ratio_to_curtain=med / med_c, pixels_per_s=W * H / (med * 1e-3))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
