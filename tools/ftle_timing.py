#!/usr/bin/env python3
"""What the FTLE passes (mops_flowmap_lattice, mops_ftle_image) cost beside the launch that
moved their particles: a 3601 x 1801 global lattice -- one particle per pixel, 6.49e6 seeds formed on the device --
over one config-3 pair (the bench's EC30to60-class mesh, two device-generated snapshots from mops_amd.synth_device,
layer 10's mid depth, deltaT 60 s, one day = 1 440 Euler steps, hourly records), then the lattice pass and the FTLE
pass between HIP events.

    python tools/ftle_timing.py [--rounds 3] [--out profiles/r15/ftle_timing.json]

Protocol: one ParticleSet seeded from the lattice; per round the Euler launch (reset, seed locate and locality order
outside the events, HIP events around one ``advance`` over all steps), then ``mops_traj_last_points`` and the death
steps back in seed order (outside the events), then mops_flowmap_lattice into a preallocated tensor and
mops_ftle_image into a preallocated image, each between HIP events.  One warm-up round; the median, minimum and
maximum over the rounds.  Yardsticks: the same pair's Euler launch time, and the compulsory bytes over the HBM peak
(MI355X: 8 TB/s) -- per pixel 24 B of seed, 24 B of last point, 4 B of death step and 32 B of image for the FTLE
pass (84 B), 24 B of seed for the lattice pass (its tables are 5 402 doubles)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s
PASSES = (("lattice", 24), ("ftle", 84))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--freq", type=int, default=158)
    ap.add_argument("--levels", type=int, default=60)
    ap.add_argument("--width", type=int, default=3601)
    ap.add_argument("--height", type=int, default=1801)
    ap.add_argument("--lat", type=float, nargs=2, default=(-90.0, 90.0))
    ap.add_argument("--lon", type=float, nargs=2, default=(-180.0, 180.0))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build_engine()
    g.build_synth()
    import bench
    from mops_amd import _lib as L
    from mops_amd import synth
    from mops_amd.engine import DeviceField, DeviceMesh, FlowMapLattice, ParticleSet, TrajectoryConfig
    from mops_amd.synth_device import DeviceSnapshotSource

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lib = L.load()
    mesh = synth.make_mesh(args.freq, n_levels=args.levels)
    dm = DeviceMesh.from_mesh(mesh)
    src = DeviceSnapshotSource(mesh, dev)
    fields = []
    for t in range(2):
        snap = src.make(timestep=t, phase=0.35 * t)
        torch.cuda.synchronize()
        fields.append(DeviceField.from_device_snapshot(dm, snap, timestep=t))
        del snap
    f0, f1 = fields
    depth = bench.layer_mid_depth(mesh, 10)
    lat = FlowMapLattice(args.width, args.height, tuple(args.lat), tuple(args.lon), device=dev)
    n = lat.n
    cfg = TrajectoryConfig(deltaT=60, simulationDuration=86400, recordT=3600, depth=depth, method=1)
    ps = ParticleSet(dm, lat.seeds, depth, cfg)
    steps, K = cfg.n_steps, cfg.n_records
    horizon = cfg.simulationDuration / 86400.0
    points = torch.empty_like(lat.seeds)
    image = torch.empty((args.height, args.width, 4), dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = {"euler": [], **{name: [] for name, _ in PASSES}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    valid = 0
    for rnd in range(args.rounds + 1):
        ps.reset(depth)
        dm.locate(ps.seeds.data_ptr(), ps.cell.data_ptr(), ps.n, stream=torch.cuda.current_stream().cuda_stream)
        ps.reorder()
        t = timed(lambda: ps.advance(f0, f1, 0, steps))
        if rnd > 0:
            ms["euler"].append(t)
        print(f"round {rnd} euler launch: {t:.1f} ms", flush=True)
        last = ps.last_points(stream=torch.cuda.current_stream().cuda_stream)
        death = ps.original(ps.death)
        torch.cuda.synchronize()
        calls = dict(
            lattice=lambda: L.check(lib.mops_flowmap_lattice(C.byref(lat.cfg), C.c_void_p(points.data_ptr()), stream),
                                    "mops_flowmap_lattice"),
            ftle=lambda: L.check(lib.mops_ftle_image(C.byref(lat.cfg), C.c_void_p(lat.seeds.data_ptr()),
                                                     C.c_void_p(last.data_ptr()), C.c_void_p(death.data_ptr()), horizon,
                                                     1 if lat.wrap_lon else 0, C.c_void_p(image.data_ptr()), stream),
                                 "mops_ftle_image"))
        for name, _ in (PASSES if rnd % 2 == 0 else PASSES[::-1]):
            t = timed(calls[name])
            if rnd > 0:
                ms[name].append(t)
            print(f"round {rnd} {name}: {t:.3f} ms", flush=True)
        valid = int((~torch.isnan(image[:, :, 1])).sum().item())
        assert torch.equal(points, lat.seeds)
    alive = int((ps.death < 0).sum().item())
    result = dict(build_id=bench.engine_build_id(), library=os.environ.get("MOPS_TRAJ_LIB", "product"),
                  device=torch.cuda.get_device_name(0), particles=n, steps=steps, records=K, cells=int(mesh.nCells),
                  depth=float(depth), image=[args.width, args.height], lat=list(args.lat), lon=list(args.lon),
                  wrap_lon=bool(lat.wrap_lon), rounds=args.rounds, alive=alive, valid_pixels=valid,
                  ftle_min=float(torch.nan_to_num(image[:, :, 0], nan=float("inf")).min().item()),
                  ftle_max=float(torch.nan_to_num(image[:, :, 0], nan=-float("inf")).max().item()),
                  hbm_peak_bytes_per_s=HBM_PEAK, passes={})
    med_e = statistics.median(ms["euler"])
    result["euler_launch"] = dict(ms_median=med_e, ms_min=min(ms["euler"]), ms_max=max(ms["euler"]),
                                  psteps_per_s=n * steps / (med_e * 1e-3))
    for name, bytes_per_pixel in PASSES:
        med = statistics.median(ms[name])
        floor_ms = n * bytes_per_pixel / HBM_PEAK * 1e3
        result["passes"][name] = dict(ms_median=med, ms_min=min(ms[name]), ms_max=max(ms[name]),
                                      share_of_euler_launch=med / med_e, compulsory_bytes=n * bytes_per_pixel,
                                      floor_ms=floor_ms, times_floor=med / floor_ms, pixels_per_s=n / (med * 1e-3))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
