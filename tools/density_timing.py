#!/usr/bin/env python3
"""What the particle density pass (mops_density_accumulate) costs beside the launch that
wrote its records: one config-3 pair -- the bench's EC30to60-class mesh, two device-generated snapshots
(mops_amd.synth_device), 1e7 particles at layer 10's mid depth, deltaT 60 s, one day (1 440 steps), hourly records
(24 slots, 2.4e8 record points) -- then the density pass over the record slab at 3601 x 1801 global, for a COUNT
map and for a SPEED map.

    python tools/density_timing.py [--particles 10000000] [--rounds 3] [--out profiles/r14/density_timing.json]

Protocol: one ParticleSet; per round the Euler launch (reset, seed locate and locality order outside the events,
HIP events around one ``advance`` over all steps), then the two density passes in turn on the slab it wrote, each
between HIP events with its accumulator zeroed outside them (alternated rounds).  One warm-up round; the median,
minimum and maximum over the rounds.  Yardsticks: the same pair's Euler launch time, and the pass's own read floor
-- 24 B per record point for COUNT (x, y, z), 48 B for SPEED (and the velocity) over the HBM peak
(MI355X: 8 TB/s)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s
KINDS = (("count", None, 24), ("speed", "speed", 48))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--freq", type=int, default=158)
    ap.add_argument("--levels", type=int, default=60)
    ap.add_argument("--width", type=int, default=3601)
    ap.add_argument("--height", type=int, default=1801)
    ap.add_argument("--lat", type=float, nargs=2, default=(-90.0, 90.0), help="latitude window (a window that holds "
                    "no particle, e.g. 89.9 90, times the reads and the pixel arithmetic without any atomic)")
    ap.add_argument("--lon", type=float, nargs=2, default=(-180.0, 180.0))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build_engine()
    g.build_synth()
    import bench
    from mops_amd import synth
    from mops_amd.engine import DensityMap, DeviceField, DeviceMesh, ParticleSet, TrajectoryConfig
    from mops_amd.synth_device import DeviceSnapshotSource

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
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
    seeds = bench.make_seeds(args.particles, 0)
    n = int(seeds.shape[0])
    cfg = TrajectoryConfig(deltaT=60, simulationDuration=86400, recordT=3600, depth=depth, method=1)
    ps = ParticleSet(dm, seeds, depth, cfg)
    steps, K = cfg.n_steps, cfg.n_records
    maps = {name: DensityMap(args.width, args.height, tuple(args.lat), tuple(args.lon), value=value)
            for name, value, _ in KINDS}
    ms = {"euler": [], **{name: [] for name, _, _ in KINDS}}
    stats = {}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for rnd in range(args.rounds + 1):
        ps.reset(depth)
        dm.locate(ps.seeds.data_ptr(), ps.cell.data_ptr(), ps.n, stream=torch.cuda.current_stream().cuda_stream)
        ps.reorder()
        t = timed(lambda: ps.advance(f0, f1, 0, steps))
        if rnd > 0:
            ms["euler"].append(t)
        print(f"round {rnd} euler launch: {t:.1f} ms", flush=True)
        for name, _, _ in (KINDS if rnd % 2 == 0 else KINDS[::-1]):
            m = maps[name]
            m.reset()
            torch.cuda.synchronize()
            t = timed(lambda: m.accumulate(ps))
            if rnd > 0:
                ms[name].append(t)
            acc = m.accum
            stats[name] = dict(samples=int(acc[:, :, 0].sum().item()), pixels_hit=int((acc[:, :, 0] > 0).sum().item()),
                               max_per_pixel=int(acc[:, :, 0].max().item()))
            print(f"round {rnd} density {name}: {t:.3f} ms, {stats[name]}", flush=True)
    alive = int((ps.death < 0).sum().item())
    result = dict(build_id=bench.engine_build_id(), library=os.environ.get("MOPS_TRAJ_LIB", "product"),
                  device=torch.cuda.get_device_name(0), particles=n, steps=steps, records=K, record_points=n * K,
                  cells=int(mesh.nCells), depth=float(depth), image=[args.width, args.height], lat=list(args.lat),
                  lon=list(args.lon), rounds=args.rounds,
                  alive=alive, hbm_peak_bytes_per_s=HBM_PEAK, passes={})
    med_e = statistics.median(ms["euler"])
    result["euler_launch"] = dict(ms_median=med_e, ms_min=min(ms["euler"]), ms_max=max(ms["euler"]),
                                  psteps_per_s=n * steps / (med_e * 1e-3))
    for name, _, bytes_per_point in KINDS:
        med = statistics.median(ms[name])
        floor_ms = n * K * bytes_per_point / HBM_PEAK * 1e3
        result["passes"][name] = dict(ms_median=med, ms_min=min(ms[name]), ms_max=max(ms[name]),
                                      share_of_euler_launch=med / med_e, read_bytes=n * K * bytes_per_point,
                                      read_floor_ms=floor_ms, share_of_hbm_peak=floor_ms / med,
                                      points_per_s=n * K / (med * 1e-3), **stats[name])
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
