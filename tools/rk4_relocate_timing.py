#!/usr/bin/env python3
"""What the relocating RK4 (MOPS_RK4_RELOCATE) costs and keeps alive: one config-3 pair --
the bench's EC30to60-class mesh, two device-generated snapshots (mops_amd.synth_device), 1e7 particles at layer
10's mid depth, deltaT 60 s, one day (1 440 steps), hourly records -- under plain RK4, the relocating RK4 and Euler.

    python tools/rk4_relocate_timing.py [--particles 10000000] [--rounds 3] [--out profiles/r13/rk4_relocate.json]

Protocol: one ParticleSet; per round the three methods in turn (alternated rounds), each from the same seeds: reset,
seed locate and locality order outside the events, then HIP events around one ``advance`` over all steps.  One
warm-up round; the median, minimum and maximum over the rounds; particle-steps/s = particles x steps / median (the
bench's convention: steps offered, dead lanes included); alive = particles whose death step is -1 at the end."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METHODS = (("rk4", 0), ("rk4_relocate", 2), ("euler", 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--freq", type=int, default=158)
    ap.add_argument("--levels", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build_engine()
    g.build_synth()
    import bench
    from mops_amd import synth
    from mops_amd.engine import DeviceField, DeviceMesh, ParticleSet, TrajectoryConfig
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
    cfgs = {name: TrajectoryConfig(deltaT=60, simulationDuration=86400, recordT=3600, depth=depth, method=m)
            for name, m in METHODS}
    ps = ParticleSet(dm, seeds, depth, cfgs["rk4"])
    steps = cfgs["rk4"].n_steps
    ms = {name: [] for name, _ in METHODS}
    alive = {}
    for rnd in range(args.rounds + 1):
        for name, _ in METHODS:
            ps.set_config(cfgs[name])
            ps.reset(depth)
            dm.locate(ps.seeds.data_ptr(), ps.cell.data_ptr(), ps.n, stream=torch.cuda.current_stream().cuda_stream)
            ps.reorder()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ps.advance(f0, f1, 0, steps)
            e1.record()
            torch.cuda.synchronize()
            if rnd > 0:
                ms[name].append(e0.elapsed_time(e1))
            alive[name] = int((ps.death < 0).sum().item())
            print(f"round {rnd} {name}: {e0.elapsed_time(e1):.1f} ms, alive {alive[name]}", flush=True)
    result = dict(build_id=bench.engine_build_id(), device=torch.cuda.get_device_name(0), particles=n, steps=steps,
                  cells=int(mesh.nCells), depth=float(depth), rounds=args.rounds, methods={})
    for name, _ in METHODS:
        med = statistics.median(ms[name])
        result["methods"][name] = dict(ms_median=med, ms_min=min(ms[name]), ms_max=max(ms[name]),
                                       psteps_per_s=n * steps / (med * 1e-3), alive=alive[name], dead=n - alive[name])
    result["relocate_over_rk4_time"] = (result["methods"]["rk4_relocate"]["ms_median"] /
                                        result["methods"]["rk4"]["ms_median"])
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
