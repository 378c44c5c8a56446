#!/usr/bin/env python3
"""What the random walk (mops_traj_advance_diffuse / mops_traj_advance_layer_diffuse) costs:
one config-3 pair -- the bench's EC30to60-class mesh, two device-generated snapshots (mops_amd.synth_device), 1e7
particles, deltaT 60 s, one day (1 440 steps), hourly records -- under Euler, in layer mode (layer 10) and in depth
mode (layer 10's mid depth), with Kh = 0 (the existing kernels) and with Kh = 100 m^2/s (the diffusion kernel).

    python tools/diffusion_timing.py [--particles 10000000] [--rounds 3] [--out profiles/r18/diffusion_timing.json]

Protocol (tools/layer_timing.py's): one ParticleSet; per round the four (mode, Kh) runs in turn (alternated rounds),
each from the same seeds: reset, seed locate and locality order outside the events, then HIP events around one
``advance`` over all steps.  One warm-up round; the median, minimum and maximum over the rounds; alive = particles
whose death step is -1 at the end."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYER = 10
KH = 100.0
SEED = 2024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--freq", type=int, default=158)
    ap.add_argument("--levels", type=int, default=60)
    ap.add_argument("--kh", type=float, default=KH)
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
    runs = [(mode, kh) for mode in ("layer", "depth") for kh in (0.0, float(args.kh))]
    cfgs = {(mode, kh): TrajectoryConfig(deltaT=60, simulationDuration=86400, recordT=3600, depth=depth, method=1,
                                         layer=LAYER if mode == "layer" else None, diffusivity=kh, seed=SEED)
            for mode, kh in runs}
    ps = ParticleSet(dm, seeds, depth, cfgs[runs[0]])
    steps = cfgs[runs[0]].n_steps
    cur = torch.cuda.current_stream().cuda_stream
    for f in (f0, f1):  # the layer slices, outside the events
        f.layer_velocity(LAYER, stream=cur)
    torch.cuda.synchronize()
    ms = {r: [] for r in runs}
    alive = {}
    for rnd in range(args.rounds + 1):
        for r in runs:
            ps.set_config(cfgs[r])
            ps.reset(depth)
            dm.locate(ps.seeds.data_ptr(), ps.cell.data_ptr(), ps.n, stream=cur)
            ps.reorder()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ps.advance(f0, f1, 0, steps, stream=cur)
            e1.record()
            torch.cuda.synchronize()
            if rnd > 0:
                ms[r].append(e0.elapsed_time(e1))
            alive[r] = int((ps.death < 0).sum().item())
            print(f"round {rnd} {r[0]} Kh={r[1]:g}: {e0.elapsed_time(e1):.1f} ms, alive {alive[r]}", flush=True)
    result = dict(build_id=bench.engine_build_id(), device=torch.cuda.get_device_name(0), particles=n, steps=steps,
                  cells=int(mesh.nCells), vertices=int(mesh.nVertices), depth=float(depth), layer=LAYER,
                  kh=float(args.kh), method="euler", rounds=args.rounds, runs={})
    for mode, kh in runs:
        v = ms[(mode, kh)]
        med = statistics.median(v)
        result["runs"][f"{mode}_kh{kh:g}"] = dict(ms_median=med, ms_min=min(v), ms_max=max(v),
                                                  psteps_per_s=n * steps / (med * 1e-3), alive=alive[(mode, kh)],
                                                  dead=n - alive[(mode, kh)])
    for mode in ("layer", "depth"):
        result[f"diffusion_over_plain_time_{mode}"] = (result["runs"][f"{mode}_kh{float(args.kh):g}"]["ms_median"] /
                                                       result["runs"][f"{mode}_kh0"]["ms_median"])
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
