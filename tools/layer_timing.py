#!/usr/bin/env python3
"""What the layer mode (mops_traj_advance_layer) costs against the depth mode: one config-3
pair -- the bench's EC30to60-class mesh, two device-generated snapshots (mops_amd.synth_device), 1e7 particles,
deltaT 60 s, one day (1 440 steps), hourly records -- at layer 10 and, with the existing kernels, at layer 10's mid
depth, under Euler, RK4 and the relocating RK4.

    python tools/layer_timing.py [--particles 10000000] [--rounds 3] [--out profiles/r16/layer_timing.json]

Protocol: one ParticleSet; per round the six (mode, method) runs in turn (alternated rounds), each from the same seeds:
reset, seed locate and locality order outside the events, then HIP events around one ``advance`` over all steps.  One
warm-up round; the median, minimum and maximum over the rounds; alive = particles whose death step is -1 at the end.
The slice kernel (mops_field_layer_velocity) is timed the same way, once per round and snapshot."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METHODS = (("euler", 1), ("rk4", 0), ("rk4_relocate", 2))
LAYER = 10


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
    runs = [(mode, name) for name, _ in METHODS for mode in ("depth", "layer")]
    cfgs = {(mode, name): TrajectoryConfig(deltaT=60, simulationDuration=86400, recordT=3600, depth=depth, method=m,
                                           layer=LAYER if mode == "layer" else None)
            for name, m in METHODS for mode in ("depth", "layer")}
    ps = ParticleSet(dm, seeds, depth, cfgs[("depth", "rk4")])
    steps = cfgs[("depth", "rk4")].n_steps
    ms = {r: [] for r in runs}
    slice_ms = []
    alive = {}
    for rnd in range(args.rounds + 1):
        for f in (f0, f1):  # the slice kernel, rebuilt into the slice the field remembers
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f.layer_velocity(LAYER, out=f._layers.get(LAYER), stream=torch.cuda.current_stream().cuda_stream)
            e1.record()
            torch.cuda.synchronize()
            if rnd > 0:
                slice_ms.append(e0.elapsed_time(e1))
        for r in runs:
            ps.set_config(cfgs[r])
            ps.reset(depth)
            dm.locate(ps.seeds.data_ptr(), ps.cell.data_ptr(), ps.n, stream=torch.cuda.current_stream().cuda_stream)
            ps.reorder()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ps.advance(f0, f1, 0, steps, stream=torch.cuda.current_stream().cuda_stream)
            e1.record()
            torch.cuda.synchronize()
            if rnd > 0:
                ms[r].append(e0.elapsed_time(e1))
            alive[r] = int((ps.death < 0).sum().item())
            print(f"round {rnd} {r[0]} {r[1]}: {e0.elapsed_time(e1):.1f} ms, alive {alive[r]}", flush=True)
    result = dict(build_id=bench.engine_build_id(), device=torch.cuda.get_device_name(0), particles=n, steps=steps,
                  cells=int(mesh.nCells), vertices=int(mesh.nVertices), depth=float(depth), layer=LAYER,
                  rounds=args.rounds, slice_bytes=int(mesh.nVertices) * 32,
                  slice_kernel_ms=dict(median=statistics.median(slice_ms), min=min(slice_ms), max=max(slice_ms)),
                  runs={})
    for mode, name in runs:
        v = ms[(mode, name)]
        med = statistics.median(v)
        result["runs"][f"{mode}_{name}"] = dict(ms_median=med, ms_min=min(v), ms_max=max(v),
                                                psteps_per_s=n * steps / (med * 1e-3), alive=alive[(mode, name)],
                                                dead=n - alive[(mode, name)])
    for name, _ in METHODS:
        result[f"layer_over_depth_time_{name}"] = (result["runs"][f"layer_{name}"]["ms_median"] /
                                                   result["runs"][f"depth_{name}"]["ms_median"])
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
