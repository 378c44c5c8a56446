#!/usr/bin/env python3
"""What sampling temperature / salinity along pathlines costs: unsampled vs the split path (a launch boundary at
every sample step, mops_traj_advance_sampled) vs the capture path (one launch per window,
mops_traj_advance_captured), DESIGN.md sections 3.13 / 3.14.

    python tools/attr_capture_timing.py [--out profiles/r12/attr_capture_timing.json] [--rows small,chain]

Protocol (section 3.13's): the bench's EC30to60-class mesh, two snapshots, deltaT 60 s, one day, hourly records
(1 440 steps, 25 sample steps), two attributes, Euler and RK4; HIP events around advance + line assembly on one
stream, one warm-up and the median of 3.  Row "small": 1e6 particles at 800 m (config 2's pathline shape); row
"chain": 1e7 particles at layer 10's mid depth (one config-3 daily pair).  The split path's kernels are the
unsampled run's and its host loop is unchanged, so it is also the cost before the capture path existed.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = {"small": dict(particles=1_000_000, depth=800.0), "chain": dict(particles=10_000_000, depth=None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="small,chain")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build_engine()
    import bench
    from mops_amd import synth
    from mops_amd.engine import DeviceField, DeviceMesh, ParticleSet, TrajectoryConfig, cell_to_vertex_attr

    torch.cuda.set_device(0)
    mesh = synth.make_mesh(158, n_levels=60)
    s0, s1 = synth.make_snapshot(mesh, timestep=0), synth.make_snapshot(mesh, timestep=1, phase=0.35)
    dm = DeviceMesh.from_mesh(mesh)
    f0, f1 = DeviceField.from_snapshot(dm, s0), DeviceField.from_snapshot(dm, s1)
    names = sorted(s0.attributes)[:2]
    lists = ([cell_to_vertex_attr(dm, s0.attributes[k]) for k in names],
             [cell_to_vertex_attr(dm, s1.attributes[k]) for k in names])
    result = dict(build_id=bench.engine_build_id(), device=torch.cuda.get_device_name(0), reps=args.reps,
                  protocol="deltaT 60 s, 86400 s, recordT 3600 s, 2 attributes; HIP events around advance + line "
                           "assembly, 1 warm-up, median of reps", rows=[])
    for row in args.rows.split(","):
        spec = ROWS[row]
        depth = spec["depth"] if spec["depth"] is not None else bench.layer_mid_depth(mesh, 10)
        seeds = bench.make_seeds(spec["particles"], 0)
        for method, mname in ((1, "euler"), (0, "rk4")):
            cfg = TrajectoryConfig(deltaT=60, simulationDuration=86400, recordT=3600, depth=depth, method=method)
            entry = dict(row=row, particles=int(seeds.shape[0]), depth=float(depth), method=mname)
            for mode, n_attr, W in (("unsampled", 0, 0), ("split", 2, 0), ("capture", 2, cfg.n_records)):
                ps = ParticleSet(dm, seeds, depth, cfg, n_attr=n_attr, capture_slots=W)
                adv, fin = [], []
                for rep in range(args.reps + 1):
                    ps.reset(depth)
                    dm.locate(ps.seeds.data_ptr(), ps.cell.data_ptr(), ps.n,  # (seeds in slot order, as bench.py)
                              stream=torch.cuda.current_stream().cuda_stream)
                    ps.reorder()
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    e[0].record()
                    ps.advance(f0, f1, 0, cfg.n_steps, attrs=lists if n_attr else None)
                    e[1].record()
                    out = ps.finalize(pathline=True)
                    e[2].record()
                    torch.cuda.synchronize()
                    del out
                    if rep > 0:
                        adv.append(e[0].elapsed_time(e[1]))
                        fin.append(e[1].elapsed_time(e[2]))
                entry[mode] = dict(advance_ms=statistics.median(adv), assembly_ms=statistics.median(fin),
                                   dead=int((ps.death >= 0).sum().item()))
                del ps
                torch.cuda.empty_cache()
                print(row, mname, mode, entry[mode], flush=True)
            base = entry["unsampled"]["advance_ms"] + entry["unsampled"]["assembly_ms"]
            for mode in ("split", "capture"):
                entry[mode]["ratio"] = (entry[mode]["advance_ms"] + entry[mode]["assembly_ms"]) / base
            result["rows"].append(entry)
    result["capture_below_split_in_every_row"] = all(r["capture"]["ratio"] < r["split"]["ratio"] for r in result["rows"])
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
