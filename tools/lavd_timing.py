#!/usr/bin/env python3
"""What the LAVD passes (mops_level_mean, mops_path_integral_abs, mops_path_integral_image)
cost, and what ``PathlineChain.run(attrs=True, integrals=...)`` adds to the same run with ``attrs=True`` alone: the
config-3 mesh (the bench's EC30to60-class mesh, 235 567 cells, 60 levels, device-generated snapshots from
mops_amd.synth_device) and a 3601 x 1801 global lattice -- one particle per pixel, 6.49e6 seeds.

    python tools/lavd_timing.py [--rounds 3] [--out lavd_timing.json]

Protocol: HIP events around every timed call, a device synchronise before the events are read, one warm-up round,
the median, minimum and maximum over the rounds; the two chain variants alternate within a round.
  level_mean      the vorticity of snapshot 0 [C, L] under the cell areas; the call allocates and frees its group
                  partials and synchronises, all inside the events.  Floor: C * L * 8 bytes read once.
  vorticity_deviation  engine.vorticity_deviation(vertex=True) of one field: gradient, areas, mean, subtraction,
                  cell-to-vertex -- what the chain's derived factory runs per snapshot.  No floor given.
  path_integral   one pair's attribute slab [K][1][n] onto the accumulator through the set's ids.  Floor: n * K * 8
                  bytes read once (the ids and the accumulator, 20 B per particle, are 1/K of that and left out).
  image           accumulator + death steps -> image.  Floor: n * (8 + 4 + 32) bytes.
  chain           three snapshots, two pairs of one day, deltaT 60 s, hourly records, Euler, keep_lines=False,
                  the fields resident and not owned; ``make_attrs`` = chain.vorticity_deviation_factory in both
                  variants, so the difference is the integral's accumulation alone.
Yardstick for the floors: the HBM peak (MI355X: 8 TB/s)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s
NAME = "vorticity_deviation"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--freq", type=int, default=158)
    ap.add_argument("--levels", type=int, default=60)
    ap.add_argument("--width", type=int, default=3601)
    ap.add_argument("--height", type=int, default=1801)
    ap.add_argument("--gap", type=int, default=86400)
    ap.add_argument("--delta-t", type=int, default=60)
    ap.add_argument("--record-t", type=int, default=3600)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build_engine()
    g.build_synth()
    import bench
    from mops_amd import _lib as L
    from mops_amd import synth
    from mops_amd.chain import EverDead, PathlineChain, vorticity_deviation_factory
    from mops_amd.engine import (DeviceField, DeviceMesh, FlowMapLattice, PathIntegral, cell_area, level_mean,
                                 velocity_gradient, vorticity_deviation)
    from mops_amd.synth_device import DeviceSnapshotSource

    if not torch.cuda.is_available():
        raise SystemExit("lavd_timing needs a GPU: nothing here is a measurement without one")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lib = L.load()
    mesh = synth.make_mesh(args.freq, n_levels=args.levels)
    dm = DeviceMesh.from_mesh(mesh)
    src = DeviceSnapshotSource(mesh, dev)
    fields = []
    for t in range(3):
        snap = src.make(timestep=t, phase=0.35 * t)
        torch.cuda.synchronize()
        fields.append(DeviceField.from_device_snapshot(dm, snap, timestep=t))
        del snap
    depth = bench.layer_mid_depth(mesh, 10)
    lat = FlowMapLattice(args.width, args.height, (-90.0, 90.0), (-180.0, 180.0), device=dev)
    n, Cn, Ln = lat.n, int(mesh.nCells), int(mesh.nVertLevels)
    K = args.gap // args.record_t
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    vort = velocity_gradient(dm, fields[0], "vorticity")["vorticity"]
    area = cell_area(dm)
    torch.cuda.synchronize()

    def run_chain(with_integral, keep):
        chain = PathlineChain(dm, lambda i, s: fields[i], 3, gap_seconds=args.gap, own_fields=False,
                              make_attrs=vorticity_deviation_factory(dm))
        it = PathIntegral(n, device=dev) if with_integral else None
        ever = EverDead()
        torch.cuda.synchronize()
        t, _ = timed(lambda: chain.run(lat.seeds, depth=depth, method=1, delta_t=args.delta_t, record_t=args.record_t,
                                       keep_lines=False, attrs=True, on_pair=ever,
                                       integrals={NAME: it} if with_integral else None))
        if with_integral:
            keep.update(integral=it, death=ever.death())
        return t

    ms = {k: [] for k in ("level_mean", "vorticity_deviation", "path_integral", "image", "chain_attrs", "chain_lavd")}
    keep = {}
    image = torch.empty((args.height, args.width, 4), dtype=torch.float64, device=dev)
    for rnd in range(args.rounds + 1):
        t = {}
        t["level_mean"], _ = timed(lambda: level_mean(vort, area))
        t["vorticity_deviation"], _ = timed(lambda: vorticity_deviation(dm, fields[0]))
        for name in (("chain_attrs", "chain_lavd") if rnd % 2 == 0 else ("chain_lavd", "chain_attrs")):
            t[name] = run_chain(name == "chain_lavd", keep)
        # one pair's slab as the chain leaves it: random data of the slab's shape, the ids a permutation
        if "slab" not in keep:
            keep["slab"] = torch.randn((K, 1, n), dtype=torch.float64, device=dev)
            keep["ids"] = torch.randperm(n, device=dev).to(torch.int32)
            keep["acc"] = torch.zeros((n,), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
        t["path_integral"], _ = timed(lambda: L.check(lib.mops_path_integral_abs(
            n, 0, K, C.c_void_p(keep["slab"].data_ptr()), n, 1, C.c_void_p(keep["ids"].data_ptr()), float(args.record_t),
            C.c_void_p(keep["acc"].data_ptr()), stream), "mops_path_integral_abs"))
        t["image"], _ = timed(lambda: L.check(lib.mops_path_integral_image(
            n, C.c_void_p(keep["integral"].accum.data_ptr()), C.c_void_p(keep["death"].data_ptr()),
            float(2 * args.gap), C.c_void_p(image.data_ptr()), stream), "mops_path_integral_image"))
        for k, v in t.items():
            if rnd > 0:
                ms[k].append(v)
            print(f"round {rnd} {k}: {v:.3f} ms", flush=True)
    floors = dict(level_mean=Cn * Ln * 8, path_integral=n * K * 8, image=n * 44)
    result = dict(build_id=bench.engine_build_id(), device=torch.cuda.get_device_name(0), cells=Cn, levels=Ln,
                  particles=n, records_per_pair=K, steps_per_pair=args.gap // args.delta_t, pairs=2,
                  image=[args.width, args.height], depth=float(depth), rounds=args.rounds, mean_group=L.MOPS_MEAN_GROUP,
                  finite_pixels=int(torch.isfinite(image[:, :, 0]).sum().item()),
                  lavd_max=float(torch.nan_to_num(image[:, :, 0], nan=0.0).max().item()),
                  hbm_peak_bytes_per_s=HBM_PEAK, passes={})
    for k, v in ms.items():
        med = statistics.median(v)
        row = dict(ms_median=med, ms_min=min(v), ms_max=max(v))
        if k in floors:
            floor_ms = floors[k] / HBM_PEAK * 1e3
            row.update(compulsory_bytes=floors[k], floor_ms=floor_ms, times_floor=med / floor_ms)
        result["passes"][k] = row
    a, b = result["passes"]["chain_attrs"]["ms_median"], result["passes"]["chain_lavd"]["ms_median"]
    result["chain_added_ms"] = b - a
    result["chain_added_share"] = (b - a) / a
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
