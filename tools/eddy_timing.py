#!/usr/bin/env python3
"""What the velocity-gradient kernel (mops_velocity_gradient) costs on the bench's
EC30to60-class mesh (config 3: 235 567 cells, 60 levels, one device-generated snapshot from
mops_amd.synth_device), beside its traffic floor: one read of the vertex velocities [V][L][3] plus the writes of
the requested outputs [C][L], at the HBM rate a streaming copy reaches on this device (6.3 TB/s).

    python tools/eddy_timing.py [--rounds 5] [--reps 20] [--out profiles/r20/eddy_timing.json]

Variants: the field as the fused derivation leaves it (the entry first rebuilds the vertex array from the
level-pair records: records_to_vertex_kernel, then the gradient kernel) and the same field uploaded again as
vertex arrays (the gradient kernel alone), each with all four outputs and with vorticity and Okubo-Weiss only;
and the signed cell-to-vertex interpolation of one array.  Protocol: `reps` launches between two HIP events on
torch's current stream into preallocated outputs (the ctypes entries, so no tensor is allocated inside the
events), the time per launch; one warm-up round, then `rounds` rounds in which the variants alternate their
order; the median and the minimum to maximum over the rounds.  Under ``rocprofv3 --kernel-trace --stats`` the same
run gives the kernels' own durations, records_to_vertex_kernel's among them."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--freq", type=int, default=158)
    ap.add_argument("--levels", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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
    fused = engine.DeviceField.from_device_snapshot(dm, snap, timestep=0)
    del snap
    zt, vel, w = fused.export()
    full = engine.DeviceField.from_derived(dm, zt, vel, w)
    del zt, vel, w
    nc, nv, nl = int(mesh.nCells), int(mesh.nVertices), int(mesh.nVertLevels)
    out = torch.empty((4, nc, nl), dtype=torch.float64, device=dev)
    vert = torch.empty((nv, nl), dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def gradient(field, four):
        ptr = [p(out[0]), p(out[1]) if four else None, p(out[2]) if four else None, p(out[3])]
        return lambda: L.check(lib.mops_velocity_gradient(dm.handle, field.handle, *ptr, stream),
                               "mops_velocity_gradient")

    calls = dict(
        fused_four=gradient(fused, True), fused_two=gradient(fused, False),
        vertex_array_four=gradient(full, True), vertex_array_two=gradient(full, False),
        cell_to_vertex_signed=lambda: L.check(lib.mops_cell_to_vertex_signed(dm.handle, p(out[0]), p(vert), stream),
                                              "mops_cell_to_vertex_signed"))
    names = list(calls)
    ms = {k: [] for k in names}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    for rnd in range(args.rounds + 1):
        k = rnd % len(names)
        for name in names[k:] + names[:k]:
            t = timed(calls[name])
            if rnd > 0:
                ms[name].append(t)
            print(f"round {rnd} {name}: {t * 1e3:.1f} us", flush=True)
    # the two sources give the same bytes
    calls["fused_four"]()
    a = out.clone()
    calls["vertex_array_four"]()
    torch.cuda.synchronize()
    same = bool(torch.equal(a.view(torch.int64), out.view(torch.int64)))
    vel_bytes = nv * nl * 3 * 8
    out_bytes = nc * nl * 8
    floor = {"four": (vel_bytes + 4 * out_bytes) / HBM_BYTES_PER_S * 1e3,
             "two": (vel_bytes + 2 * out_bytes) / HBM_BYTES_PER_S * 1e3,
             "cell_to_vertex_signed": (out_bytes + nv * nl * 8) / HBM_BYTES_PER_S * 1e3}
    result = dict(build_id=bench.engine_build_id(), device=torch.cuda.get_device_name(0), cells=nc, vertices=nv,
                  levels=nl, rounds=args.rounds, reps=args.reps, same_bytes_from_both_sources=same,
                  finite_fraction=float(torch.isfinite(out).double().mean().item()),
                  hbm_bytes_per_s=HBM_BYTES_PER_S, vertex_velocity_bytes=vel_bytes, output_bytes_each=out_bytes,
                  record_bytes=nv * (nl - 1) * 80, calls={})
    for name in names:
        med = statistics.median(ms[name])
        fl = floor[name.rsplit("_", 1)[1]] if name != "cell_to_vertex_signed" else floor[name]
        result["calls"][name] = dict(ms_median=med, ms_min=min(ms[name]), ms_max=max(ms[name]), floor_ms=fl,
                                     ratio_to_floor=med / fl)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
