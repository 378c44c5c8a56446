#!/usr/bin/env python3
"""What the eddy census (engine.eddy_census) costs on the bench's EC30to60-class mesh
(config 3: 235 567 cells, 60 levels, one device-generated snapshot from mops_amd.synth_device) at layer 10 and at
the two thresholds of the tests, -0.2 and -0.05 standard deviations of the layer's Okubo-Weiss parameter.

    python tools/census_timing.py [--rounds 5] [--out profiles/r22/census_timing.json]

Per threshold: the classes, components and eddies found, the labelling rounds, and the median and minimum to
maximum over `rounds` rounds (after one warm-up round) of
  velocity_gradient, cell_area, classify   HIP events around one launch each (the entries do not synchronise)
  label                                    HIP events around one mops_label_components call: its kernels and the
                                           host's read of the convergence flag between them (it synchronises)
  label_host, table_host, census_host      the host's clock around mops_label_components, around mops_eddy_count +
                                           mops_eddy_table (both synchronise; their host passes over the labels
                                           are part of the figure) and around the whole engine.eddy_census call
                                           with the gradient handed in, the device idle before and after."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--freq", type=int, default=158)
    ap.add_argument("--levels", type=int, default=60)
    ap.add_argument("--layer", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build_engine()
    g.build_synth()
    import bench
    from mops_amd import engine, synth
    from mops_amd.synth_device import DeviceSnapshotSource

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    mesh = synth.make_mesh(args.freq, n_levels=args.levels)
    dm = engine.DeviceMesh.from_mesh(mesh)
    snap = DeviceSnapshotSource(mesh, dev).make(timestep=0, phase=0.0)
    torch.cuda.synchronize()
    field = engine.DeviceField.from_device_snapshot(dm, snap, timestep=0)
    del snap
    zt, vel, w = field.export()
    field = engine.DeviceField.from_derived(dm, zt, vel, w)     # the vertex array in place: the gradient kernel alone
    del zt, vel, w
    layer = args.layer

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def host(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    grad = engine.velocity_gradient(dm, field, which=("vorticity", "okubo_weiss"))
    col = grad["okubo_weiss"][:, layer]
    sigma = float(torch.std(col[torch.isfinite(col)], unbiased=False))
    result = dict(build_id=bench.engine_build_id(), device=torch.cuda.get_device_name(0), cells=int(mesh.nCells),
                  levels=int(mesh.nVertLevels), layer=layer, rounds=args.rounds, sigma=sigma, thresholds={})
    for k_sigma in (0.2, 0.05):
        thr = -k_sigma * sigma
        ms = {k: [] for k in ("velocity_gradient", "cell_area", "classify", "label", "label_host", "table_host",
                              "census_host")}
        info = {}
        for rnd in range(args.rounds + 1):
            t = {}
            t["velocity_gradient"], _ = events(lambda: engine.velocity_gradient(dm, field,
                                                                               which=("vorticity", "okubo_weiss")))
            t["cell_area"], area = events(lambda: engine.cell_area(dm))
            t["classify"], cls = events(lambda: engine.eddy_classify(dm, grad["okubo_weiss"], grad["vorticity"],
                                                                     layer, thr))
            t["label"], (comp, rounds) = events(lambda: engine.label_components(dm, cls, return_rounds=True))
            t["label_host"], _ = host(lambda: engine.label_components(dm, cls))
            t["table_host"], (eoc, table) = host(lambda: engine.eddy_table(dm, comp, cls, area, grad["vorticity"],
                                                                           grad["okubo_weiss"], layer, 4))
            t["census_host"], cen = host(lambda: engine.eddy_census(dm, field, layer=layer, threshold=thr,
                                                                    gradient=grad))
            if rnd > 0:
                for k in ms:
                    ms[k].append(t[k])
            sizes = torch.bincount(comp[comp >= 0].long(), minlength=1)
            info = dict(threshold=thr, classed_cells=int((cls != 0).sum()), components=int((sizes > 0).sum()),
                        largest_component=int(sizes.max()), eddies_min_cells_4=int(len(table["root"])),
                        cyclonic=int((table["polarity"] > 0).sum()), anticyclonic=int((table["polarity"] < 0).sum()),
                        label_rounds=rounds, census_rounds=cen.rounds,
                        log2_bound=math.ceil(math.log2(max(int(sizes.max()), 1))) + 2,
                        same_labels=bool(torch.equal(cen.labels, eoc)))
            print(f"k_sigma {k_sigma} round {rnd}: " + " ".join(f"{k} {v:.3f}" for k, v in t.items()), flush=True)
        info["ms"] = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ms.items()}
        result["thresholds"][str(k_sigma)] = info
    # the labelling alone on class arrays that load it: every cell in one class (one component per basin) and
    # seeded random classes in {-1, 0, +1} (many small components, opposite classes side by side)
    result["synthetic"] = {}
    gen = torch.Generator(device="cpu").manual_seed(20)
    synthetic = dict(ones=torch.ones(mesh.nCells, dtype=torch.int32, device=dev),
                     random=torch.randint(-1, 2, (mesh.nCells,), generator=gen, dtype=torch.int32).to(dev))
    for name, cls in synthetic.items():
        ev, hs, rounds = [], [], 0
        for rnd in range(args.rounds + 1):
            t_ev, (comp, rounds) = events(lambda: engine.label_components(dm, cls, return_rounds=True))
            t_hs, again = host(lambda: engine.label_components(dm, cls))
            if rnd > 0:
                ev.append(t_ev)
                hs.append(t_hs)
        sizes = torch.bincount(comp[comp >= 0].long(), minlength=1)
        result["synthetic"][name] = dict(
            components=int((sizes > 0).sum()), largest_component=int(sizes.max()), label_rounds=rounds,
            log2_bound=math.ceil(math.log2(max(int(sizes.max()), 1))) + 2, same_bytes_twice=bool(torch.equal(comp, again)),
            roots_are_minima=bool((comp[comp >= 0] <= torch.nonzero(comp >= 0).reshape(-1)).all()),
            ms=dict(label=dict(median=statistics.median(ev), min=min(ev), max=max(ev)),
                    label_host=dict(median=statistics.median(hs), min=min(hs), max=max(hs))))
        print(f"synthetic {name}: {result['synthetic'][name]}", flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
