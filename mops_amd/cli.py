"""MOPS_CLI on the MI355X engine: ``python -m mops_amd.cli -i <yaml> [...]``.

Mirrors the reference's command-line driver (CLI/main.cpp) option for option:

    -i/--input     ftk stream YAML (required)          cxxopts "input,i"
    -p/--prefix    data path prefix                     "prefix,p"
    -t/--timestep  single timestep (default 0)          "timestep,t"
    -r/--range     timestep list ("-r 1,2" or repeated) "range,r"
    -g/--day       day gap (default 1)                  "day,g"
    -d/--depth     fixed depth in metres (default 10)   "depth,d"
    --vti          extension: also write the VTI of the reference's MOPS_VTK build branch
    --layer K      extension: the streamline advects within model layer K (TrajectorySettings.fixedLayer)
                   instead of at the fixed depth; absent = the reference's run
    --kh KH        extension: a horizontal random walk of eddy diffusivity KH (m^2/s) on top of the streamline
                   (TrajectorySettings.diffusivity); needs --layer
    --seed N       extension: the random walk's seed (TrajectorySettings.randomSeed, default 0)
    --section "lat,lon;lat,lon[;...]"
                   extension: per timestep also a vertical section along the great-circle legs through these
                   waypoints (3601 columns x 201 rows over the reference bottom depths; the YAML carries no image
                   size), written as ``section_output_<i>_ch<c>.png`` (with ``--vti`` also
                   ``section_timestep_<t>_tile_0_fixed_depth_0.000000.vti``), and its transport, printed
    --eddy         extension: per timestep also the relative vorticity and Okubo-Weiss image at the fixed depth, on
                   the remap's window and size, written as ``eddy_output_0_ch<c>.png`` (with ``--vti`` also
                   ``eddy_timestep_<t>_tile_0_fixed_depth_<depth>.vti``)
    --eddy-census  extension: per timestep also the eddy census of model layer ``--layer K`` (layer 0 without it):
                   ``eddy_census_<t>.txt``, one line per eddy (index, lat, lon, radius in km, area in m^2, polarity,
                   circulation in m^2/s, cells), the label image ``eddy_labels_output_0_ch<c>.png`` on the remap's
                   window and size (with ``--vti`` also ``eddy_labels_timestep_<t>_tile_0_fixed_depth_<K>.vti``),
                   and the count, printed

and its run (CLI/main.cpp:94-262): grid and one solution per timestep from the
YAML (initGrid_DemoLoading / initSolution_DemoLoading, with temperature and
salinity attributes); per timestep a 3601 x 1801 global fixed-depth remap
written as ``output_<i>_ch<c>.png`` (:133-187; with ``--vti`` also
``timestep_<t>_tile_0_fixed_depth_<depth>.vti``); a 31x31 sample lattice in
lat [35, 45), lon [-90, -15) at the fixed depth, and -- for a single timestep
-- a StreamLine with deltaT = 1 h, simulationDuration = day_gap days,
recordT = 6 h, written as ``traj_line_<t>.txt`` (the reference's text dump)
and ``traj_line_<t>.vtp`` (its VTK build's SaveTrajectoryLinesAsVTP) in the
working directory.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

ONE_HOUR = 3600
ONE_DAY = 86400


def _int_list(values):
    out = []
    for v in values or []:
        out.extend(int(x) for x in str(v).split(",") if x.strip())
    return out


def parse_command_line(argv):
    """CLI/main.cpp:28-56 (cxxopts); returns None where the reference returns false (help, no input)."""
    p = argparse.ArgumentParser(prog="MOPS_CLI", add_help=False)
    p.add_argument("-i", "--input", default=None, help="Input yaml file")
    p.add_argument("-p", "--prefix", default="", help="Data path prefix")
    p.add_argument("-t", "--timestep", type=int, default=0, help="single timestep")
    p.add_argument("-r", "--range", action="append", default=None, help="Timestep range")
    p.add_argument("-g", "--day", type=int, default=1, help="Day Gap")
    p.add_argument("-d", "--depth", type=float, default=10.0, help="Fixed depth")
    p.add_argument("--vti", action="store_true", help="Also write the remapped images as VTK ImageData")
    p.add_argument("--layer", type=int, default=None, help="Streamline within this model layer (default: at the depth)")
    p.add_argument("--kh", type=float, default=0.0, help="Horizontal eddy diffusivity in m^2/s (needs --layer)")
    p.add_argument("--seed", type=int, default=0, help="Seed of the random walk")
    p.add_argument("--section", default=None, help='Vertical section along "lat,lon;lat,lon[;...]"')
    p.add_argument("--eddy", action="store_true", help="Also write the vorticity / Okubo-Weiss image")
    p.add_argument("--eddy-census", dest="eddy_census", action="store_true",
                   help="Also write the eddy census of layer --layer (default 0) and its label image")
    p.add_argument("-h", "--help", action="store_true", help="Print this information")
    argv = list(argv)
    for i in range(len(argv) - 1):  # a path that begins with a southern latitude ("-30,...") is a value, not an option
        if argv[i] == "--section":
            argv[i:i + 2] = ["--section=" + argv[i + 1]]
            break
    args = p.parse_args(argv)
    if args.help:
        print(p.format_help())
        return None
    if not args.input:
        print("[ERROR]::Input yaml file is required.")
        return None
    if args.layer is not None and args.layer < 0:
        print("[ERROR]::--layer must be a model layer index (>= 0).")
        return None
    if not (args.kh >= 0.0) or not np.isfinite(args.kh):
        print("[ERROR]::--kh must be a finite diffusivity (>= 0).")
        return None
    if args.kh > 0.0 and args.layer is None:
        print("[ERROR]::--kh needs --layer (the streamline at a fixed depth has no diffusion).")
        return None
    if args.seed < 0 or args.seed >= 2 ** 64:
        print("[ERROR]::--seed must be in [0, 2^64).")
        return None
    if args.section is not None:
        try:
            args.section = parse_section(args.section)
        except ValueError as e:
            print(f'[ERROR]::--section must be "lat,lon;lat,lon[;...]" ({e}).')
            return None
    args.range = _int_list(args.range)
    return args


REMAP_WIDTH, REMAP_HEIGHT = 3601, 1801   # CLI/main.cpp:137
VTI_NAMES = ("E: Zonal Velocity", "N: Meridional Velocity", "Velocity Magnitude",
             "Temperature", "Salinity", "None")  # CLI/main.cpp:157-160 (image 1 holds salinity first: quirk Q16)


def run_remapping_stage(M, mio, timestep, depth, vti=False, width=REMAP_WIDTH, height=REMAP_HEIGHT):
    """CLI/main.cpp:133-187 for one active timestep: the global fixed-depth remap, then ``output_<i>_ch<c>.png``
    for every image i and channel c < 3 (the same names at every timestep, as the reference), and with ``vti``
    ``timestep_<t>_tile_0_fixed_depth_<depth>.vti``.  The images are coloured on the device; only their RGBA
    bytes come to the host (the doubles too for a VTI, which stores them).  Returns the files written."""
    from . import engine
    cfg = M.VisualizationSettings()
    cfg.imageSize = (float(width), float(height))
    cfg.LatRange = (-90.0, 90.0)
    cfg.LonRange = (-180.0, 180.0)
    cfg.FixedDepth = depth
    cfg.TimeStep = timestep
    cfg.SaveType = M.SaveType.kVTI if vti else M.SaveType.kPNG
    images = M._remap_device(cfg)
    if images is None:
        return []
    written = []
    for i in range(images.shape[0]):
        planes = engine.colormap_rgba(images[i], channels=(0, 1, 2)).cpu().numpy()
        for ch in range(3):
            name = f"output_{i}_ch{ch}.png"
            mio.write_png_rgba8(name, planes[ch])
            written.append(name)
    if vti:
        written.append(M.SaveVTI(images.cpu().numpy(), cfg, VTI_NAMES, f"timestep_{timestep}_tile_{cfg.tile_index}"))
    print(f"[MOPS_CLI] timestep {timestep}: remapping images written: " + " ".join(written))
    return written


SECTION_WIDTH, SECTION_HEIGHT = REMAP_WIDTH, 201   # the remap's columns; rows every 1/200 of the depth range
SECTION_VTI_NAMES = ("E: Zonal Velocity", "N: Meridional Velocity", "Across-section Velocity",
                     "Salinity", "Temperature", "None")   # image 1: the attributes in name order


def parse_section(text):
    """``"lat,lon;lat,lon[;...]"`` -> [(lat, lon), ...]; ValueError for anything else."""
    path = []
    for part in str(text).split(";"):
        xy = part.split(",")
        if len(xy) != 2:
            raise ValueError(f"bad waypoint {part!r}")
        path.append((float(xy[0]), float(xy[1])))
    if len(path) < 2:
        raise ValueError("a section needs two waypoints")
    return path


def run_section_stage(M, mio, timestep, path, vti=False, width=SECTION_WIDTH, height=SECTION_HEIGHT):
    """The extension ``--section``: the vertical section of the active timestep along ``path`` over the grid's
    reference bottom depths, written beside the remapping stage's files in its naming with a ``section_``
    prefix -- ``section_output_<i>_ch<c>.png`` and, with ``vti``, ``section_timestep_<t>_tile_0_fixed_depth_
    0.000000.vti`` (x: metres along the path, y: -depth) -- and its transport, printed.  Returns (the files
    written, the transport in Sverdrups), or ([], None) for invalid inputs."""
    from . import engine
    cfg = M.VisualizationSettings()
    cfg.imageSize = (float(width), float(height))
    cfg.SectionPath = list(path)
    cfg.TimeStep = timestep
    cfg.SaveType = M.SaveType.kVTI if vti else M.SaveType.kPNG
    images = M._section_device(cfg)
    if images is None:
        return [], None
    written = []
    for i in range(images.shape[0]):
        planes = engine.colormap_rgba(images[i], channels=(0, 1, 2)).cpu().numpy()
        for ch in range(3):
            name = f"section_output_{i}_ch{ch}.png"
            mio.write_png_rgba8(name, planes[ch])
            written.append(name)
    _, _, dist = engine.section_points(path, int(width))
    ref = np.asarray(M._app.grid.cellRefBottomDepth_vec, dtype=np.float64).reshape(-1)
    if vti:
        cfg.FixedDepth = 0.0
        cfg.LonRange = (0.0, float(dist[-1]))
        cfg.LatRange = (-float(ref[-1]), -float(ref[0]))
        written.append(M.SaveVTI(images.cpu().numpy(), cfg, SECTION_VTI_NAMES,
                                 f"section_timestep_{timestep}_tile_{cfg.tile_index}"))
    sv, _ = engine.section_transport(images[0], dist, (float(ref[0]), float(ref[-1])))
    print(f"[MOPS_CLI] timestep {timestep}: section images written: " + " ".join(written))
    print(f"[MOPS_CLI] timestep {timestep}: section of {dist[-1] / 1000.0:.3f} km, transport {sv:.6f} Sv "
          "(positive to the left of the direction of travel)")
    return written, sv


EDDY_VTI_NAMES = ("Relative Vorticity", "Okubo-Weiss", "None")


def run_eddy_stage(M, mio, timestep, depth, vti=False, width=REMAP_WIDTH, height=REMAP_HEIGHT):
    """The extension ``--eddy``: the relative vorticity and the Okubo-Weiss parameter of the active timestep on
    the remapping stage's window, size and depth (``MOPS_RunEddyMap``), written beside its files in its naming
    with an ``eddy_`` prefix -- ``eddy_output_0_ch<c>.png`` (channel 2 is the image's zero channel) and, with
    ``vti``, ``eddy_timestep_<t>_tile_0_fixed_depth_<depth>.vti``.  Returns the files written."""
    from . import engine
    cfg = M.VisualizationSettings()
    cfg.imageSize = (float(width), float(height))
    cfg.LatRange = (-90.0, 90.0)
    cfg.LonRange = (-180.0, 180.0)
    cfg.FixedDepth = depth
    cfg.TimeStep = timestep
    cfg.SaveType = M.SaveType.kVTI if vti else M.SaveType.kPNG
    image = M._eddy_device(cfg)
    if image is None:
        return []
    written = []
    planes = engine.colormap_rgba(image, channels=(0, 1, 2)).cpu().numpy()
    for ch in range(3):
        name = f"eddy_output_0_ch{ch}.png"
        mio.write_png_rgba8(name, planes[ch])
        written.append(name)
    if vti:
        written.append(M.SaveVTI(image.cpu().numpy()[None], cfg, EDDY_VTI_NAMES,
                                 f"eddy_timestep_{timestep}_tile_{cfg.tile_index}"))
    print(f"[MOPS_CLI] timestep {timestep}: eddy images written: " + " ".join(written))
    return written


CENSUS_VTI_NAMES = ("Eddy Index", "Polarity", "None")


def run_census_stage(M, mio, timestep, layer, vti=False, width=REMAP_WIDTH, height=REMAP_HEIGHT):
    """The extension ``--eddy-census``: the eddies of the active timestep at model layer ``layer``
    (``MOPS_RunEddyCensus`` with the settings' defaults: 0.2 standard deviations, 4 cells), written as
    ``eddy_census_<t>.txt`` -- one line per eddy: index, lat, lon, radius in km, area in m^2, polarity,
    circulation in m^2/s, cells -- and their label image on the remapping stage's window and size as
    ``eddy_labels_output_0_ch<c>.png`` and, with ``vti``, ``eddy_labels_timestep_<t>_tile_0_fixed_depth_
    <layer>.vti``.  Prints the count.  Returns (the files written, the eddies), or ([], None) for invalid inputs."""
    from . import engine
    cfg = M.VisualizationSettings()
    cfg.imageSize = (float(width), float(height))
    cfg.LatRange = (-90.0, 90.0)
    cfg.LonRange = (-180.0, 180.0)
    cfg.FixedLayer = float(layer)
    cfg.TimeStep = timestep
    cfg.SaveType = M.SaveType.kVTI if vti else M.SaveType.kPNG
    got = M._census_device(cfg)
    if got is None:
        return [], None
    census, image = got
    eddies = M._census_rows(census)
    written = [f"eddy_census_{timestep}.txt"]
    with open(written[0], "w") as f:
        f.write("# index lat lon radius_km area_m2 polarity circulation_m2_s cells\n")
        for e in eddies:
            f.write(f"{e['index']} {e['lat']:.6f} {e['lon']:.6f} {e['radius'] / 1000.0:.6f} {e['area']:.9e} "
                    f"{e['polarity']:+d} {e['circulation']:.9e} {e['n_cells']}\n")
    planes = engine.colormap_rgba(image, channels=(0, 1, 2)).cpu().numpy()
    for ch in range(3):
        name = f"eddy_labels_output_0_ch{ch}.png"
        mio.write_png_rgba8(name, planes[ch])
        written.append(name)
    if vti:
        written.append(M.SaveVTI(image.cpu().numpy()[None], cfg, CENSUS_VTI_NAMES,
                                 f"eddy_labels_timestep_{timestep}_tile_{cfg.tile_index}"))
    n_pos = sum(1 for e in eddies if e["polarity"] > 0)
    print(f"[MOPS_CLI] timestep {timestep}: eddy census of layer {census.layer}: {len(eddies)} eddies "
          f"({n_pos} of positive vorticity, {len(eddies) - n_pos} of negative) below Okubo-Weiss "
          f"{census.threshold:.6e}; written: " + " ".join(written))
    return written, eddies


def main(argv=None) -> int:
    args = parse_command_line(sys.argv[1:] if argv is None else argv)
    if args is None:
        return 1
    print("== command line arguments ==")
    print(f"== input_yaml_filename: {args.input}")
    print(f"== data_path_prefix: {args.prefix}")
    print(f"== timestep: {args.timestep}")
    print(f"== day_gap: {args.day}")
    print(f"== fixed_depth: {args.depth}")
    print("== time_range_vec: " + "".join(f"{t} " for t in args.range))

    from . import io as mio
    from . import pyMOPS as M

    # 1-4. engine, grid, one solution per timestep, attributes
    M.MOPS_Init("gpu")
    timesteps = list(args.range) if args.range else [args.timestep]
    grid = M.MPASOGrid()
    grid.init_from_yaml(args.input)
    sols = []
    for t in timesteps:
        s = M.MPASOSolution()
        s.init_from_yaml(args.input, "", t)       # initSolution_DemoLoading(yaml, t)
        s.add_attribute("temperature")
        s.add_attribute("salinity")
        sols.append(s)
    M.MOPS_Begin()
    M.MOPS_AddGridMesh(grid)
    for t, s in zip(timesteps, sols):
        M.MOPS_AddAttribute(t, s)
    M.MOPS_End()

    # 5-6. per-timestep remapping (CLI/main.cpp:133-187); the last timestep stays active, as in the reference
    for t in timesteps:
        M.MOPS_ActiveAttribute(t)
        run_remapping_stage(M, mio, t, args.depth, args.vti)
        if args.section is not None:
            run_section_stage(M, mio, t, args.section, args.vti)
        if args.eddy:
            run_eddy_stage(M, mio, t, args.depth, args.vti)
        if args.eddy_census:
            run_census_stage(M, mio, t, args.layer if args.layer is not None else 0, args.vti)

    # 7. sample points: 31 x 31 lattice request in [35, 45] x [-90, -15] (exclusive upper bounds)
    print("== generate sample points ==")
    ss = M.SeedsSettings()                    # SamplingSettings, atCellCenter(false)
    ss.setSeedsRange((31, 31))
    ss.setGeoBox((35.0, 45.0), (-90.0, -15.0))
    ss.setDepth(args.depth)
    sample_points = M.MOPS_GenerateSeedsPoints(ss)

    # 8. trajectories: a streamline for a single timestep (the reference runs none for a range)
    cfg = M.TrajectorySettings()
    cfg.depth = args.depth
    cfg.deltaT = ONE_HOUR * 1
    cfg.simulationDuration = ONE_DAY * args.day
    cfg.recordT = ONE_HOUR * 6
    cfg.fileName = f"traj_line_{timesteps[0]}"
    if args.layer is not None:
        cfg.fixedLayer = args.layer
    cfg.diffusivity = args.kh
    cfg.randomSeed = args.seed
    if len(timesteps) == 1:
        print("== single timestep [streamline] ==")
        lines = M.MOPS_RunStreamLine(cfg, sample_points)
        if lines:
            stacked = {"points": np.stack([ln["points"] for ln in lines]),
                       "velocity": np.stack([ln["velocity"] for ln in lines])}
            mio.save_trajectory_lines_vtp(cfg.fileName + ".vtp", stacked)
            mio.save_trajectory_lines_txt(cfg.fileName + ".txt", stacked)
            print(f"[✓] Trajectory lines saved to {cfg.fileName}.txt")
        else:
            print(f"[Error] Unable to open file for writing: {cfg.fileName}.txt", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
