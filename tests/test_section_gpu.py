"""Vertical sections on the GPU (mops_remap_section) against the per-pixel restatement
(tests/section_reference.py) and against the existing curtain: every channel of every image bit for bit, on the
small mesh and across the live wide cells of the wheel meshes, then the same through pyMOPS, the C++ API and
the CLI.  The restatement's own outcome codes are asserted first, so that each comparison means something."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_reference as IR  # noqa: E402
import remap_reference as RR  # noqa: E402
import section_reference as SR  # noqa: E402
import wide_case as WC  # noqa: E402
from test_remap_gpu import _assert_coverage, _pymops  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO = [(-30.0, -20.0), (50.0, 80.0)]                     # South Atlantic -> across Africa (culled) -> Asia
THREE = [(-30.0, -40.0), (20.0, 10.0), (35.0, 80.0)]
# key: (path, width, height, attributes, normals?)
CASES = {
    "two_37x20": (TWO, 37, 20, 2, True),
    "two_one_attr": (TWO, 37, 20, 1, True),
    "two_no_attr_no_normals": (TWO, 37, 20, 0, False),
    "three_65x3": (THREE, 65, 3, 2, True),
    "w2": ([(10.0, 170.0), (-10.0, -170.0)], 2, 20, 1, True),
    "h1": (TWO, 37, 1, 2, True),
}


@pytest.fixture(scope="module")
def case(engine_lib, oracle_lib, gpu, small_case):
    from mops_amd import engine
    mesh, s0, _ = small_case
    dm = engine.DeviceMesh.from_mesh(mesh)
    df = engine.DeviceField.from_snapshot(dm, s0)
    derived = oracle_lib.preprocess(mesh, s0)
    names = sorted(s0.attributes)
    assert names[:2] == ["salinity", "temperature"]
    vattrs = tuple(engine.cell_to_vertex_attr(dm, s0.attributes[k]) for k in names[:2])
    drange = (float(mesh.refBottomDepth[0]), float(mesh.refBottomDepth[-1]))
    return dict(mesh=mesh, snap=s0, dm=dm, df=df, derived=derived, names=names, vattrs=vattrs, O=oracle_lib,
                drange=drange, cache={})


def _reference(c, key):
    if key not in c["cache"]:
        path, w, h, n_attr, with_normals = CASES[key]
        pts, nrm, dist = SR.section_points(path, w)
        cells = c["O"].knn(c["mesh"], pts)
        ref = SR.section(c["mesh"], c["derived"], pts, nrm if with_normals else None, h, c["drange"], cells,
                         attrs=[c["derived"].attrs[k] for k in c["names"][:n_attr]])
        c["cache"][key] = dict(ref, pts=pts, nrm=nrm, dist=dist, cells=cells)
    return c["cache"][key]


def test_same_bytes_as_the_fixed_latitude_curtain(case):
    """The curtain of test_remap_gpu.test_fixed_latitude_bit_exact (36 x 20 at 20 N), fed to the section as
    explicit columns: channels 0 and 1, alpha and the cells are mops_remap_fixed_latitude's bytes."""
    from mops_amd import engine
    w, h, lon, flat = 36, 20, (-170.0, 150.0), 20.0
    curtain, ccells = engine.remap_fixed_latitude(case["dm"], case["df"], w, h, lon, flat, case["drange"],
                                                  return_cells=True)
    curtain = curtain.cpu().numpy()
    assert np.isfinite(curtain[..., 0]).mean() > 0.4 and np.isnan(curtain[..., 0]).mean() > 0.05
    pts = RR.latitude_positions(w, lon, flat)
    images, dist, cells = engine.remap_section(case["dm"], case["df"], None, w, h, case["drange"],
                                               columns=(pts, None), return_cells=True)
    got = images.cpu().numpy()
    assert got.shape == (1, h, w, 4) and dist is None
    assert np.array_equal(cells.cpu().numpy(), ccells.cpu().numpy())
    assert got[0][..., [0, 1, 3]].tobytes() == curtain[..., [0, 1, 3]].tobytes()
    assert np.array_equal(np.isnan(got[0][..., 2]), np.isnan(curtain[..., 0]))
    assert np.all(got[0][..., 2][np.isfinite(curtain[..., 0])] == 0.0)   # no normals: across = 0.0


@pytest.mark.parametrize("key", sorted(CASES))
def test_section_images_bit_exact(case, key):
    """Asserted on the restatement before the comparison: the two- and three-waypoint paths hold valid, outside
    (culled land) and out-of-range pixels, enough of each, and valid pixels in at least three layers."""
    from mops_amd import engine
    path, w, h, n_attr, with_normals = CASES[key]
    ref = _reference(case, key)
    code = ref["code"]
    if key in ("two_37x20", "three_65x3"):
        _assert_coverage(code)
        assert (code == RR.OUTSIDE).any() and (code == RR.OUT_OF_RANGE).any()
        assert len(np.unique(ref["layer"][code == RR.VALID])) >= 3
    assert (code == RR.VALID).any()
    kw = dict(vertex_attrs=case["vattrs"][:n_attr], return_cells=True)
    if with_normals:
        images, dist, cells = engine.remap_section(case["dm"], case["df"], path, w, h, case["drange"], **kw)
        assert dist.tobytes() == ref["dist"].tobytes()
    else:
        images, dist, cells = engine.remap_section(case["dm"], case["df"], None, w, h, case["drange"],
                                                   columns=(ref["pts"], None), **kw)
    got = images.cpu().numpy()
    assert got.shape == ref["images"].shape == ((2 if n_attr else 1), h, w, 4)
    assert np.array_equal(cells.cpu().numpy(), ref["cells"])
    for k in range(got.shape[0]):
        assert np.array_equal(got[k], ref["images"][k], equal_nan=True), (key, k)
    assert np.all(got[..., 3] == 1.0)
    valid = code == RR.VALID
    if with_normals:
        assert np.abs(got[0][..., 2][valid]).max() > 1e-4      # the across channel is not idle
    else:
        assert np.all(got[0][..., 2][valid] == 0.0)
    if n_attr:
        assert np.isfinite(got[1][valid]).all() and np.abs(got[1][..., 0][valid]).max() > 1.0
        assert np.isnan(got[1][~valid][:, :3]).all()
        if n_attr == 1:
            assert np.all(got[1][..., 1][valid] == 0.0)
        else:
            assert np.abs(got[1][..., 1][valid]).max() > 0.1


def test_default_depth_range_is_the_reference_bottom_depths(case):
    from mops_amd import engine
    path, w, h, _, _ = CASES["three_65x3"]
    a, _ = engine.remap_section(case["dm"], case["df"], path, w, h)
    b, _ = engine.remap_section(case["dm"], case["df"], path, w, h, case["drange"])
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("key", ["me12", "me20"])
def test_section_across_wide_cells(engine_lib, oracle_lib, gpu, key):
    """The MAXV 12 and 20 instantiations: sections through the centres of the wheels of the Voronoi wheel
    meshes, whose cells of 8 to 20 vertices are alive."""
    from mops_amd import engine
    mesh, s0, _ = WC.world(key)
    d = WC.derived(key)[0]
    drange = WC.depth_range(mesh)
    names = sorted(d.attrs)[:2]
    dm = engine.DeviceMesh.from_mesh(mesh)
    df = engine.DeviceField.from_snapshot(dm, s0)
    va = tuple(engine.cell_to_vertex_attr(dm, s0.attributes[k]) for k in names)
    seen = {}
    for path, w, h in (([(0.0, -160.0), (0.0, -120.0)], 41, 7),
                       ([(-37.0, -128.0), (-33.0, -88.0), (27.0, -50.0), (23.0, -15.0)], 61, 7)):
        pts, nrm, dist = SR.section_points(path, w)
        cells = oracle_lib.knn(mesh, pts)
        ref = SR.section(mesh, d, pts, nrm, h, drange, cells, attrs=[d.attrs[k] for k in names])
        _assert_coverage(ref["code"])
        for deg, n in WC.valid_by_degree(mesh, cells, ref["code"]).items():
            seen[deg] = seen.get(deg, 0) + n
        images, gdist, gcells = engine.remap_section(dm, df, path, w, h, drange, vertex_attrs=va, return_cells=True)
        assert np.array_equal(gcells.cpu().numpy(), cells) and gdist.tobytes() == dist.tobytes()
        assert np.array_equal(images.cpu().numpy(), ref["images"], equal_nan=True), (key, path)
    wide = {deg: n for deg, n in seen.items() if deg > (7 if key == "me12" else 12) and n > 0}
    assert max(seen) == WC.MAX_EDGES[key] and seen[max(seen)] >= 10 and len(wide) >= 2, seen


def test_refusal_leaves_the_outputs_untouched(case):
    """A field of another mesh is refused before any launch (the other refusals need no device:
    test_section_cpu.py)."""
    import torch
    from mops_amd import _lib, engine
    other = engine.DeviceMesh.from_mesh(case["mesh"])
    pts = np.ascontiguousarray(_reference(case, "two_37x20")["pts"])
    img = torch.full((20, 37, 4), 7.0, dtype=torch.float64, device="cuda")
    cells = torch.full((37,), -5, dtype=torch.int32, device="cuda")
    st = _lib.load().mops_remap_section(
        other.handle, case["df"].handle, 37, 20, 0.0, 4000.0, pts.ctypes.data_as(C.c_void_p), None, 0, None, None,
        C.c_void_p(img.data_ptr()), None, C.c_void_p(cells.data_ptr()), None)
    assert st == _lib.MOPS_ERR_INVALID and b"another mesh" in _lib.load().mops_last_error()
    torch.cuda.synchronize()
    assert bool((img == 7.0).all()) and bool((cells == -5).all())
    with pytest.raises(ValueError):
        engine.remap_section(case["dm"], case["df"], TWO, 37, 20, case["drange"], vertex_attrs=case["vattrs"] * 2)
    with pytest.raises(ValueError):
        engine.remap_section(case["dm"], case["df"], TWO, 37, 20, (0.0, float("nan")))


@pytest.mark.parametrize("n_attr", [0, 1, 2])
def test_pymops_section_end_to_end(case, n_attr):
    mesh, snap = case["mesh"], case["snap"]
    M = _pymops(mesh, snap, case["names"][:n_attr])
    key = {0: "two_no_attr_no_normals", 1: "two_one_attr", 2: "two_37x20"}[n_attr]
    path, w, h, _, _ = CASES[key]
    ref = _reference(case, "two_37x20" if n_attr == 2 else "two_one_attr")
    cfg = M.VisualizationSettings()
    assert cfg.SectionPath == [] and cfg.DepthRange == (0.0, 0.0)
    cfg.imageSize = (w, h)
    assert M.MOPS_RunRemappingSection(cfg) == []          # no path: Error() and an empty list
    cfg.SectionPath = [path[0]]
    assert M.MOPS_RunRemappingSection(cfg) == []
    cfg.SectionPath = list(path)
    imgs = M.MOPS_RunRemappingSection(cfg)                 # DepthRange (0, 0): the reference bottom depths
    assert isinstance(imgs, list) and len(imgs) == (2 if n_attr else 1)
    assert all(a.shape == (h, w, 4) and a.dtype == np.float64 for a in imgs)
    assert np.array_equal(imgs[0], ref["images"][0], equal_nan=True)
    if n_attr == 1:
        assert np.array_equal(imgs[1], ref["images"][1], equal_nan=True)
    if n_attr == 2:
        assert np.array_equal(imgs[1], ref["images"][1], equal_nan=True)
    cfg.DepthRange = case["drange"]
    again = M.MOPS_RunRemappingSection(cfg)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(imgs, again))
    sv = M.MOPS_SectionTransport(imgs[0], cfg)
    want, area = SR.transport(ref["images"][0], ref["dist"], case["drange"])
    assert sv == want and area > 0.0 and abs(sv) > 1e-3
    cfg.imageSize = (0, h)
    assert M.MOPS_RunRemappingSection(cfg) == [] and np.isnan(M.MOPS_SectionTransport(imgs[0], cfg))


def test_section_cpp_driver_equals_the_python_path(case, tmp_path):
    """tests/cpp/section_api.cpp, compiled against the engine library: MOPS::MOPS_RunRemappingSection's images
    are the Python path's bytes, its PNGs decode to the Python path's pixels, and MOPS::MOPS_SectionTransport is
    the Python value bit for bit."""
    from mops_amd import engine, pyMOPS as M
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    mesh, s0 = case["mesh"], case["snap"]
    exe = os.path.join(str(tmp_path), "section_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "section_api.cpp"), "-L" + libdir, "-lmops_traj",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    path, w, h, _, _ = CASES["two_37x20"]
    names = case["names"][:2]
    d = str(tmp_path)
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{mesh.nCells} {mesh.nVertices} {mesh.maxEdges} {mesh.nVertLevels} {len(names)} {w} {h} {len(path)} "
                + " ".join(f"{lat!r} {lon!r}" for lat, lon in path) + "\n")
    arrays = dict(nEdgesOnCell=mesh.nEdgesOnCell, verticesOnCell=mesh.verticesOnCell, cellsOnCell=mesh.cellsOnCell,
                  cellsOnVertex=mesh.cellsOnVertex, cellCoord=mesh.cellCoord, vertexCoord=mesh.vertexCoord,
                  layerThickness=s0.layerThickness, bottomDepth=s0.bottomDepth, zonal=s0.zonalVelocity,
                  meridional=s0.meridionalVelocity, vvel=s0.vertVelocityTop, refBottomDepth=mesh.refBottomDepth)
    arrays.update({f"attr_{k}": s0.attributes[n] for k, n in enumerate(names)})
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        (a.astype(np.uint64) if a.dtype.kind in "iu" else a.astype(np.float64)).tofile(os.path.join(d, k))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    images, dist = engine.remap_section(case["dm"], case["df"], path, w, h, vertex_attrs=case["vattrs"])
    host = images.cpu().numpy()
    ref = _reference(case, "two_37x20")
    assert np.array_equal(host, ref["images"], equal_nan=True)
    for i in range(2):
        got = np.fromfile(os.path.join(d, f"section_{i}.f64"), dtype=np.float64).reshape(h, w, 4)
        assert got.tobytes() == host[i].tobytes()
    for i, ch in ((0, 0), (0, 1), (0, 2), (1, 0)):
        name = os.path.join(d, f"py_{i}_ch{ch}.png")
        assert M.SaveToPNG(images[i], name, ch)
        assert np.array_equal(IR.decode_png(os.path.join(d, f"section_{i}_ch{ch}.png")), IR.decode_png(name))
    n_img, sv_hex, n_bad, sv_bad = open(os.path.join(d, "summary.txt")).read().split()
    sv, _ = engine.section_transport(host[0], dist, case["drange"])
    assert (n_img, n_bad, sv_bad) == ("2", "0", "nan")
    assert float.fromhex(sv_hex) == sv == SR.transport(ref["images"][0], ref["dist"], case["drange"])[0]


def test_cli_section_stage(engine_lib, gpu, tmp_path, monkeypatch, capsys):
    """``--section`` writes the section's files beside the remapping stage's and prints the transport; without
    it the stage writes what it wrote before.  The stages are run at a small image size (the CLI's own sizes are
    its constants); the option itself is parsed on the CPU below."""
    from test_mpas_reader import YAML, _mesh, _write_hist, _write_mesh
    from mops_amd import cli, engine, io as mio, pyMOPS as M
    mesh, snaps = _mesh()
    _write_mesh(str(tmp_path / "mesh.nc"), mesh, 2)
    _write_hist(str(tmp_path / "hist.am.timeSeriesStatsMonthly.0001-01-01.nc"), mesh, snaps[:2], 2, 1)
    y = tmp_path / "mpas.yaml"
    y.write_text(YAML.format(prefix=str(tmp_path)))
    args = cli.parse_command_line(["-i", str(y), "-t", "1", "--section", "-30,-20;50,80", "--vti"])
    assert args.section == TWO and args.vti
    assert cli.parse_command_line(["-i", str(y)]).section is None
    for bad in ("-30,-20", "1,2;3", "a,b;c,d", ""):
        assert cli.parse_command_line(["-i", str(y), "--section", bad]) is None
    M.MOPS_Init("gpu")
    grid = M.MPASOGrid()
    grid.init_from_yaml(str(y))
    sol = M.MPASOSolution()
    sol.init_from_yaml(str(y), "", 1)
    for k in ("temperature", "salinity"):   # (the history fixture carries no tracers)
        sol.add_attribute(k, snaps[1].attributes[k])
    M.MOPS_Begin()
    M.MOPS_AddGridMesh(grid)
    M.MOPS_AddAttribute(1, sol)
    M.MOPS_End()
    M.MOPS_ActiveAttribute(1)
    before = tmp_path / "before"
    before.mkdir()
    monkeypatch.chdir(before)
    base = cli.run_remapping_stage(M, mio, 1, 150.0, vti=True, width=48, height=24)
    assert sorted(os.listdir(before)) == sorted(base)
    assert sorted(base) == sorted([f"output_{i}_ch{c}.png" for i in range(2) for c in range(3)]
                                  + ["timestep_1_tile_0_fixed_depth_150.000000.vti"])
    after = tmp_path / "after"
    after.mkdir()
    monkeypatch.chdir(after)
    base2 = cli.run_remapping_stage(M, mio, 1, 150.0, vti=True, width=48, height=24)
    capsys.readouterr()
    written, sv = cli.run_section_stage(M, mio, 1, args.section, vti=True, width=37, height=20)
    out = capsys.readouterr().out
    assert base2 == base and sorted(os.listdir(after)) == sorted(base + written)
    assert sorted(written) == sorted([f"section_output_{i}_ch{c}.png" for i in range(2) for c in range(3)]
                                     + ["section_timestep_1_tile_0_fixed_depth_0.000000.vti"])
    for name in base:   # the stage's own files are the bytes they were
        assert (after / name).read_bytes() == (before / name).read_bytes()
    assert f"transport {sv:.6f} Sv" in out and np.isfinite(sv)
    images, dist = engine.remap_section(M._app.mesh, M._app.front, args.section, 37, 20,
                                        (float(mesh.refBottomDepth[0]), float(mesh.refBottomDepth[-1])),
                                        vertex_attrs=tuple(M._vertex_attr(1, k) for k in ("salinity", "temperature")))
    host = images.cpu().numpy()
    assert np.isfinite(host[0, ..., 2]).any() and np.isnan(host[0, ..., 2]).any()
    for i in range(2):
        for ch in range(3):
            assert np.array_equal(IR.decode_png(str(after / f"section_output_{i}_ch{ch}.png")),
                                  IR.save_to_png_rgba(host[i, ..., ch])[0])
    v = IR.read_vti(str(after / "section_timestep_1_tile_0_fixed_depth_0.000000.vti"))
    assert len(v["arrays"]) == 6 and v["arrays"][2][0] == "Across-section Velocity"
    assert np.array_equal(v["arrays"][2][2], host[0, ::-1, :, 2], equal_nan=True)
    assert sv == engine.section_transport(host[0], dist, (float(mesh.refBottomDepth[0]),
                                                           float(mesh.refBottomDepth[-1])))[0]
