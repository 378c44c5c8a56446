"""The image path on the GPU: the colour-mapping kernels (engine.colormap_rgba) byte for byte and the fixed-layer
remapping (engine.remap_fixed_layer) bit for bit against the restatements of tests/image_reference.py, then the
pyMOPS entries and the CLI's remapping stage on top of them."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_reference as IR  # noqa: E402
import remap_reference as RR  # noqa: E402
from test_remap_gpu import CASES, _pymops  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colormap_reference.npz")
LAYERS = ((0, 0), (4, 4), (2.9, 2), (-3, 0), (99, 9))  # FixedLayer -> the layer ClampLayer gives with 10 levels


@pytest.fixture(scope="module")
def case(engine_lib, oracle_lib, gpu, small_case):
    from mops_amd import engine
    mesh, s0, _ = small_case
    dm = engine.DeviceMesh.from_mesh(mesh)
    df = engine.DeviceField.from_snapshot(dm, s0)
    names = sorted(s0.attributes)
    vattrs = tuple(engine.cell_to_vertex_attr(dm, s0.attributes[k]) for k in names[:2])
    return dict(mesh=mesh, snap=s0, dm=dm, df=df, derived=oracle_lib.preprocess(mesh, s0), names=names, vattrs=vattrs,
                O=oracle_lib, cache={})


def _assert_coverage(rgba):
    """At least 5 % transparent and at least 40 % opaque pixels, by the restatement's own output."""
    n = rgba.shape[0] * rgba.shape[1]
    opaque = int((rgba[..., 3] == 255).sum())
    assert opaque >= 0.4 * n and n - opaque >= 0.05 * n, (opaque, n)


def _check(image, channels=(0, 1, 2, 3), coverage=()):
    """engine.colormap_rgba of a host or device image [H, W, 4] against the restatement, channel by channel."""
    import torch
    from mops_amd import engine
    dev = image if isinstance(image, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(image)).cuda()
    host = dev.cpu().numpy()
    got, mm = engine.colormap_rgba(dev, channels=channels, return_minmax=True)
    assert got.shape == (len(channels),) + host.shape and got.dtype == torch.uint8 and got.is_cuda
    assert mm.shape == (len(channels), 2) and mm.dtype == np.float32
    got = got.cpu().numpy()
    refs = []
    for k, c in enumerate(channels):
        ref, (mn, mx) = IR.save_to_png_rgba(host[..., c])
        if c in coverage:
            _assert_coverage(ref)
        assert np.array_equal(mm[k], np.array([mn, mx], dtype=np.float32)), (c, mm[k], mn, mx)
        assert np.array_equal(got[k], ref), (c, int((got[k] != ref).sum()))
        refs.append(ref)
    return refs


def test_colormap_golden_inputs(engine_lib, gpu):
    """The four golden channels side by side in one image each: the kernel's bytes are the reference's own."""
    g = np.load(GOLDEN)
    for name in ("normal_nan", "constant", "all_nan", "subfloat"):
        a = g[name + "_in"]
        img = np.stack([a, -a, a * 3.0 + 1.0, np.ones_like(a)], axis=-1)
        refs = _check(img, coverage=(0, 1, 2) if name == "normal_nan" else ())
        assert np.array_equal(refs[0], g[name + "_rgba"])


def test_colormap_single_pixel(engine_lib, gpu):
    _check(np.array([[[2.5, np.nan, -7.0, 1.0]]]))


def test_colormap_odd_size(engine_lib, gpu):
    """37 x 23 = 851 pixels: no multiple of 64, one block of the range pass."""
    rng = np.random.default_rng(3)
    img = rng.standard_normal((23, 37, 4)) * np.array([1.0, 1e-3, 1e6, 1.0])
    img[rng.random((23, 37)) < 0.10] = np.nan
    _check(img, coverage=(0, 1, 2, 3))
    _check(img, channels=(1, 3))  # a channel subset: planes in ascending channel order


def test_colormap_several_blocks_and_rounds(engine_lib, gpu):
    """300 x 70 = 21 000 pixels: 21 blocks of the range pass, each with several grid-stride rounds, so the
    partial reduction decides the range.  The extremes sit where only the last block reads them: the maximum in
    its first round (pixel 20 * 256 + 5), the minimum in its third (two grid strides of 21 * 256 later); channel 1
    has its extremes in the image's last two pixels."""
    rng = np.random.default_rng(4)
    h, w = 70, 300
    img = rng.standard_normal((h, w, 4))
    img[rng.random((h, w)) < 0.10] = np.nan
    flat = img.reshape(-1, 4)
    flat[20 * 256 + 5, 0] = 50.0
    flat[20 * 256 + 5 + 2 * 21 * 256, 0] = -60.0
    flat[-1, 1], flat[-2, 1] = 70.0, -80.0
    _check(img, coverage=(0, 1, 2, 3))
    assert IR.save_to_png_rgba(img[..., 0])[1] == (-60.0, 50.0) and IR.save_to_png_rgba(img[..., 1])[1] == (-80.0, 70.0)


@pytest.mark.parametrize("key", ["global_800", "box_0"])
def test_colormap_of_remapped_images_on_the_device(case, key):
    """Both fixed-depth images coloured where the kernel wrote them; channel 3 is all 1.0 (min >= max)."""
    from mops_amd import engine
    w, h, (lat, lon), depth = CASES[key]
    images = engine.remap_fixed_depth(case["dm"], case["df"], w, h, lat, lon, depth, n_attr=2,
                                      vertex_attrs=case["vattrs"])
    nan = int(np.isnan(images[0, ..., 0].cpu().numpy()).sum())
    assert nan == {"global_800": 1152 - 1055, "box_0": 1280 - 633}[key]
    for k in range(2):
        refs = _check(images[k], coverage=(0, 1, 2))
        assert (refs[0][..., 3] == 0).sum() == nan
        alpha = refs[3]  # channel 3: every pixel 1.0 -> max = 1 + 1e-5f, norm 0, table entry 0
        assert np.array_equal(alpha, np.broadcast_to(alpha[0, 0], alpha.shape)) and alpha[0, 0, 3] == 255


def test_colormap_rejects_bad_input(engine_lib, gpu):
    import torch
    from mops_amd import engine
    img = torch.zeros((4, 5, 4), dtype=torch.float64, device="cuda")
    for bad in ((), (4,), (1, 0), (2, 2)):
        with pytest.raises(ValueError):
            engine.colormap_rgba(img, channels=bad)
    with pytest.raises(ValueError):
        engine.colormap_rgba(img.float())


# ---- fixed layer ------------------------------------------------------------------------------------------
def _layer_reference(c, key, layer):
    k = (key, layer)
    if k not in c["cache"]:
        w, h, (lat, lon), _ = CASES[key]
        if ("cells", key) not in c["cache"]:
            c["cache"][("cells", key)] = c["O"].knn(c["mesh"], RR.depth_positions(w, h, lat, lon))
        c["cache"][k] = IR.fixed_layer(c["mesh"], c["derived"], w, h, lat, lon, layer, c["cache"][("cells", key)])
    return c["cache"][k]


@pytest.mark.parametrize("key", ["global_800", "box_0"])
def test_fixed_layer_bit_exact(case, key):
    from mops_amd import engine
    w, h, (lat, lon), _ = CASES[key]
    outside = {"global_800": 92, "box_0": 82}[key]
    for value, want_layer in LAYERS:
        ref = _layer_reference(case, key, value)
        assert ref["layer"] == want_layer
        assert int((ref["code"] == RR.OUTSIDE).sum()) == outside and int((ref["code"] == RR.VALID).sum()) == w * h - outside
        image, cells = engine.remap_fixed_layer(case["dm"], case["df"], w, h, lat, lon, value, return_cells=True)
        got = image.cpu().numpy()
        assert got.shape == (h, w, 4) and cells.shape == (h, w)
        assert np.array_equal(cells.cpu().numpy().reshape(-1), case["cache"][("cells", key)])
        assert np.array_equal(got, ref["image"], equal_nan=True), (key, value)
        assert np.all(got[..., 3] == 1.0) and int(np.isnan(got[..., 0]).sum()) == outside
        assert np.all(got[..., 2][ref["code"] == RR.VALID] == 0.0)
    a, b = _layer_reference(case, key, 0)["image"], _layer_reference(case, key, 4)["image"]
    ok = _layer_reference(case, key, 0)["code"] == RR.VALID
    assert np.isfinite(a[ok]).all() and np.isfinite(b[ok]).all() and (a[ok][:, :2] != b[ok][:, :2]).any()
    assert np.array_equal(_layer_reference(case, key, 2.9)["image"], _layer_reference(case, key, 2)["image"],
                          equal_nan=True)


# ---- pyMOPS -----------------------------------------------------------------------------------------------
def test_pymops_images(case, tmp_path):
    """SaveToPNG of a MOPS_RunRemapping image (host array and device tensor alike) decodes to the restatement's
    RGBA; MOPS_RunRemappingFixedLayer is engine.remap_fixed_layer; VisType = kFixedLayer leaves MOPS_RunRemapping
    fixed-depth (MOPSApp.cpp:192)."""
    import torch
    from mops_amd import engine
    M = _pymops(case["mesh"], case["snap"], case["names"][:2])
    key = "global_800"
    w, h, (lat, lon), depth = CASES[key]
    cfg = M.VisualizationSettings()
    cfg.imageSize = (w, h)
    cfg.LatRange, cfg.LonRange = lat, lon
    cfg.FixedDepth = depth
    imgs = M.MOPS_RunRemapping(cfg)
    want = engine.remap_fixed_depth(case["dm"], case["df"], w, h, lat, lon, depth, n_attr=2,
                                    vertex_attrs=case["vattrs"]).cpu().numpy()
    assert len(imgs) == 2 and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(imgs, want))
    for ch in (0, 1, 3):
        ref, _ = IR.save_to_png_rgba(imgs[0][..., ch])
        p = str(tmp_path / f"h{ch}.png")
        assert M.SaveToPNG(imgs[0], p, ch) is True
        assert np.array_equal(IR.decode_png(p), ref)
        assert M.SaveToPNG(torch.as_tensor(imgs[0]).cuda(), p, ch) is True
        assert np.array_equal(IR.decode_png(p), ref)
    _assert_coverage(IR.save_to_png_rgba(imgs[0][..., 0])[0])
    assert M.SaveToPNG(imgs[0], str(tmp_path / "bad.png"), 4) is False and not (tmp_path / "bad.png").exists()
    # kFixedLayer changes nothing in MOPS_RunRemapping: FixedLayer and FixedDepth are one double
    cfg.VisType = M.VisualizeType.kFixedLayer
    again = M.MOPS_RunRemapping(cfg)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again, want))
    cfg.FixedLayer = 4
    got = M.MOPS_RunRemappingFixedLayer(cfg)
    layer = engine.remap_fixed_layer(case["dm"], case["df"], w, h, lat, lon, 4).cpu().numpy()
    assert got.shape == (h, w, 4) and got.dtype == np.float64 and np.array_equal(got, layer, equal_nan=True)
    assert np.array_equal(got, _layer_reference(case, key, 4)["image"], equal_nan=True)


# ---- CLI --------------------------------------------------------------------------------------------------
def _write_hist_with_tracers(path, mesh, snaps):
    """test_mpas_reader._write_hist's file plus the two tracers (that dataset has none, so its solution has no
    double attribute and one image only): two attributes make MOPS_RunRemapping return two images."""
    from scipy import io as scipy_io
    C, L = mesh.nCells, mesh.nVertLevels
    f = scipy_io.netcdf_file(path, "w", version=2)
    f.createDimension("Time", None); f.createDimension("nCells", C)
    f.createDimension("nVertLevels", L); f.createDimension("nVertLevelsP1", L + 1); f.createDimension("StrLen", 64)
    xt = f.createVariable("xtime_startMonthly", "c", ("Time", "StrLen"))
    cell = {k: f.createVariable("timeMonthly_avg_" + k, "d", ("Time", "nCells", "nVertLevels"))
            for k in ("layerThickness", "velocityZonal", "velocityMeridional", "activeTracers_temperature",
                      "activeTracers_salinity")}
    vv = f.createVariable("timeMonthly_avg_vertVelocityTop", "d", ("Time", "nCells", "nVertLevelsP1"))
    bd = f.createVariable("bottomDepth", "d", ("nCells",))
    bd[:] = snaps[0].bottomDepth
    for t, s in enumerate(snaps):
        xt[t] = np.frombuffer(f"{1 + t:04d}-01-01_00:00:00".ljust(64).encode(), dtype="S1")
        cell["layerThickness"][t] = s.layerThickness.reshape(C, L)
        cell["velocityZonal"][t] = s.zonalVelocity.reshape(C, L)
        cell["velocityMeridional"][t] = s.meridionalVelocity.reshape(C, L)
        cell["activeTracers_temperature"][t] = np.asarray(s.attributes["temperature"]).reshape(C, L)
        cell["activeTracers_salinity"][t] = np.asarray(s.attributes["salinity"]).reshape(C, L)
        vv[t] = s.vertVelocityTop.reshape(C, L + 1)
    f.close()


def test_cli_writes_the_remapped_images(engine_lib, gpu, tmp_path, monkeypatch, capsys):
    """A CLI run with --vti on the test_mpas_reader dataset (with its snapshots' two tracers in the history file):
    six 3601 x 1801 PNGs, output_0_ch0.png equal to the restatement on MOPS_RunRemapping's image 0 channel 0, and
    the VTI's six arrays under the reference's names."""
    from test_mpas_reader import YAML, _mesh, _write_mesh
    from mops_amd import cli, pyMOPS as M
    mesh, snaps = _mesh()
    _write_mesh(str(tmp_path / "mesh.nc"), mesh, 2)
    _write_hist_with_tracers(str(tmp_path / "hist.am.timeSeriesStatsMonthly.0001-01-01.nc"), mesh, snaps[:2])
    y = tmp_path / "mpas.yaml"
    tracer = ("        - name: temperature\n"
              "          possible_names: [temperature, timeMonthly_avg_activeTracers_temperature]\n"
              "          optional: true\n")
    assert "        - name: salinity\n" in YAML
    y.write_text(YAML.replace("        - name: salinity\n", tracer + "        - name: salinity\n").format(
        prefix=str(tmp_path)))
    monkeypatch.chdir(tmp_path)
    t0 = time.perf_counter()
    assert cli.main(["-i", str(y), "-t", "1", "-d", "150", "-g", "1", "--vti"]) == 0
    t_cli = time.perf_counter() - t0
    out = capsys.readouterr().out
    assert "skipped" not in out and "output_1_ch2.png" in out
    assert (tmp_path / "traj_line_1.txt").stat().st_size > 0
    W, H = 3601, 1801
    cfg = M.VisualizationSettings()
    cfg.imageSize = (W, H)
    cfg.LatRange, cfg.LonRange = (-90.0, 90.0), (-180.0, 180.0)
    cfg.FixedDepth = 150.0
    imgs = M.MOPS_RunRemapping(cfg)  # timestep 1 is still active
    assert len(imgs) == 2 and imgs[0].shape == (H, W, 4)
    for i in range(2):
        for ch in range(3):
            rgba = IR.decode_png(str(tmp_path / f"output_{i}_ch{ch}.png"))
            assert rgba.shape == (H, W, 4)
            if (i, ch) == (0, 0):
                ref, _ = IR.save_to_png_rgba(imgs[0][..., 0])
                assert np.array_equal(rgba, ref)
                assert (ref[..., 3] == 0).any() and (ref[..., 3] == 255).any()
    name = "timestep_1_tile_0_fixed_depth_150.000000.vti"
    v = IR.read_vti(str(tmp_path / name))
    assert [n for n, _, _ in v["arrays"]] == ["E: Zonal Velocity", "N: Meridional Velocity", "Velocity Magnitude",
                                              "Temperature", "Salinity", "None"]
    assert v["extent"] == [0, W - 1, 0, H - 1, 0, 0] and v["origin"] == [-180.0, -90.0, 150.0]
    assert v["spacing"] == [360.0 / (W - 1), 180.0 / (H - 1), 1.0]
    assert np.array_equal(v["arrays"][0][2], imgs[0][::-1, :, 0], equal_nan=True)
    assert np.array_equal(v["arrays"][3][2], imgs[1][::-1, :, 0], equal_nan=True)  # "Temperature" holds salinity (Q16)
    print(f"cli run {t_cli:.2f} s, whole test {time.perf_counter() - t0:.2f} s")
