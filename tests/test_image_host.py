"""Image output without a GPU: the colour-map restatement against the reference's own SaveToPNG output
(tests/golden/colormap_reference.npz), the PNG and VTI writers against the readers of tests/image_reference.py,
and the VTI file name."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_reference as IR  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colormap_reference.npz")
GOLDEN_CASES = ("normal_nan", "constant", "all_nan", "subfloat")


def test_viridis_header_is_the_published_table():
    t = IR.viridis_table()
    assert t.shape == (256, 3) and t.min() >= 0.0 and t.max() < 1.0
    assert t[0].tolist() == [0.267004, 0.004874, 0.329415] and t[255].tolist() == [0.993248, 0.906157, 0.143936]


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_restatement_reproduces_the_reference_png(name):
    g = np.load(GOLDEN)
    rgba, (mn, mx) = IR.save_to_png_rgba(g[name + "_in"])
    assert rgba.dtype == np.uint8 and np.array_equal(rgba, g[name + "_rgba"])
    assert mn.dtype == np.float32 and mx.dtype == np.float32
    assert mx > mn or name == "all_nan"  # FLT_MAX + 1e-5f is FLT_MAX


def test_golden_cases_are_what_they_claim():
    g = np.load(GOLDEN)
    a = g["normal_nan_in"]
    assert a.shape == (23, 37) and 0.05 < np.isnan(a).mean() < 0.15
    assert (g["normal_nan_rgba"][..., 3] == 0).sum() == np.isnan(a).sum()
    assert len(np.unique(g["normal_nan_rgba"].reshape(-1, 4), axis=0)) > 100
    assert np.unique(g["constant_in"]).size == 1 and np.unique(g["constant_rgba"].reshape(-1, 4), axis=0).shape[0] == 1
    assert np.isnan(g["all_nan_in"]).all() and not g["all_nan_rgba"].any()
    s = g["subfloat_in"]
    assert np.unique(s).size == s.size and np.unique(s.astype(np.float32)).size == 1
    assert np.array_equal(g["subfloat_rgba"], np.broadcast_to(g["subfloat_rgba"][0, 0], s.shape + (4,)))


def _chunk(typ, body):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) & 0xFFFFFFFF)


def test_decoder_undoes_all_five_filters():
    """A PNG filtered here with every filter type (rows cycle through 0..4) decodes to the pixels."""
    rng = np.random.default_rng(1)
    h, w = 11, 7
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    rows = px.reshape(h, w * 4).astype(np.int64)
    raw = bytearray()
    for r in range(h):
        ft = r % 5
        cur, up = rows[r], rows[r - 1] if r else np.zeros(w * 4, dtype=np.int64)
        left = np.concatenate([np.zeros(4, dtype=np.int64), cur[:-4]])
        upleft = np.concatenate([np.zeros(4, dtype=np.int64), up[:-4]])
        pred = [np.zeros_like(cur), left, up, (left + up) >> 1,
                np.array([IR._paeth(int(a), int(b), int(c)) for a, b, c in zip(left, up, upleft)])][ft]
        raw.append(ft)
        raw += bytes(((cur - pred) & 255).astype(np.uint8))
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(bytes(raw), 6)) + _chunk(b"IEND", b""))
    assert np.array_equal(IR.decode_png(png), px)
    bad = bytearray(png)
    bad[40] ^= 1
    with pytest.raises(AssertionError):
        IR.decode_png(bytes(bad))


@pytest.mark.parametrize("w,h", [(1, 1), (37, 23), (300, 70)])
def test_png_writer_round_trip(engine_lib, tmp_path, w, h):
    """mops_write_png_rgba8 -> decode_png (CRCs verified, zlib's inflate checks the Adler-32): the pixels;
    300 x 70 needs two stored blocks (84 070 filtered bytes > 65 535)."""
    from mops_amd import io as mio
    px = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 4), dtype=np.uint8)
    p = str(tmp_path / "a.png")
    mio.write_png_rgba8(p, px)
    data = open(p, "rb").read()
    assert np.array_equal(IR.decode_png(data), px)
    # signature, IHDR, exactly one IDAT of stored blocks, IEND
    raw = h * (1 + 4 * w)
    blocks = (raw + 65534) // 65535
    assert len(data) == 8 + (12 + 13) + (12 + 2 + 5 * blocks + raw + 4) + 12
    assert data.count(b"IDAT") >= 1 and data[37:41] == b"IDAT" and data[41:43] == b"\x78\x01"
    assert blocks == (2 if (w, h) == (300, 70) else 1)


def test_png_writer_rejects_bad_arguments(engine_lib, tmp_path):
    from mops_amd import _lib
    a = np.zeros(4, dtype=np.uint8)
    assert engine_lib.mops_write_png_rgba8(str(tmp_path / "x.png").encode(), 0, 1, a.ctypes.data) == _lib.MOPS_ERR_INVALID
    assert engine_lib.mops_write_png_rgba8(str(tmp_path / "no" / "x.png").encode(), 1, 1, a.ctypes.data) \
        == _lib.MOPS_ERR_INVALID
    assert engine_lib.mops_colormap_rgba8(None, 4, 4, 1, None, None, None) == _lib.MOPS_ERR_INVALID
    assert engine_lib.mops_colormap_image(a.ctypes.data, 1, 1, 16, a.ctypes.data, None, None) == _lib.MOPS_ERR_INVALID


def _images():
    rng = np.random.default_rng(7)
    img = rng.standard_normal((2, 3, 5, 4))  # 2 images of 5 x 3 (W x H)
    img[..., 3] = 1.0
    img[0, 1, 2, :3] = np.nan
    img[1, 0, 4, 1] = np.nan
    return img


def test_vti_writer_round_trip(engine_lib, tmp_path):
    from mops_amd import io as mio
    img = _images()
    p = str(tmp_path / "m.vti")
    names = ["E: Zonal Velocity", "N: Meridional <&> \"Velocity\"", "Velocity Magnitude", "Temperature"]
    mio.save_images_vti(p, img, (-180.0, -90.0, 10.0), (0.1, 0.25, 1.0), names)
    v = IR.read_vti(p)
    assert v["extent"] == [0, 4, 0, 2, 0, 0] and v["origin"] == [-180.0, -90.0, 10.0] and v["spacing"] == [0.1, 0.25, 1.0]
    assert [n for n, _, _ in v["arrays"]] == names + ["attr_4", "attr_5"] and v["scalars"] is None
    for i, (_, nc, a) in enumerate(v["arrays"]):
        assert nc == 1 and a.shape == (3, 5)
        assert np.array_equal(a, img[i // 3, ::-1, :, i % 3], equal_nan=True), i  # VTK row i = image row H - 1 - i
    assert np.isnan(v["arrays"][0][2][1, 2]) and np.isnan(v["arrays"][4][2][2, 4])
    # a list of images is the same file
    mio.save_images_vti(str(tmp_path / "l.vti"), [img[0], img[1]], (-180.0, -90.0, 10.0), (0.1, 0.25, 1.0), names)
    assert open(str(tmp_path / "l.vti"), "rb").read() == open(p, "rb").read()


def test_vti_single_image_variant(engine_lib, tmp_path):
    from mops_amd import io as mio
    img = _images()[0]
    p = str(tmp_path / "s.vti")
    mio.save_image_vti(p, img, (1.0, 2.0, 3.0), (0.5, 0.5, 3.0))
    v = IR.read_vti(p)
    assert v["scalars"] == "ImageScalars" and len(v["arrays"]) == 1 and v["spacing"] == [0.5, 0.5, 3.0]
    name, nc, a = v["arrays"][0]
    assert (name, nc) == ("ImageScalars", 3) and np.array_equal(a, img[::-1, :, :3], equal_nan=True)


def test_save_vti_names_and_geometry(engine_lib, tmp_path, monkeypatch):
    """pyMOPS.SaveVTI: outputName + "_" + TypeToStr + std::to_string(k) + ".vti", origin and spacing from the
    settings (VTKFileManager.hpp:86-95, :133)."""
    from mops_amd import pyMOPS as M
    monkeypatch.chdir(tmp_path)
    img = _images()
    cfg = M.VisualizationSettings()
    cfg.imageSize = (5, 3)
    cfg.LatRange, cfg.LonRange = (-60.0, 60.0), (-170.0, 150.0)
    cfg.FixedDepth = 10.0
    assert M.vti_file_name(cfg) == "output_fixed_depth_10.000000.vti"
    name = M.SaveVTI([img[0], img[1]], cfg, ["a", "b"], "timestep_3_tile_0")
    assert name == "timestep_3_tile_0_fixed_depth_10.000000.vti" and os.path.exists(name)
    v = IR.read_vti(name)
    assert v["origin"] == [-170.0, -60.0, 10.0] and v["spacing"] == [320.0 / 4, 120.0 / 2, 1.0]
    assert [n for n, _, _ in v["arrays"]] == ["a", "b", "attr_2", "attr_3", "attr_4", "attr_5"]
    cfg.VisType = M.VisualizeType.kFixedLayer
    cfg.FixedLayer = 2.5                       # the union: FixedDepth reads the same double
    assert cfg.FixedDepth == 2.5 and M.vti_file_name(cfg, "o") == "o_fixed_layer_2.500000.vti"
    single = M.SaveVTI(img[0], cfg)
    v = IR.read_vti(single)
    assert single == "output_fixed_layer_2.500000.vti" and v["spacing"][2] == 2.5 and v["arrays"][0][1] == 3
