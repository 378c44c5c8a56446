"""``MOPS_CLI --eddy``: the stage writes the vorticity / Okubo-Weiss image beside the remapping stage's files,
whose bytes stay what they were.  The stages are run at a small image size (the CLI's own sizes are its
constants); the option itself is parsed on the CPU (tests/test_eddy_cpu.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_reference as IR  # noqa: E402

pytestmark = pytest.mark.gpu


def test_cli_eddy_stage(engine_lib, gpu, tmp_path, monkeypatch, capsys):
    from test_mpas_reader import YAML, _mesh, _write_hist, _write_mesh
    from mops_amd import cli, engine, io as mio, pyMOPS as M
    mesh, snaps = _mesh()
    _write_mesh(str(tmp_path / "mesh.nc"), mesh, 2)
    _write_hist(str(tmp_path / "hist.am.timeSeriesStatsMonthly.0001-01-01.nc"), mesh, snaps[:2], 2, 1)
    y = tmp_path / "mpas.yaml"
    y.write_text(YAML.format(prefix=str(tmp_path)))
    args = cli.parse_command_line(["-i", str(y), "-t", "1", "--eddy", "--vti"])
    assert args.eddy and args.vti and not cli.parse_command_line(["-i", str(y)]).eddy
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
    w, h, depth = 48, 24, 150.0
    before = tmp_path / "before"
    before.mkdir()
    monkeypatch.chdir(before)
    base = cli.run_remapping_stage(M, mio, 1, depth, vti=True, width=w, height=h)
    assert sorted(os.listdir(before)) == sorted(base)
    after = tmp_path / "after"
    after.mkdir()
    monkeypatch.chdir(after)
    base2 = cli.run_remapping_stage(M, mio, 1, depth, vti=True, width=w, height=h)
    capsys.readouterr()
    written = cli.run_eddy_stage(M, mio, 1, depth, vti=True, width=w, height=h)
    out = capsys.readouterr().out
    assert "eddy images written" in out
    assert base2 == base and sorted(os.listdir(after)) == sorted(base + written)
    assert sorted(written) == sorted([f"eddy_output_0_ch{c}.png" for c in range(3)]
                                     + ["eddy_timestep_1_tile_0_fixed_depth_150.000000.vti"])
    for name in base:   # the stage's own files are the bytes they were
        assert (after / name).read_bytes() == (before / name).read_bytes()
    # the image is the engine's: image 1 of the fixed-depth remapping with the two signed vertex arrays
    g = engine.velocity_gradient(M._app.mesh, M._app.front, which=("vorticity", "okubo_weiss"), vertex=True)
    images = engine.remap_fixed_depth(M._app.mesh, M._app.front, w, h, (-90.0, 90.0), (-180.0, 180.0), depth,
                                      n_attr=2, vertex_attrs=(g["vorticity"], g["okubo_weiss"]))
    host = images[1].cpu().numpy()
    assert np.isfinite(host[..., 0]).any() and np.isnan(host[..., 0]).any()
    assert (host[..., 0] < 0).any() and (host[..., 0] > 0).any()
    for ch in range(3):
        assert np.array_equal(IR.decode_png(str(after / f"eddy_output_0_ch{ch}.png")),
                              IR.save_to_png_rgba(host[..., ch])[0])
    v = IR.read_vti(str(after / "eddy_timestep_1_tile_0_fixed_depth_150.000000.vti"))
    assert [a[0] for a in v["arrays"]] == list(cli.EDDY_VTI_NAMES)
    assert np.array_equal(v["arrays"][0][2], host[::-1, :, 0], equal_nan=True)
    assert np.array_equal(v["arrays"][1][2], host[::-1, :, 1], equal_nan=True)
