"""``MOPS_CLI --eddy-census``: the stage writes the census table and the label image beside the remapping stage's
files, whose bytes stay what they were; without the stage none of its files appears.  The stages are run at a
small image size (the CLI's own sizes are its constants); the option itself is parsed on the CPU
(tests/test_census_cpu.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_reference as IR  # noqa: E402

pytestmark = pytest.mark.gpu


def test_cli_census_stage(engine_lib, gpu, tmp_path, monkeypatch, capsys):
    from test_mpas_reader import YAML, _mesh, _write_hist, _write_mesh
    from mops_amd import cli, engine, io as mio, pyMOPS as M
    mesh, snaps = _mesh()
    _write_mesh(str(tmp_path / "mesh.nc"), mesh, 2)
    _write_hist(str(tmp_path / "hist.am.timeSeriesStatsMonthly.0001-01-01.nc"), mesh, snaps[:2], 2, 1)
    y = tmp_path / "mpas.yaml"
    y.write_text(YAML.format(prefix=str(tmp_path)))
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
    w, h, depth, layer = 48, 24, 150.0, 1
    before = tmp_path / "before"
    before.mkdir()
    monkeypatch.chdir(before)
    base = cli.run_remapping_stage(M, mio, 1, depth, vti=True, width=w, height=h)
    assert sorted(os.listdir(before)) == sorted(base)           # without the stage: the remapping's files only
    assert not any("eddy" in name for name in base)
    after = tmp_path / "after"
    after.mkdir()
    monkeypatch.chdir(after)
    base2 = cli.run_remapping_stage(M, mio, 1, depth, vti=True, width=w, height=h)
    capsys.readouterr()
    written, eddies = cli.run_census_stage(M, mio, 1, layer, vti=True, width=w, height=h)
    out = capsys.readouterr().out
    cen = engine.eddy_census(M._app.mesh, M._app.front, layer=layer)
    assert cen.n_eddies >= 2 and len(eddies) == cen.n_eddies
    assert f"{cen.n_eddies} eddies" in out and f"layer {layer}" in out
    assert base2 == base and sorted(os.listdir(after)) == sorted(base + written)
    assert sorted(written) == sorted(["eddy_census_1.txt"] + [f"eddy_labels_output_0_ch{c}.png" for c in range(3)]
                                     + ["eddy_labels_timestep_1_tile_0_fixed_depth_1.000000.vti"])
    for name in base:   # the remapping stage's own files are the bytes they were
        assert (after / name).read_bytes() == (before / name).read_bytes()
    # the table: one line per eddy holding index, lat, lon, radius in km, area, polarity, circulation, cells
    lines = [ln.split() for ln in (after / "eddy_census_1.txt").read_text().splitlines() if not ln.startswith("#")]
    assert len(lines) == cen.n_eddies
    t = cen.table
    for e, f in enumerate(lines):
        assert len(f) == 8 and int(f[0]) == e and int(f[5]) == t["polarity"][e] and int(f[7]) == t["n_cells"][e]
        assert float(f[1]) == pytest.approx(t["lat"][e], abs=1e-6)
        assert float(f[2]) == pytest.approx(t["lon"][e], abs=1e-6)
        assert float(f[3]) == pytest.approx(t["radius"][e] / 1000.0, abs=1e-6)
        assert float(f[4]) == pytest.approx(t["area"][e], rel=1e-9)
        assert float(f[6]) == pytest.approx(t["circulation"][e], rel=1e-9)
    # the image is the engine's label image on the stage's window
    host = cen.image(w, h, (-90.0, 90.0), (-180.0, 180.0)).cpu().numpy()
    assert np.isfinite(host[..., 0]).any() and np.isnan(host[..., 0]).any()
    for ch in range(3):
        assert np.array_equal(IR.decode_png(str(after / f"eddy_labels_output_0_ch{ch}.png")),
                              IR.save_to_png_rgba(host[..., ch])[0])
    v = IR.read_vti(str(after / "eddy_labels_timestep_1_tile_0_fixed_depth_1.000000.vti"))
    assert [a[0] for a in v["arrays"]] == list(cli.CENSUS_VTI_NAMES)
    assert np.array_equal(v["arrays"][0][2], host[::-1, :, 0], equal_nan=True)
    assert np.array_equal(v["arrays"][1][2], host[::-1, :, 1], equal_nan=True)
