"""The layer mode's outer entry points: ``MOPS_CLI --layer K`` and ``MOPSPathline.run(layer=)`` / ``.ftle(layer=)``
forward the layer to the engine, whose lines are the restatement's (tests/layer_reference.py) bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

import layer_reference as LR

HERE = os.path.dirname(os.path.abspath(__file__))
LAYER = 2


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_layer_option(capsys):
    from mops_amd.cli import parse_command_line
    assert parse_command_line(["-i", "x.yaml"]).layer is None          # absent: the reference's run
    assert parse_command_line(["-i", "x.yaml", "--layer", "3"]).layer == 3
    assert parse_command_line(["-i", "x.yaml", "--layer", "0"]).layer == 0
    capsys.readouterr()
    assert parse_command_line(["-i", "x.yaml", "--layer", "-1"]) is None
    assert "--layer" in capsys.readouterr().out


@pytest.mark.gpu
def test_cli_streamline_in_a_layer(engine_lib, oracle_lib, gpu, tmp_path, monkeypatch):
    pytest.importorskip("scipy.io")
    from test_mpas_reader import YAML, _mesh, _write_hist, _write_mesh
    from mops_amd import cli, io as mio, pyMOPS as M
    mesh, snaps = _mesh()
    _write_mesh(str(tmp_path / "mesh.nc"), mesh, 2)
    _write_hist(str(tmp_path / "hist.am.timeSeriesStatsMonthly.0001-01-01.nc"), mesh, snaps[:2], 2, 1)
    y = tmp_path / "mpas.yaml"
    y.write_text(YAML.format(prefix=str(tmp_path)))
    monkeypatch.chdir(tmp_path)
    assert cli.main(["-i", str(y), "-t", "1", "-d", "150", "-g", "1", "--layer", str(LAYER)]) == 0
    got = (tmp_path / "traj_line_1.txt").read_text()
    ss = M.SeedsSettings(); ss.setSeedsRange((31, 31)); ss.setGeoBox((35.0, 45.0), (-90.0, -15.0))
    seeds = M.MOPS_GenerateSeedsPoints(ss)
    depths = np.full(len(seeds), 150.0, dtype=np.float32)
    ref = LR.run_case(oracle_lib, mesh, oracle_lib.preprocess(mesh, snaps[1]), None, seeds, depths, LAYER, euler=True,
                      delta_t=3600, duration=86400, record_t=6 * 3600)
    want = LR.lines(oracle_lib, ref, False)
    mio.save_trajectory_lines_txt(str(tmp_path / "ref.txt"), {"points": want["points"], "velocity": want["velocity"]})
    assert got == (tmp_path / "ref.txt").read_text()
    assert int((ref["death"] < 0).sum()) >= 100
    # ... and it is not the depth run's file
    assert cli.main(["-i", str(y), "-t", "1", "-d", "150", "-g", "1"]) == 0
    assert (tmp_path / "traj_line_1.txt").read_text() != got


@pytest.mark.gpu
def test_mopspathline_run_and_ftle_in_a_layer(engine_lib, oracle_lib, gpu, tmp_path):
    pytest.importorskip("scipy.io")
    from mops_amd import synth
    from mops_amd.engine import FlowMapLattice
    from mops_amd.pathline import MOPSPathline
    rd = _module("test_mpas_reader")
    write_month = _module("test_pathline_api")._write_month
    O = oracle_lib
    mesh = synth.make_mesh(8, n_levels=6)
    snaps = [synth.make_snapshot(mesh, timestep=t, phase=0.3 * t) for t in range(2)]
    rd._write_mesh(str(tmp_path / "mesh.nc"), mesh, 2)
    for d, s in zip(["0001-01-01", "0001-02-01"], snaps):
        write_month(str(tmp_path / f"hist.am.timeSeriesStatsMonthly.{d}.nc"), mesh, s, d + "_00:00:00")
    y = tmp_path / "mpas.yaml"
    y.write_text(rd.YAML.format(prefix=str(tmp_path)))
    r0, r1 = O.preprocess(mesh, snaps[0]), O.preprocess(mesh, snaps[1])
    times = dict(delta_t=10800, duration=31 * 86400, record_t=86400)
    seeds = synth.uniform_band_seeds(40, seed=4)
    p = MOPSPathline(str(y)).init("gpu")
    p.set_time(1, 1, 1, 2)
    p.set_seed(depth=150.0, points=seeds)
    lines = p.run(method="euler", delta_minutes=180, record_every_minutes=1440, layer=LAYER)
    ref = LR.run_case(O, mesh, r0, r1, seeds, np.full(len(seeds), 150.0, dtype=np.float32), LAYER, euler=True, **times)
    want = LR.lines(O, ref, True)
    assert len(lines) == len(seeds) and int((ref["death"] < 0).sum()) >= 10
    for k in ("points", "velocity", "temperature", "salinity", "lastPoint"):
        assert np.stack([ln[k] for ln in lines]).tobytes() == want[k].tobytes(), k
    with pytest.raises(ValueError, match="layer"):
        p.run(method="euler", layer=LAYER, sample_attributes=True)
    # the FTLE image of the layer: the lattice's last points are the restatement's
    win = (6, 4, (-30.0, 30.0), (-160.0, -110.0))
    img = p.ftle(*win, depth=150.0, method="euler", delta_minutes=180, layer=LAYER).cpu().numpy()
    lat = FlowMapLattice(*win)
    ls = lat.seeds.cpu().numpy()
    fref = LR.run_case(O, mesh, r0, r1, ls, np.full(len(ls), 150.0, dtype=np.float32), LAYER, euler=True,
                       delta_t=10800, duration=31 * 86400, record_t=86400)
    last = LR.lines(O, fref, True)["lastPoint"]
    want_img = lat.ftle(last, fref["death"], horizon=31.0).cpu().numpy()
    assert img.shape == (4, 6, 4) and img.tobytes() == want_img.tobytes()
    assert int((~np.isnan(img[:, :, 1])).sum()) >= 6
