"""MOPS_CLI's --kh and --seed (mops_amd/cli.py): the options and their refusals (no GPU), and on the GPU the
streamline of a layer with the random walk against the restatement (tests/diffusion_reference.py)."""
import numpy as np
import pytest

import diffusion_reference as D

LAYER, KH, SEED = 2, 100.0, 77


def test_cli_kh_and_seed_options(capsys):
    from mops_amd.cli import parse_command_line
    a = parse_command_line(["-i", "x.yaml"])
    assert a.kh == 0.0 and a.seed == 0                                  # absent: the reference's run
    a = parse_command_line(["-i", "x.yaml", "--layer", "3", "--kh", "100", "--seed", "9"])
    assert (a.layer, a.kh, a.seed) == (3, 100.0, 9)
    assert parse_command_line(["-i", "x.yaml", "--seed", "9"]).seed == 9   # (a seed alone changes nothing)
    capsys.readouterr()
    assert parse_command_line(["-i", "x.yaml", "--kh", "100"]) is None   # without --layer: refused
    out = capsys.readouterr().out
    assert "--kh" in out and "--layer" in out and out.startswith("[ERROR]::")
    for bad in ("-1", "nan", "inf"):
        assert parse_command_line(["-i", "x.yaml", "--layer", "3", "--kh", bad]) is None
        assert "--kh" in capsys.readouterr().out
    assert parse_command_line(["-i", "x.yaml", "--layer", "3", "--kh", "1", "--seed", "-4"]) is None
    assert "--seed" in capsys.readouterr().out


@pytest.mark.gpu
def test_cli_streamline_with_diffusion(engine_lib, oracle_lib, gpu, tmp_path, monkeypatch):
    pytest.importorskip("scipy.io")
    from test_mpas_reader import YAML, _mesh, _write_hist, _write_mesh
    from mops_amd import cli, io as mio, pyMOPS as M
    mesh, snaps = _mesh()
    _write_mesh(str(tmp_path / "mesh.nc"), mesh, 2)
    _write_hist(str(tmp_path / "hist.am.timeSeriesStatsMonthly.0001-01-01.nc"), mesh, snaps[:2], 2, 1)
    y = tmp_path / "mpas.yaml"
    y.write_text(YAML.format(prefix=str(tmp_path)))
    monkeypatch.chdir(tmp_path)
    base = ["-i", str(y), "-t", "1", "-d", "150", "-g", "1", "--layer", str(LAYER)]
    assert cli.main(base + ["--kh", str(KH), "--seed", str(SEED)]) == 0
    got = (tmp_path / "traj_line_1.txt").read_text()
    ss = M.SeedsSettings(); ss.setSeedsRange((31, 31)); ss.setGeoBox((35.0, 45.0), (-90.0, -15.0))
    seeds = M.MOPS_GenerateSeedsPoints(ss)
    depths = np.full(len(seeds), 150.0, dtype=np.float32)
    ref = D.run_case(oracle_lib, mesh, oracle_lib.preprocess(mesh, snaps[1]), None, seeds, depths, layer=LAYER,
                     euler=True, kh=KH, seed=SEED, delta_t=3600, duration=86400, record_t=6 * 3600)
    want = D.lines(oracle_lib, ref, False)
    mio.save_trajectory_lines_txt(str(tmp_path / "ref.txt"), {"points": want["points"], "velocity": want["velocity"]})
    assert got == (tmp_path / "ref.txt").read_text()
    assert int((ref["death"] < 0).sum()) >= 100
    # ... and it is not the file of the run without it
    assert cli.main(base) == 0
    assert (tmp_path / "traj_line_1.txt").read_text() != got
