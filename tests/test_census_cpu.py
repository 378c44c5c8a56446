"""The eddy census's restatement (tests/census_reference.py) against a brute-force search on the small mesh, the
agreement of header, ctypes stubs and exports on the new entries, and the refusals of the C entries, of
engine.eddy_census and of pyMOPS.MOPS_RunEddyCensus, none of which needs a device."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_case as CC  # noqa: E402
import census_reference as CR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mops_cell_area": 3, "mops_eddy_classify": 7, "mops_label_components": 5, "mops_eddy_count": 6,
           "mops_eddy_table": 17}


def _bfs_labels(mesh, cls):
    """Brute force: symmetric adjacency lists, then a breadth-first search from every unvisited cell in
    ascending order -- the first cell of a component is its minimum."""
    C_ = len(cls)
    adj = [set() for _ in range(C_)]
    for c, d in CR.edges(mesh, cls):
        adj[c].add(d)
        adj[d].add(c)
    out = np.full(C_, -1, dtype=np.int32)
    for c in range(C_):
        if cls[c] == 0 or out[c] >= 0:
            continue
        out[c] = c
        todo = [c]
        while todo:
            nxt = []
            for x in todo:
                for y in adj[x]:
                    if out[y] < 0:
                        out[y] = c
                        nxt.append(y)
            todo = nxt
    return out


@pytest.fixture(scope="module")
def classes(oracle_lib, small_case):
    mesh = small_case[0]
    out = dict(CC.synthetic_classes(mesh))
    for k in CC.K_SIGMAS:
        out[f"eddy_{k}"] = CC.census(oracle_lib, small_case, k, 1)["classes"]
    return out


@pytest.mark.parametrize("name", ["ones", "zeros", "single", "random", "band", "eddy_0.2", "eddy_0.05"])
def test_restatement_against_brute_force(small_case, classes, name):
    mesh, cls = small_case[0], classes[name]
    lab = CR.label_components(mesh, cls)
    assert lab.dtype == np.int32 and lab.shape == (mesh.nCells,)
    assert np.array_equal(lab, _bfs_labels(mesh, cls))
    assert np.array_equal(lab < 0, cls == 0)
    live = np.flatnonzero(lab >= 0)
    # a label is the minimum of its component, a member of it, and of the same class: a partition by roots
    assert np.all(lab[live] <= live) and np.array_equal(lab[lab[live]], lab[live])
    assert np.array_equal(cls[lab[live]], cls[live])
    for root, size in CR.component_sizes(lab).items():
        assert np.flatnonzero(lab == root).min() == root and size >= 1
    for c, d in CR.edges(mesh, cls):
        assert lab[c] == lab[d]
    # labelling the labels again (as classes, shifted off 0) changes nothing
    assert np.array_equal(CR.label_components(mesh, np.where(lab >= 0, lab + 1, 0)), lab)


def test_small_mesh_census_has_the_shapes_the_gpu_tests_rely_on(oracle_lib, small_case):
    c = CC.small(oracle_lib, small_case)
    assert np.isfinite(c["area"]).all() and (c["area"] > 0).all()
    a = CC.census(oracle_lib, small_case, 0.2, 1)
    sizes = sorted(CR.component_sizes(a["components"]).values())
    assert a["E"] == len(sizes) >= 5 and sizes[0] == 1
    assert (a["table"]["polarity"] == 1).any() and (a["table"]["polarity"] == -1).any()
    b = CC.census(oracle_lib, small_case, 0.05, 1)
    assert max(CR.component_sizes(b["components"]).values()) > 256
    # membership: min_cells drops the small ones and renumbers the rest by ascending root
    four = CC.census(oracle_lib, small_case, 0.2, 4)
    keep = a["table"]["n_cells"] >= 4
    assert 0 < four["E"] == int(keep.sum()) < a["E"]
    assert np.all(np.diff(four["table"]["root"]) > 0)
    for k in CR.COLUMNS:
        assert four["table"][k].tobytes() == np.ascontiguousarray(a["table"][k][keep]).tobytes(), k
    none = CC.census(oracle_lib, small_case, 0.2, 10_000)
    assert none["E"] == 0 and (none["labels"] == -1).all() and none["table"]["centre"].shape == (0, 3)
    # the table's sums against numpy's own, loosely: the area is the members' and the centre a unit vector
    t = a["table"]
    for e in range(a["E"]):
        m = np.flatnonzero(a["labels"] == e)
        assert t["root"][e] == m[0] and t["n_cells"][e] == len(m)
        assert t["area"][e] == pytest.approx(c["area"][m].sum(), rel=1e-12)
        assert np.linalg.norm(t["centre"][e]) == pytest.approx(1.0, abs=1e-12)
        assert t["ow_min"][e] == c["g0"]["okubo_weiss"][m, 0].min() == c["g0"]["okubo_weiss"][t["core_cell"][e], 0]
        assert np.sign(t["circulation"][e]) == t["polarity"][e]


def test_header_stubs_and_exports_agree(engine_lib):
    from mops_amd import _lib
    text = open(os.path.join(ROOT, "include", "mops_traj.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in ENTRIES.items():
        assert name in _lib.EXPORTED and hasattr(engine_lib, name), name
        m = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        stub = getattr(engine_lib, name).argtypes
        assert len(params) == len(stub) == n_args, name
        for p, t in zip(params, stub):
            if "*" in p:
                assert t is C.c_void_p, (name, p)
            elif p.startswith("int32_t"):
                assert t is C.c_int32, (name, p)
            elif p.startswith("int64_t"):
                assert t is C.c_int64, (name, p)
            elif p.startswith("double"):
                assert t is C.c_double, (name, p)
            else:
                raise AssertionError((name, p))
    assert engine_lib.mops_abi_version() == 4


def test_c_entry_refusals_need_no_device(engine_lib):
    from mops_amd import _lib
    fake = C.c_void_p(0x1000)   # never dereferenced
    n = C.c_int64(7)
    rounds = C.c_int32(7)
    calls = [
        ("mops_cell_area", (None, fake, None)), ("mops_cell_area", (fake, None, None)),
        ("mops_eddy_classify", (None, fake, fake, 0, -1.0, fake, None)),
        ("mops_eddy_classify", (fake, None, fake, 0, -1.0, fake, None)),
        ("mops_eddy_classify", (fake, fake, fake, 0, -1.0, None, None)),
        ("mops_label_components", (None, fake, fake, C.byref(rounds), None)),
        ("mops_label_components", (fake, None, fake, None, None)),
        ("mops_label_components", (fake, fake, None, None, None)),
        ("mops_eddy_count", (None, fake, 1, fake, C.byref(n), None)),
        ("mops_eddy_count", (fake, fake, 1, fake, None, None)),
        ("mops_eddy_count", (fake, fake, 0, fake, C.byref(n), None)),
        ("mops_eddy_table", (None, fake, 1, fake, fake, fake, fake, 0) + (fake,) * 8 + (None,)),
        ("mops_eddy_table", (fake, fake, 1, None, fake, fake, fake, 0) + (fake,) * 8 + (None,)),
    ]
    for name, args in calls:
        assert getattr(engine_lib, name)(*args) == _lib.MOPS_ERR_INVALID, (name, args)
        assert name.encode() in engine_lib.mops_last_error()
    assert n.value == 7 and rounds.value == 7


def test_eddy_census_refusals_come_before_any_launch():
    """A layer outside the levels, min_cells < 1, a non-finite threshold and a gradient of the wrong shape are
    ValueErrors raised before anything touches the device: the mesh here is a stand-in without one."""
    import torch
    from mops_amd import engine
    mesh = types.SimpleNamespace(nCells=12, nVertLevels=3, handle=None)
    for kw in (dict(layer=3), dict(layer=-1), dict(min_cells=0), dict(threshold=float("nan")),
               dict(threshold=float("-inf")), dict(gradient={"vorticity": None}),
               dict(gradient={"vorticity": torch.zeros(12, 3, dtype=torch.float64),
                              "okubo_weiss": torch.zeros(12, 3, dtype=torch.float64)}),       # not on the device
               dict(gradient={"vorticity": torch.zeros(12, 2, dtype=torch.float64),
                              "okubo_weiss": torch.zeros(12, 2, dtype=torch.float64)}),
               dict(gradient=[1, 2])):
        with pytest.raises(ValueError):
            engine.eddy_census(mesh, None, **kw)
    with pytest.raises(ValueError, match="layer"):
        engine.eddy_classify(mesh, None, None, 5, -1.0)
    with pytest.raises(ValueError, match="min_cells"):
        engine.eddy_table(mesh, None, None, None, None, None, 0, min_cells=0)


def test_pymops_refusals_and_settings(capsys):
    from mops_amd import pyMOPS as M
    cfg = M.VisualizationSettings()
    assert cfg.EddyThreshold == 0.2 and cfg.EddyMinCells == 4
    assert M.MOPS_RunEddyCensus(None) == ([], [])
    cfg.imageSize = (0, 4)
    assert M.MOPS_RunEddyCensus(cfg) == ([], [])
    assert "EddyCensus" in "".join(capsys.readouterr())
    cfg.FixedLayer = 3.7
    assert M._census_layer(cfg, 10) == 3
    for fl, want in ((-2.0, 0), (0.99, 0), (9.0, 9), (10.0, 9), (1e30, 9), (float("nan"), 0)):
        cfg.FixedLayer = fl
        assert M._census_layer(cfg, 10) == want, fl


def test_cli_eddy_census_option():
    from mops_amd.cli import parse_command_line
    a = parse_command_line(["-i", "x.yaml"])
    assert a.eddy_census is False and a.eddy is False
    a = parse_command_line(["-i", "x.yaml", "--eddy-census", "--layer", "3", "--vti"])
    assert a.eddy_census and a.layer == 3 and a.vti and not a.eddy


def test_lat_lon_radius_columns():
    from mops_amd import engine
    centre = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.0, -0.8]])
    area = np.array([np.pi, 4 * np.pi, 0.0, 1.0])
    lat, lon, radius = engine.eddy_lat_lon_radius(centre, area)
    want = CR.lat_lon_radius(centre, area)
    for a, b in zip((lat, lon, radius), want):
        assert a.tobytes() == b.tobytes()
    assert list(lat[:3]) == [0.0, 0.0, 90.0] and list(lon[:2]) == [0.0, -90.0] and list(radius[:3]) == [1.0, 2.0, 0.0]
    assert lat[3] == pytest.approx(-53.13010235415598)
