"""Vorticity, divergence, strain and Okubo-Weiss on the GPU (mops_velocity_gradient, mops_cell_to_vertex_signed)
against the numpy restatement (tests/eddy_reference.py), bit for bit: the cell arrays on the small culled mesh,
on the wheel meshes' live cells of 7 to 20 vertices, on a one-level field and on both sources of the vertex
velocity; any subset of outputs; the signed interpolation; and the four existing products fed the signed vertex
arrays -- depth image, section, pathline samples, density map -- against the existing restatements."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_reference as D  # noqa: E402
import eddy_case as EC  # noqa: E402
import eddy_reference as ER  # noqa: E402
import pathline_attr_reference as PR  # noqa: E402
import remap_reference as RR  # noqa: E402
import section_reference as SR  # noqa: E402
import wide_case as WC  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ER.NAMES


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _assert_same(got, want, what):
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
        ok = ~np.isnan(want[k])
        assert np.array_equal(np.signbit(got[k][ok]), np.signbit(want[k][ok])), (what, k)


@pytest.fixture(scope="module")
def case(engine_lib, oracle_lib, gpu, small_case):
    from mops_amd import engine
    c = dict(EC.small(oracle_lib, small_case))
    c["O"] = oracle_lib
    c["dm"] = engine.DeviceMesh.from_mesh(c["mesh"])
    c["f0"] = engine.DeviceField.from_snapshot(c["dm"], c["s0"])     # the fused derivation: records only
    c["f1"] = engine.DeviceField.from_snapshot(c["dm"], c["s1"])
    return c


# ---- 4. the cell arrays ---------------------------------------------------------------------------------------
def test_small_mesh_bit_exact_from_records_and_from_the_vertex_array(case):
    """10 levels on the culled mesh (boundary vertices carry zero velocity): a field from a snapshot keeps its
    velocities in the level-pair records (the entry rebuilds the vertex array from them first), the same field
    uploaded as vertex arrays has them in place; both give the restatement's bytes."""
    from mops_amd import engine
    want = case["g0"]
    mesh = case["mesh"]
    cov = np.asarray(mesh.cellsOnVertex).reshape(-1, 3)
    assert (cov == 0).any()                                          # boundary vertices are present
    for k in NAMES:
        assert np.isfinite(want[k]).all() and want[k].shape == (mesh.nCells, 10)
    for k in ("vorticity", "divergence", "okubo_weiss"):
        assert (want[k] > 0).any() and (want[k] < 0).any(), k
    assert (want["strain"] >= 0).all() and (want["strain"] > 0).any()
    got = _host(engine.velocity_gradient(case["dm"], case["f0"]))
    assert list(got) == list(NAMES)
    _assert_same(got, want, "records")
    d = case["d0"]
    zt, vel, w = case["f0"].export()
    assert vel.tobytes() == d.vertex_vel.tobytes()                  # the restatement read the field's doubles
    up = engine.DeviceField.from_derived(case["dm"], zt, vel, w)
    again = _host(engine.velocity_gradient(case["dm"], up))
    for k in NAMES:
        assert again[k].tobytes() == got[k].tobytes(), k
    # once more on the snapshot field, whose vertex array has been rebuilt by now: the answer stays
    third = _host(engine.velocity_gradient(case["dm"], case["f0"]))
    for k in NAMES:
        assert third[k].tobytes() == got[k].tobytes(), k


def test_one_level_field(case):
    """nVertLevels = 1: no level pair, no record; the vertex array alone."""
    from mops_amd import engine
    m, d = case["mesh"], case["d0"]
    V = m.nVertices
    dm1 = engine.DeviceMesh(nCells=m.nCells, nVertices=V, maxEdges=m.maxEdges, nVertLevels=1,
                            nEdgesOnCell=m.nEdgesOnCell, verticesOnCell=m.verticesOnCell, cellsOnCell=m.cellsOnCell,
                            cellsOnVertex=m.cellsOnVertex, cellCoord=m.cellCoord, vertexCoord=m.vertexCoord)
    lvl = 3
    zt = np.ascontiguousarray(d.vertex_ztop.reshape(V, -1)[:, lvl:lvl + 1])
    vel = np.ascontiguousarray(d.vertex_vel.reshape(V, -1, 3)[:, lvl:lvl + 1])
    w = np.ascontiguousarray(d.vertex_w.reshape(V, -1)[:, lvl:lvl + 2])
    f = engine.DeviceField.from_derived(dm1, zt, vel, w)
    got = _host(engine.velocity_gradient(dm1, f))
    for k in NAMES:
        assert got[k].shape == (m.nCells, 1)
        assert got[k][:, 0].tobytes() == np.ascontiguousarray(case["g0"][k][:, lvl]).tobytes(), k


@pytest.mark.parametrize("key", WC.KEYS)
def test_wheel_meshes_bit_exact(engine_lib, oracle_lib, gpu, key):
    """The MAXV 7, 12 and 20 instantiations on meshes whose cells of 7 to 20 vertices are alive."""
    from mops_amd import engine
    mesh, s0, _ = WC.world(key)
    d = WC.derived(key)[0]
    want = ER.velocity_gradient(mesh, d.vertex_vel)
    deg = WC.degrees(mesh)
    finite = np.all([np.isfinite(want[k]).all(axis=1) for k in NAMES], axis=0)
    wide = sorted(set(int(x) for x in deg[deg >= 7]))
    assert max(wide) == WC.MAX_EDGES[key] and len(wide) >= (1 if key == "me7" else 3), wide
    for n in wide:
        assert finite[deg == n].any(), (key, n)
    for k in ("vorticity", "divergence", "okubo_weiss"):
        assert (want[k][finite] > 0).any() and (want[k][finite] < 0).any(), (key, k)
    dm = engine.DeviceMesh.from_mesh(mesh)
    f = engine.DeviceField.from_snapshot(dm, s0)
    got = _host(engine.velocity_gradient(dm, f))
    _assert_same(got, want, key)
    vel = f.export()[1]
    assert vel.tobytes() == d.vertex_vel.tobytes()
    up = engine.DeviceField.from_derived(dm, d.vertex_ztop, d.vertex_vel, d.vertex_w)
    again = _host(engine.velocity_gradient(dm, up))
    for k in NAMES:
        assert again[k].tobytes() == got[k].tobytes(), (key, k)


# ---- 5. NULL outputs ------------------------------------------------------------------------------------------
def test_any_subset_of_outputs(case):
    from mops_amd import engine
    full = _host(engine.velocity_gradient(case["dm"], case["f0"]))
    for mask in range(1, 15):
        which = tuple(k for i, k in enumerate(NAMES) if mask >> i & 1)
        got = _host(engine.velocity_gradient(case["dm"], case["f0"], which=which))
        assert tuple(got) == which
        for k in which:
            assert got[k].tobytes() == full[k].tobytes(), (which, k)
    one = engine.velocity_gradient(case["dm"], case["f0"], which="okubo_weiss")
    assert list(one) == ["okubo_weiss"] and one["okubo_weiss"].cpu().numpy().tobytes() == full["okubo_weiss"].tobytes()
    with pytest.raises(ValueError, match="which"):
        engine.velocity_gradient(case["dm"], case["f0"], which=("vorticity", "shear"))


def test_refusals_leave_the_outputs_untouched(case):
    """A field of another mesh is refused before any launch (the other refusals need no device:
    test_eddy_cpu.py)."""
    import torch
    from mops_amd import _lib, engine
    other = engine.DeviceMesh.from_mesh(case["mesh"])
    out = torch.full((case["mesh"].nCells, 10), 7.0, dtype=torch.float64, device="cuda")
    p = C.c_void_p(out.data_ptr())
    st = _lib.load().mops_velocity_gradient(other.handle, case["f0"].handle, p, None, None, None, None)
    assert st == _lib.MOPS_ERR_INVALID and b"another mesh" in _lib.load().mops_last_error()
    st = _lib.load().mops_velocity_gradient(case["dm"].handle, case["f0"].handle, None, None, None, None, None)
    assert st == _lib.MOPS_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- 6. the signed interpolation ------------------------------------------------------------------------------
def test_signed_cell_to_vertex(case):
    from mops_amd import engine
    mesh, dm = case["mesh"], case["dm"]
    g = engine.velocity_gradient(dm, case["f0"], which=("vorticity", "okubo_weiss"))
    for k in ("vorticity", "okubo_weiss"):
        got = engine.cell_to_vertex_attr(dm, g[k], signed=True).cpu().numpy()
        want = case["v0"][k]
        assert (want < 0).any() and (want > 0).any()
        assert got.shape == want.shape == (mesh.nVertices, 10)
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), k
        clamped = engine.cell_to_vertex_attr(dm, g[k]).cpu().numpy()
        assert np.array_equal(clamped, np.where(want < 0, 0.0, want))       # the old entry still clamps
        assert (clamped != got).any()
    vg = _host(engine.velocity_gradient(dm, case["f0"], which=("vorticity", "okubo_weiss"), vertex=True))
    for k in vg:
        assert vg[k].tobytes() == np.ascontiguousarray(case["v0"][k]).tobytes(), k
    cov = np.asarray(mesh.cellsOnVertex).reshape(-1, 3)
    assert np.all(vg["vorticity"][(cov == 0).any(axis=1)] == 0.0)           # boundary vertices get 0
    # on a non-negative array the two entries are the same bytes
    temp = np.asarray(case["s0"].attributes["temperature"], dtype=np.float64)
    assert (temp >= 0).all()
    a = engine.cell_to_vertex_attr(dm, temp).cpu().numpy()
    b = engine.cell_to_vertex_attr(dm, temp, signed=True).cpu().numpy()
    assert a.tobytes() == b.tobytes() and a.tobytes() == case["d0"].attrs["temperature"].tobytes()
    # an all-negative array: the old entry returns zeros, the new one the values
    neg = engine.cell_to_vertex_attr(dm, -1.0 - temp).cpu().numpy()
    sneg = engine.cell_to_vertex_attr(dm, -1.0 - temp, signed=True).cpu().numpy()
    assert not neg.any() and (sneg < 0).any() and not (sneg > 0).any()
    with pytest.raises(ValueError):
        engine.cell_to_vertex_attr(dm, temp[:-1], signed=True)


# ---- 7. composition through the existing entries ----------------------------------------------------------------
@pytest.fixture(scope="module")
def vattrs(case):
    from mops_amd import engine
    v0 = engine.velocity_gradient(case["dm"], case["f0"], which=("vorticity", "okubo_weiss"), vertex=True)
    v1 = engine.velocity_gradient(case["dm"], case["f1"], which=("vorticity", "okubo_weiss"), vertex=True)
    for v, want in ((v0, case["v0"]), (v1, case["v1"])):
        for k in v:
            assert v[k].cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes()
    return v0, v1


@pytest.mark.parametrize("rule", EC.RULES)
def test_fixed_depth_image(case, vattrs, small_case, rule):
    from mops_amd import engine
    ref = EC.depth_image(case["O"], small_case, rule)
    v0 = vattrs[0]
    images, cells = engine.remap_fixed_depth(case["dm"], case["f0"], EC.WIDTH, EC.HEIGHT, EC.LAT, EC.LON, EC.DEPTH,
                                             n_attr=2, vertex_attrs=(v0["vorticity"], v0["okubo_weiss"]),
                                             layer_rule=rule, return_cells=True)
    got = images.cpu().numpy()
    assert got.shape == (2, EC.HEIGHT, EC.WIDTH, 4)
    assert np.array_equal(cells.cpu().numpy().reshape(-1), EC.depth_cells(case["O"], small_case))
    for k in range(2):
        assert np.array_equal(got[k], ref["images"][k], equal_nan=True), (rule, k)
    valid = ref["code"] == RR.VALID
    assert np.all(got[1][valid][:, 2] == 0.0) and np.all(got[1][..., 3] == 1.0)
    if rule == "bracket":
        assert len(np.unique(ref["layer"][valid])) >= 2


def test_section(case, vattrs):
    from mops_amd import engine
    path, w, h = [(-30.0, -20.0), (50.0, 80.0)], 37, 20
    mesh = case["mesh"]
    drange = (float(mesh.refBottomDepth[0]), float(mesh.refBottomDepth[-1]))
    pts, nrm, dist = SR.section_points(path, w)
    cells = case["O"].knn(mesh, pts)
    ref = SR.section(mesh, case["d0"], pts, nrm, h, drange, cells,
                     attrs=[case["v0"]["vorticity"].reshape(-1), case["v0"]["okubo_weiss"].reshape(-1)])
    valid = ref["code"] == RR.VALID
    assert valid.sum() >= 0.4 * valid.size and (~valid).any()
    a = ref["images"][1][valid]
    assert (a[:, 0] > 0).any() and (a[:, 0] < 0).any() and (a[:, 1] != 0).any()
    v0 = vattrs[0]
    images, gdist = engine.remap_section(case["dm"], case["f0"], path, w, h, drange,
                                         vertex_attrs=(v0["vorticity"], v0["okubo_weiss"]))
    assert gdist.tobytes() == dist.tobytes()
    assert np.array_equal(images.cpu().numpy(), ref["images"], equal_nan=True)


DELTA_T, N_STEPS, EVERY = 21600, 12, 3        # 12 steps, a record every 3: K = 4
N_SEEDS = 40                                  # not a multiple of the 64-lane wave


@pytest.fixture(scope="module")
def pathline(case, vattrs):
    """A short pathline with the vorticity carried along, on the device and in the restatement."""
    from mops_amd import synth
    from mops_amd.engine import TrajectoryConfig, run_trajectories
    O, mesh = case["O"], case["mesh"]
    seeds = synth.uniform_band_seeds(N_SEEDS, seed=5)
    depths = np.random.default_rng(9).uniform(5, 1500, N_SEEDS).astype(np.float32)
    cells = O.knn(mesh, seeds)
    front = EC.derived_with_eddy(O, case["d0"], case["v0"], names=("vorticity",))
    back = EC.derived_with_eddy(O, case["d1"], case["v1"], names=("vorticity",))
    ref = PR.run(mesh, front, back, seeds, depths, cells, DELTA_T, N_STEPS * DELTA_T, EVERY * DELTA_T, euler=True)
    K = N_STEPS // EVERY
    want = PR.attr_lines(O, seeds, ref, K)[0]
    cfg = TrajectoryConfig(deltaT=DELTA_T, simulationDuration=N_STEPS * DELTA_T, recordT=EVERY * DELTA_T, depth=0.0,
                           method=1)
    got = run_trajectories(case["dm"], case["f0"], case["f1"], cfg, seeds, depths=depths, cells=cells,
                           attrs={"vorticity": (vattrs[0]["vorticity"], vattrs[1]["vorticity"])})
    return dict(ref=ref, want=want, got=got, K=K)


def test_vorticity_along_pathlines(pathline):
    ref, want, got = pathline["ref"], pathline["want"], pathline["got"]
    alive = ref["death"] < 0
    assert alive.sum() >= N_SEEDS // 2
    assert (want[alive] > 0).any() and (want[alive] < 0).any()        # negative samples are carried as they are
    assert np.array_equal(got["death_step"], ref["death"])
    assert list(got["attributes"]) == ["vorticity"]
    assert np.array_equal(got["attributes"]["vorticity"], want)
    assert np.array_equal(np.signbit(got["attributes"]["vorticity"]), np.signbit(want))


def test_density_map_of_the_samples(pathline):
    from mops_amd.engine import DensityMap
    win = (24, 12, (-90.0, 90.0), (-180.0, 180.0))
    pts = pathline["got"]["points"][:, 1:]
    vals = pathline["got"]["attributes"]["vorticity"][:, 1:]
    d = D.edge_distance(pts.reshape(-1, 3), *win)
    assert d > D.EDGE_GUARD, f"a test point lies {d:.3g} of a pixel from a pixel edge"
    m = DensityMap(*win, value="vorticity")
    m.accumulate_lines(pts, vals)
    acc = D.accumulate(D.new_accum(win[0], win[1]), pts.reshape(-1, 3), *win, values=vals.reshape(-1))
    assert (acc[:, :, 0] > 0).any() and (acc[:, :, 1] < 0).any() and (acc[:, :, 1] > 0).any()
    assert m.accum.cpu().numpy().tobytes() == acc.tobytes()
    assert m.image().cpu().numpy().tobytes() == D.image(acc).tobytes()
