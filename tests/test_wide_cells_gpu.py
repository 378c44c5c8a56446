"""GPU: every kernel that reads a cell polygon, on cells of 7 to 20 vertices that are alive.

The meshes are tests/wide_case.py's: true Voronoi meshes with "wheels" (tests/golden/voronoi_me{7,12,20}.npz),
whose wide cells contain their own centres -- unlike the flipped heptagons and the padded maxEdges 10 / 16 / 20
meshes of the other files, on which no particle lives and no pixel is valid in a cell of more than six vertices
(tests/test_wide_cells_cpu.py).  maxEdges 7, 12 and 20 select the MAXV 7, 12 and 20 instantiations.

Every comparison is on bytes: np.array_equal against the oracle (oracle/mops_oracle.c) or a Python restatement
(remap_reference, image_reference, pathline_attr_reference, rk4_relocate_reference), which
tests/test_reference_pin.py pins to the compiled reference on these same meshes.  The conditions that make the
comparisons mean something (particles alive per degree, cell crossings into and between wide cells, valid pixels
per degree) are asserted from the oracle's and the restatements' own results, and printed.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_reference as IR  # noqa: E402
import pathline_attr_reference as PR  # noqa: E402
import remap_reference as RR  # noqa: E402
import rk4_relocate_reference as KR  # noqa: E402
import wide_case as WC  # noqa: E402
from test_gpu_parity import assert_lines_match  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["salinity", "temperature"]  # std::map order
LINE_KEYS = ("points", "velocity", "temperature", "salinity", "lastPoint")
RELOCATE = 2  # MOPS_RK4_RELOCATE


def _report(capsys, text):
    with capsys.disabled():
        print("\n    [wide cells] " + text, end="")


class _Device:
    """One wide mesh on the device with both snapshots' fields and attribute vertex arrays."""

    def __init__(self, key):
        from mops_amd.engine import DeviceField, DeviceMesh, cell_to_vertex_attr
        self.key = key
        self.mesh, s0, s1 = WC.world(key)
        self.dm = DeviceMesh.from_mesh(self.mesh)
        self.f0, self.f1 = DeviceField.from_snapshot(self.dm, s0), DeviceField.from_snapshot(self.dm, s1)
        self.attrs = {k: (cell_to_vertex_attr(self.dm, s0.attributes[k]), cell_to_vertex_attr(self.dm, s1.attributes[k]))
                      for k in NAMES}


@pytest.fixture(scope="module")
def device(gpu, engine_lib, oracle_lib):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = _Device(key)
        return cache[key]
    return get


def _cfg(times, euler=True, backward=False, depth=0.0, method=None):
    from mops_amd.engine import TrajectoryConfig
    dt, duration, record_t = times
    return TrajectoryConfig(deltaT=dt, simulationDuration=duration, recordT=record_t, depth=depth,
                            method=(1 if euler else 0) if method is None else method, direction=1 if backward else 0)


# ---- the premise ----------------------------------------------------------------------------------------------
def test_device_trig_equals_host_below_the_step_angle(gpu, engine_lib):
    """Bit parity with the oracle needs the device library's sin / cos (which dev::sincos_small reproduces) to give
    the host library's doubles for the angle an Euler step turns by.  That holds for small angles only: on an
    MI355X 4 of 2e6 cosines in [1e-3, 3e-3) differ from glibc's by an ulp -- cos(0.0010925430624395252) is one,
    within 3e-7 ulp of a tie -- and none of 8e6 below 1e-3.  The cases of this file keep every step below
    wide_case.MAX_STEP_ANGLE (asserted from the oracle's velocities in tests/test_wide_cells_cpu.py); here 2e6
    angles up to twice that, log-uniform from 1e-8, must agree."""
    import ctypes
    import math
    import torch
    th = 10.0 ** np.random.default_rng(12).uniform(-8.0, np.log10(2.0 * WC.MAX_STEP_ANGLE), 2_000_000)
    th[::2] *= -1.0
    d = torch.as_tensor(th, device=gpu)
    out = torch.empty((len(th), 4), dtype=torch.float64, device=gpu)
    assert engine_lib.mops_selftest_math(len(th), ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(out.data_ptr()), 1,
                                         None) == 0
    o = out.cpu().numpy()
    assert np.array_equal(o[:, 0], o[:, 1]) and np.array_equal(o[:, 2], o[:, 3]), "sincos_small != device sin / cos"
    # the host library the oracle calls: libm through math, not numpy's own loops
    assert np.array_equal(o[:, 1], np.array([math.sin(x) for x in th])), "device sin != libm sin"
    assert np.array_equal(o[:, 3], np.array([math.cos(x) for x in th])), "device cos != libm cos"


# ---- derived fields and location ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WC.KEYS)
def test_derived_fields_and_location_bitwise(device, oracle_lib, gpu, key):
    """The cell-to-vertex kernels and the 1-NN location on the wheel meshes (vertices shared by cells of 4 to 20
    vertices; a wheel's ring cells are a quarter of a hexagon across) against oracle.preprocess and oracle.knn."""
    import torch
    d = device(key)
    for f, r in zip((d.f0, d.f1), WC.derived(key)):
        zt, ve, w = f.export()
        assert np.array_equal(zt, r.vertex_ztop) and np.array_equal(ve, r.vertex_vel) and np.array_equal(w, r.vertex_w)
    for k in NAMES:
        for t, r in zip(d.attrs[k], WC.derived(key)):
            assert np.array_equal(t.cpu().numpy().reshape(-1), r.attrs[k].reshape(-1)), k
    pts = np.concatenate([WC.seeds(key), d.mesh.cellCoord[WC.degrees(d.mesh) >= 7] * 1.0]
                         + [RR.depth_positions(w, h, lat, lon) for w, h, (lat, lon) in WC.WINDOWS.values()])
    ref = oracle_lib.knn(d.mesh, pts)
    assert (WC.degrees(d.mesh)[ref] >= 7).sum() >= 1000
    dp = torch.as_tensor(pts, device=gpu)
    out = torch.empty(len(pts), dtype=torch.int32, device=gpu)
    d.dm.locate(dp.data_ptr(), out.data_ptr(), len(pts))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)


# ---- trajectories ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", WC.MODES, ids=lambda m: WC.mode_name(*m))
@pytest.mark.parametrize("key", WC.KEYS)
def test_trajectories_bit_exact(device, capsys, key, mode):
    """{stream, path} x {Euler, RK4} x {forward, backward} on wide_case.seeds(): whole waves in hexagons, whole
    waves in one wide cell, waves that mix degrees, seeds on wide cells' centres, vertices and edge planes."""
    from mops_amd.engine import run_trajectories
    pathline, euler, backward = mode
    d = device(key)
    seeds = WC.seeds(key)
    assert len(seeds) <= 3000
    ref = WC.oracle_run(key, pathline, euler, backward)
    got = run_trajectories(d.dm, d.f0, d.f1 if pathline else None,
                           _cfg(WC.times(euler), euler, backward, depth=WC.DEPTH), seeds)
    assert np.array_equal(got["cells"], WC.seed_cells(key))
    nv = WC.degrees(d.mesh)[ref["cells"]]
    past0 = {int(k): int(((nv == k) & (ref["death"] != 0)).sum()) for k in np.unique(nv[nv >= 7])}
    end = {int(k): int(((nv == k) & (ref["death"] < 0)).sum()) for k in np.unique(nv[nv >= 7])}
    _report(capsys, f"{key} {WC.mode_name(*mode)}: seeded in wide cells and alive after step 0 {past0}, at the end {end}")
    assert min(past0.values()) >= 20, past0
    assert_lines_match(got, ref, f"{key} {WC.mode_name(*mode)}")
    if pathline:
        assert np.array_equal(got["temperature"], ref["temperature"]) and np.array_equal(got["salinity"], ref["salinity"])


@pytest.mark.parametrize("mode", WC.MODES, ids=lambda m: WC.mode_name(*m))
@pytest.mark.parametrize("key", WC.KEYS)
def test_waves_of_every_kind_in_seed_order(device, key, mode):
    """The same runs launched in seed order (use_order=False: no locality sort), where slots 0-127 are two whole
    waves in hexagons, 128-255 two whole waves in the first wheel's cell, 256-383 two in the widest cell, and the
    following waves alternate wide cells and hexagons lane by lane
    (test_wide_cells_cpu.test_seeds_cover_every_kind_of_wave) -- every record, state and line against the oracle."""
    from mops_amd.engine import ParticleSet
    pathline, euler, backward = mode
    d = device(key)
    cfg = _cfg(WC.times(euler), euler, backward, depth=WC.DEPTH)
    ref = WC.oracle_run(key, pathline, euler, backward)
    ps = ParticleSet(d.dm, WC.seeds(key), WC.DEPTH, cfg, use_order=False)
    assert np.array_equal(ps.ids.cpu().numpy(), np.arange(ps.n)), "the particles were reordered"
    assert np.array_equal(ps.cell.cpu().numpy(), WC.seed_cells(key))
    ps.advance(d.f0, d.f1 if pathline else None, 0, cfg.n_steps)
    fin = ps.finalize(pathline=pathline)
    assert np.array_equal(ps.ids.cpu().numpy(), np.arange(ps.n))
    assert np.array_equal(ps.death.cpu().numpy(), ref["death"])
    for k in LINE_KEYS:
        assert np.array_equal(fin[k].cpu().numpy(), ref[k], equal_nan=True), k
    assert np.array_equal(ps.depth.cpu().numpy(), ref["final_depth"])
    assert np.array_equal(np.stack([ps.x.cpu().numpy(), ps.y.cpu().numpy(), ps.z.cpu().numpy()], 1), ref["final_pos"],
                          equal_nan=True)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_dense_waves_on_heptagons(device, oracle_lib, capsys, euler, backward):
    """test_pathline_cooperative_waves' density (45..58 particles per cell, one or two depth groups) with five of
    the 14 cells heptagons and the other nine hexagons upstream of one, run twice against one oracle result:
    through run_trajectories, which launches with a processing order and so runs the plain kernels on live
    heptagons, and slot-ordered (tile_case.run_slot_ordered, selection flag 1 asserted), which runs the cooperative
    tile and, in RK4, the hand-off kernel and the resumed one: waves with a lane in a heptagon are handed over at
    step 0, and the particles seeded towards a heptagon die at its edge there (quirk Q1) or, in Euler, cross
    into it on the tile."""
    import tile_case
    from mops_amd.engine import run_trajectories
    d = device("me7")
    seeds, depths, cells = WC.dense_seeds("me7")
    r0, r1 = WC.derived("me7")
    dt, duration, record_t = WC.DENSE_TIMES
    got = run_trajectories(d.dm, d.f0, d.f1, _cfg(WC.DENSE_TIMES, euler, backward), seeds, depths=depths)
    ref = oracle_lib.run(d.mesh, r0, r1, seeds, depths=depths, delta_t=dt, duration=duration, record_t=record_t,
                         euler=euler, backward=backward, cells=got["cells"])
    nv = WC.degrees(d.mesh)
    live7 = int(((nv[ref["cells"]] == 7) & (ref["death"] != 0)).sum())
    _report(capsys, f"dense me7 {'euler' if euler else 'rk4'} {'backward' if backward else 'forward'}: {live7} "
                    f"particles in heptagons alive after step 0, {int((ref['death'] < 0).sum())} of {len(seeds)} at the end")
    assert len(seeds) % 64 != 0 and (nv[cells] == 7).sum() >= 4 and live7 >= 200
    assert (ref["death"] >= 0).any() and (ref["death"] < 0).any()
    assert_lines_match(got, ref, "dense waves on heptagons")
    tiled = tile_case.run_slot_ordered(d.dm, d.f0, d.f1, _cfg(WC.DENSE_TIMES, euler, backward), seeds, depths,
                                       got["cells"], expect_flag=1)
    assert_lines_match(tiled, ref, "dense waves on heptagons, tile kernels")


@pytest.mark.parametrize("key", WC.KEYS)
def test_segmented_run_with_compaction_equals_single(device, gpu, key):
    """Two segments with a reorder between them, and the pipelined advance with its dead-particle compaction
    before every chunk, against one launch: RK4 pathlines, whose particles die at crossings throughout the run."""
    import torch
    from mops_amd.engine import ParticleSet
    d = device(key)
    seeds = WC.seeds(key)
    cfg = _cfg(WC.times(False), euler=False, depth=WC.DEPTH)
    want = WC.oracle_run(key, True, False, False)
    a = ParticleSet(d.dm, seeds, WC.DEPTH, cfg)
    a.advance(d.f0, d.f1, 0, cfg.n_steps)
    la = a.finalize(pathline=True)
    assert np.array_equal(a.original(a.death).cpu().numpy(), want["death"])
    assert np.array_equal(la["points"].cpu().numpy(), want["points"])
    assert (want["death"] > 0).sum() >= 100
    b = ParticleSet(d.dm, seeds, WC.DEPTH, cfg)
    b.advance(d.f0, d.f1, 0, 13)
    b.reorder()
    b.advance(d.f0, d.f1, 13, cfg.n_steps)
    c = ParticleSet(d.dm, seeds, WC.DEPTH, cfg)
    c.records.fill_(float("nan"))
    streams = [torch.cuda.Stream() for _ in range(2)]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    c.advance_pipelined(d.f0, d.f1, 0, cfg.n_steps, streams, 7, compact=True)
    for st in streams:
        torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    for other in (b, c):
        lo = other.finalize(pathline=True)
        for k in LINE_KEYS:
            assert torch.equal(la[k], lo[k]), k
        for k in ("x", "y", "z", "depth", "cell", "death"):
            assert torch.equal(a.original(getattr(a, k)), other.original(getattr(other, k))), k


# ---- the relocating RK4 and the attribute samplers ------------------------------------------------------------
@pytest.mark.parametrize("key", WC.KEYS)
def test_rk4_relocate_bit_exact(device, oracle_lib, capsys, key):
    """traj_lane_kernel<7 / 12 / 20>'s relocating RK4 against tests/rk4_relocate_reference.py: stages that land in a wide
    cell from a hexagon and in a hexagon from a wide cell."""
    from mops_amd.engine import run_trajectories
    d = device(key)
    seeds, depths, cells = WC.sample_seeds(key)
    r0, r1 = WC.derived(key)
    dt, duration, record_t = WC.SAMPLE_TIMES
    ref = KR.run_case(oracle_lib, d.mesh, r0, r1, seeds, depths, relocate=True, delta_t=dt, duration=duration,
                      record_t=record_t, cells=cells)
    _report(capsys, f"{key} relocating RK4: {int((ref['death'] < 0).sum())} of {len(seeds)} alive, "
                    f"{int(ref['relocations'].sum())} relocated stages, {int(ref['relocations_poly'].sum())} onto another polygon size")
    assert int(ref["relocations_poly"].sum()) >= 50 and int((ref["death"] < 0).sum()) > len(seeds) // 2
    got = run_trajectories(d.dm, d.f0, d.f1, _cfg(WC.SAMPLE_TIMES, method=RELOCATE), seeds, depths=depths,
                           cells=cells)
    want = KR.lines(oracle_lib, ref)
    assert np.array_equal(got["death_step"], ref["death"])
    for k in LINE_KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["final_depth"].tobytes() == ref["final_depth"].tobytes()
    assert got["final_pos"].tobytes() == ref["final_pos"].tobytes()


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
@pytest.mark.parametrize("key", WC.KEYS)
def test_attributes_along_pathlines_bit_exact(device, oracle_lib, capsys, key, euler):
    """Temperature and salinity along pathlines against tests/pathline_attr_reference.py: through the capture
    path (a window of 5 slots) on me7, through the sampler between launches on me12 and me20."""
    import torch
    from mops_amd.engine import ParticleSet, run_trajectories
    d = device(key)
    seeds, depths, cells = WC.sample_seeds(key)
    r0, r1 = WC.derived(key)
    times = WC.SAMPLE_TIMES
    ref = PR.run(d.mesh, r0, r1, seeds, depths, cells, *times, euler=euler)
    K = times[1] // times[2]
    nv = WC.degrees(d.mesh)[cells]
    _report(capsys, f"{key} attributes {'euler' if euler else 'rk4'}: {int(((nv >= 7) & (ref['death'] != 0)).sum())} "
                    f"particles in wide cells alive after step 0, {int(ref['cell_changes'].sum())} cell changes")
    assert ((nv >= 7) & (ref["death"] != 0)).sum() >= 40 and (not euler or ref["cell_changes"].sum() >= 40)
    cfg = _cfg(times, euler)
    if key == "me7":
        ps = ParticleSet(d.dm, seeds, depths, cfg, cells=cells, n_attr=2, capture_slots=5)
        ps.advance(d.f0, d.f1, 0, cfg.n_steps, attrs=([d.attrs[k][0] for k in NAMES], [d.attrs[k][1] for k in NAMES]))
        slab = torch.empty_like(ps.attr_records)     # [K][n_attr][slot] -> [K][n_attr][particle]
        slab[..., ps.ids.long()] = ps.attr_records
        assert np.array_equal(slab.cpu().numpy(),np.ascontiguousarray(ref["rec_attr"].transpose(1, 2, 0)))
        assert np.array_equal(ps.original(ps.death).cpu().numpy(), ref["death"])
        return
    got = run_trajectories(d.dm, d.f0, d.f1, cfg, seeds, depths=depths, cells=cells, attrs=d.attrs)
    want = PR.attr_lines(oracle_lib, seeds, ref, K)
    for a, name in enumerate(NAMES):
        assert np.array_equal(got["attributes"][name], want[a]), name
    assert np.array_equal(got["death_step"], ref["death"])


# ---- remapping ------------------------------------------------------------------------------------------------
def _assert_coverage(code):
    valid, other = WC.coverage(code)
    assert valid >= 0.4 * code.size and other >= 0.05 * code.size, (valid, other)


@pytest.mark.parametrize("rule", ["reference", "bracket"])
@pytest.mark.parametrize("win", sorted(WC.WINDOWS))
@pytest.mark.parametrize("key", WC.KEYS)
def test_fixed_depth_on_wide_cells(device, capsys, key, win, rule):
    """remap_fixed_*_kernel<7 / 12 / 20> with two attributes, and the cell map; every window reaches land."""
    from mops_amd import engine
    d = device(key)
    w, h, (lat, lon) = WC.WINDOWS[win]
    ref = WC.restated_depth(key, win, rule)
    _assert_coverage(ref["code"])
    _report(capsys, f"{key} fixed depth {win} ({rule}): valid pixels per degree "
                    f"{WC.valid_by_degree(d.mesh, WC.window_cells(key, win), ref['code'])}, {WC.coverage(ref['code'])[0]} of {w * h} in all")
    assert (ref["code"] == RR.OUTSIDE).any() and w != h and (w * h) % 64 != 0
    images, cells = engine.remap_fixed_depth(d.dm, d.f0, w, h, lat, lon, WC.IMAGE_DEPTH, n_attr=2,
                                             vertex_attrs=tuple(d.attrs[k][0] for k in NAMES), layer_rule=rule,
                                             return_cells=True)
    assert np.array_equal(cells.cpu().numpy().reshape(-1), WC.window_cells(key, win))
    got = images.cpu().numpy()
    assert got.shape == ref["images"].shape == (2, h, w, 4)
    assert np.array_equal(got, ref["images"], equal_nan=True)
    assert np.all(got[..., 3] == 1.0)


@pytest.mark.parametrize("win", sorted(WC.WINDOWS))
@pytest.mark.parametrize("key", WC.KEYS)
def test_fixed_layer_on_wide_cells(device, capsys, key, win):
    from mops_amd import engine
    d = device(key)
    w, h, (lat, lon) = WC.WINDOWS[win]
    ref = WC.restated_layer(key, win)
    _assert_coverage(ref["code"])
    _report(capsys, f"{key} fixed layer {win}: valid pixels per degree "
                    f"{WC.valid_by_degree(d.mesh, WC.window_cells(key, win), ref['code'])}")
    image, cells = engine.remap_fixed_layer(d.dm, d.f0, w, h, lat, lon, WC.IMAGE_LAYER, return_cells=True)
    assert np.array_equal(cells.cpu().numpy().reshape(-1), WC.window_cells(key, win))
    assert np.array_equal(image.cpu().numpy(), ref["image"], equal_nan=True)


@pytest.mark.parametrize("row", sorted(WC.LATITUDES))
@pytest.mark.parametrize("key", WC.KEYS)
def test_fixed_latitude_through_wheel_centres(device, capsys, key, row):
    from mops_amd import engine
    d = device(key)
    w, h, lon, lat = WC.LATITUDES[row]
    ref = WC.restated_latitude(key, row)
    _assert_coverage(ref["code"])
    _report(capsys, f"{key} fixed latitude {row}: valid pixels per degree "
                    f"{WC.valid_by_degree(d.mesh, WC.latitude_cells(key, row), ref['code'])}")
    assert len(np.unique(ref["layer"][ref["code"] == RR.VALID])) >= 3 and (w * h) % 64 != 0
    image, cells = engine.remap_fixed_latitude(d.dm, d.f0, w, h, lon, lat, WC.depth_range(d.mesh), return_cells=True)
    assert np.array_equal(cells.cpu().numpy(), WC.latitude_cells(key, row))
    assert np.array_equal(image.cpu().numpy(), ref["image"], equal_nan=True)


# ---- level bounds of the remapping kernels --------------------------------------------------------------------
GLOBAL = (48, 24, (-90.0, 90.0), (-180.0, 180.0))


@pytest.fixture(scope="module")
def plain(gpu, engine_lib, oracle_lib):
    """make_mesh(8, n_levels=L) on the device and in the oracle, per L."""
    from mops_amd import engine, synth
    cache = {}

    def get(levels):
        if levels not in cache:
            mesh = synth.make_mesh(8, n_levels=levels)
            snap = synth.make_snapshot(mesh)
            dm = engine.DeviceMesh.from_mesh(mesh)
            w, h, lat, lon = GLOBAL
            cache[levels] = dict(mesh=mesh, dm=dm, df=engine.DeviceField.from_snapshot(dm, snap),
                                 derived=oracle_lib.preprocess(mesh, snap),
                                 vattrs=tuple(engine.cell_to_vertex_attr(dm, snap.attributes[k]) for k in NAMES),
                                 cells=oracle_lib.knn(mesh, RR.depth_positions(w, h, lat, lon)))
        return cache[levels]
    return get


def test_fixed_layer_with_one_level(plain):
    """nVertLevels 1: remap_velocity reads the vertex array itself (one-level fields carry no per-level records).
    The restatement gives 1054 finite pixels of 1152."""
    from mops_amd import engine
    c = plain(1)
    w, h, lat, lon = GLOBAL
    ref = IR.fixed_layer(c["mesh"], c["derived"], w, h, lat, lon, 0, c["cells"])
    assert int((ref["code"] == RR.VALID).sum()) == 1054
    image, cells = engine.remap_fixed_layer(c["dm"], c["df"], w, h, lat, lon, 0, return_cells=True)
    assert np.array_equal(cells.cpu().numpy().reshape(-1), c["cells"])
    assert np.array_equal(image.cpu().numpy(), ref["image"], equal_nan=True)
    assert np.isfinite(ref["image"][ref["code"] == RR.VALID]).all()


@pytest.mark.parametrize("rule", ["reference", "bracket"])
@pytest.mark.parametrize("levels,valid", [(2, 970), (100, 1045), (101, 0), (1, 0)])
def test_fixed_depth_level_bounds(plain, levels, valid, rule):
    """VisualizeFixedDepth's bounds on nVertLevels (:338, `L <= 0 || L > 100`): 2 and 100 levels bit-exact at
    800 m, 970 and 1045 valid pixels of 1152; 101 levels and a single one give NaN everywhere, alpha 1."""
    from mops_amd import engine
    c = plain(levels)
    w, h, lat, lon = GLOBAL
    ref = RR.fixed_depth(c["mesh"], c["derived"], w, h, lat, lon, 800.0, c["cells"], layer_rule=rule)
    assert int((ref["code"] == RR.VALID).sum()) == valid
    got = engine.remap_fixed_depth(c["dm"], c["df"], w, h, lat, lon, 800.0, n_attr=2, vertex_attrs=c["vattrs"],
                                   layer_rule=rule).cpu().numpy()
    assert np.array_equal(got, ref["images"], equal_nan=True)
    assert np.all(got[..., 3] == 1.0)
    if valid == 0:
        assert np.isnan(got[..., :3]).all()
