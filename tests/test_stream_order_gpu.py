"""GPU: the analysis and imaging entries on a stream that is not torch's current one.

Every entry that takes ``stream=`` (and the few documented to run on torch's current stream, called under
``torch.cuda.stream(side)``) is handed an input that is still on its way on ``side`` -- the harness of
tests/stream_case.py -- and must give, after ``side.synchronize()`` alone, the bytes it gives from that input on the
default stream.  A part of an entry that runs on another stream reads the stale input and changes the bytes.  Each
case runs with the ``torch.cuda.Stream`` object and with its raw handle, prints the sleep it used, and a few are also
held against the numpy restatements directly.  The last test runs four of the entries from two threads at once.

The module stands on the positive control of ``stream_case.Harness`` (torch only): where that fails, every case
fails with it."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import census_case as CC  # noqa: E402
import census_reference as CR  # noqa: E402
import eddy_reference as ER  # noqa: E402
import ftle_reference as F  # noqa: E402
import pathline_attr_reference as R  # noqa: E402
import remap_reference as RR  # noqa: E402
import section_reference as SR  # noqa: E402
import stream_case as SC  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = SC.FORMS
RAW_KEYS = ("layerThickness", "bottomDepth", "zonalVelocity", "meridionalVelocity", "vertVelocityTop")
# the odd window of test_remap_gpu.py and test_image_cpp.py: 37 x 23 = 851 pixels, no multiple of 64, W != H
W, H = 37, 23
LAT, LON = (-75.0, 80.0), (-180.0, 175.0)
DEPTH, LATITUDE, FIXED_LAYER = 300.0, 20.0, 4.0
PATH, SECTION_H = [(-30.0, -20.0), (50.0, 80.0)], 20
# the lattice of test_ftle_gpu.py's end-to-end cases and its 36 steps, with MOPS_RK4: particles die at cell
# crossings (quirk Q1) with a finite last point, so the death steps decide pixels
LATTICE = dict(W=24, H=16, lat=(-80.0, 80.0), lon=(-180.0, 180.0), depth=300.0)
N_STEPS, HALF = R.DURATION // R.DELTA_T, 18
HORIZON = R.DURATION / 86400.0
DENSITY = (361, 179, (-90.0, 90.0), (-180.0, 180.0))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(t, want):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()


@pytest.fixture(scope="module")
def harness(engine_lib, gpu):
    """The side stream, the sleep's calibration and the positive control; every case depends on it."""
    h = SC.Harness()
    yield h
    total = sum(ms for _, ms in h.delays)
    print(f"\nstream order: {len(h.delays)} late-input runs, {total:.0f} ms of sleep in all, the longest "
          f"{max([ms for _, ms in h.delays] or [0.0]):.0f} ms")


@pytest.fixture(scope="module")
def world(harness, engine_lib, oracle_lib, small_case):
    """The small culled mesh on the device; ``late``: the field the cases rebuild in place (real: snapshot 0, stale:
    snapshot 1) from raw snapshots kept in HBM; ``f``: the two snapshots as fixed fields."""
    import torch
    from mops_amd import engine
    c = dict(CC.small(oracle_lib, small_case))
    c["O"], c["small_case"] = oracle_lib, small_case
    dm = c["dm"] = engine.DeviceMesh.from_mesh(c["mesh"])
    c["raw"] = [{k: torch.as_tensor(getattr(s, k), device="cuda") for k in RAW_KEYS} for s in (c["s0"], c["s1"])]
    torch.cuda.synchronize()
    c["late"] = engine.DeviceField.from_device_snapshot(dm, c["raw"][1], timestep=1)
    c["real_field"] = SC.rebuild(c["late"], c["raw"][0], 0)
    c["stale_field"] = SC.rebuild(c["late"], c["raw"][1], 1)
    c["f"] = [engine.DeviceField.from_snapshot(dm, c["s0"]), engine.DeviceField.from_snapshot(dm, c["s1"])]
    names = sorted(c["s0"].attributes)
    assert names[:2] == ["salinity", "temperature"]
    c["names"] = names[:2]
    c["vreal"] = [engine.cell_to_vertex_attr(dm, c["s0"].attributes[k]) for k in c["names"]]
    c["vstale"] = [0.5 * v + 1.0 for v in c["vreal"]]              # other finite vertex arrays
    c["vbuf"] = [v.clone() for v in c["vreal"]]
    c["drange"] = (float(c["mesh"].refBottomDepth[0]), float(c["mesh"].refBottomDepth[-1]))
    c["gdev"] = [{k: _dev(g[k]) for k in ("vorticity", "okubo_weiss")} for g in (c["g0"], c["g1"])]
    c["area_dev"] = _dev(c["area"])
    c["classes"] = CC.synthetic_classes(c["mesh"])
    torch.cuda.synchronize()
    return c


def test_positive_control(harness):
    """Torch only: a clone on the default stream sees the stale bytes, a clone on the side stream the late ones."""
    print(f"positive control: delay {harness.control['delay_ms']:.0f} ms at "
          f"{harness.control['cycles_per_ms']:.0f} sleep cycles per ms")
    assert harness.control["cycles_per_ms"] > 0


# ---- 1. the velocity gradient ---------------------------------------------------------------------------------
@pytest.mark.parametrize("vertex", [False, True], ids=["cells", "vertices"])
@pytest.mark.parametrize("form", FORMS)
def test_velocity_gradient(harness, world, form, vertex):
    from mops_amd import engine
    c = world
    got, _ = harness.case(f"velocity_gradient({'vertex' if vertex else 'cell'})", form, c["stale_field"],
                          c["real_field"],
                          lambda st: engine.velocity_gradient(c["dm"], c["late"], vertex=vertex, stream=st))
    assert tuple(got) == ER.NAMES
    want = c["v0"] if vertex else c["g0"]                            # the restatement, directly
    for k in (sorted(c["v0"]) if vertex else ER.NAMES):
        assert _same(got[k], want[k]), k


# ---- 2. cell_to_vertex_attr: torch's current stream -------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_cell_to_vertex_attr_under_a_stream_context(harness, world, form):
    from mops_amd import engine
    c = world
    real, stale = (_dev(g["okubo_weiss"]).reshape(-1) for g in (c["g0"], c["g1"]))
    buf = real.clone()
    got, _ = harness.case("cell_to_vertex_attr", form, SC.copy_into(buf, stale), SC.copy_into(buf, real),
                          lambda st: SC.under(st, lambda: engine.cell_to_vertex_attr(c["dm"], buf, signed=True)))
    assert _same(got, c["v0"]["okubo_weiss"])


# ---- 3. the census, piece by piece --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_eddy_classify(harness, world, form):
    from mops_amd import engine
    c = world
    thr = c["thresholds"][0.2]
    ow, vo = c["gdev"][0]["okubo_weiss"].clone(), c["gdev"][0]["vorticity"].clone()
    write = [SC.both(SC.copy_into(ow, g["okubo_weiss"]), SC.copy_into(vo, g["vorticity"])) for g in c["gdev"]]
    got, _ = harness.case("eddy_classify", form, write[1], write[0],
                          lambda st: engine.eddy_classify(c["dm"], ow, vo, CC.LAYER, thr, stream=st))
    assert _same(got, CR.classify(c["g0"]["okubo_weiss"], c["g0"]["vorticity"], CC.LAYER, thr))


@pytest.mark.parametrize("form", FORMS)
def test_label_components(harness, world, form):
    from mops_amd import engine
    c = world
    real, stale = _dev(c["classes"]["band"]), _dev(c["classes"]["random"])
    buf = real.clone()
    got, _ = harness.case("label_components", form, SC.copy_into(buf, stale), SC.copy_into(buf, real),
                          lambda st: engine.label_components(c["dm"], buf, stream=st))
    assert _same(got, CR.label_components(c["mesh"], c["classes"]["band"]))


@pytest.mark.parametrize("form", FORMS)
def test_eddy_table(harness, world, form):
    """Late labels and classes; both states are the component and class arrays of a census of the mesh."""
    from mops_amd import engine
    c = world
    refs = [CC.census(c["O"], c["small_case"], k, 1) for k in (0.2, 0.05)]
    assert refs[0]["E"] > 0 and refs[1]["E"] > 0
    src = [(_dev(r["components"]), _dev(r["classes"])) for r in refs]
    lab, cls = src[0][0].clone(), src[0][1].clone()
    write = [SC.both(SC.copy_into(lab, a), SC.copy_into(cls, b)) for a, b in src]
    g = c["gdev"][0]
    got, _ = harness.case("eddy_table", form, write[1], write[0],
                          lambda st: engine.eddy_table(c["dm"], lab, cls, c["area_dev"], g["vorticity"],
                                                       g["okubo_weiss"], CC.LAYER, 1, stream=st))
    assert _same(got[0], refs[0]["labels"])
    for k in engine.EDDY_COLUMNS:
        assert got[1][k].tobytes() == refs[0]["table"][k].tobytes(), k


@pytest.mark.parametrize("form", FORMS)
def test_cell_area(harness, world, form):
    """No late input exists (the entry reads the mesh alone): the bytes after ``side.synchronize()`` alone."""
    import torch
    from mops_amd import engine
    want = engine.cell_area(world["dm"])
    torch.cuda.synchronize()
    got = engine.cell_area(world["dm"], stream=harness.form(form))
    harness.side.synchronize()
    assert SC.to_bytes(got) == SC.to_bytes(want) and _same(got, world["area"])


def _census_result(cen):
    return dict(classes=cen.classes, components=cen.components, labels=cen.labels, table=cen.table,
                threshold=cen.threshold)


@pytest.mark.parametrize("form", FORMS)
def test_eddy_census_under_a_stream_context(harness, world, form):
    """``eddy_census`` has no ``stream=``: it runs on torch's current stream, here ``side``, with a late field."""
    from mops_amd import engine
    c = world
    thr = c["thresholds"][0.2]
    got, _ = harness.case(
        "eddy_census", form, c["stale_field"], c["real_field"],
        lambda st: SC.under(st, lambda: _census_result(
            engine.eddy_census(c["dm"], c["late"], layer=CC.LAYER, threshold=thr, min_cells=4))))
    ref = CC.census(c["O"], c["small_case"], 0.2, 4)
    assert ref["E"] > 0
    assert _same(got["classes"], ref["classes"]) and _same(got["labels"], ref["labels"])
    assert sorted(got["table"]) == sorted(ref["table"])
    for k in ref["table"]:
        assert got["table"][k].tobytes() == ref["table"][k].tobytes(), k


@pytest.mark.parametrize("form", FORMS)
def test_census_image(harness, world, form):
    """``EddyCensus.image(stream=side)``: the fixed-layer remap (late field) and the torch gather behind it (late
    labels) both on ``side``."""
    import torch
    from mops_amd import engine
    c = world
    c["real_field"]()
    torch.cuda.synchronize()
    cen = engine.eddy_census(c["dm"], c["late"], layer=CC.LAYER, threshold=c["thresholds"][0.05], min_cells=4)
    real = cen.labels.clone()
    stale = _dev(CC.census(c["O"], c["small_case"], 0.2, 4)["labels"])      # another census's eddy indices
    assert real.dtype == stale.dtype and not torch.equal(real, stale)
    got, _ = harness.case("EddyCensus.image", form, SC.both(c["stale_field"], SC.copy_into(cen.labels, stale)),
                          SC.both(c["real_field"], SC.copy_into(cen.labels, real)),
                          lambda st: cen.image(W, H, LAT, LON, return_cells=True, stream=st))
    img, _, layer_image = (t.cpu().numpy() for t in got)
    nan = np.isnan(layer_image[..., 0])
    inside = ~np.isnan(img[..., 0])
    assert nan.any() and inside.any() and not (inside & nan).any()    # NaN pixels follow the layer image


# ---- 4. the remaps ------------------------------------------------------------------------------------------------
def _late_field_and_attrs(c, n):
    stale = SC.both(c["stale_field"], *[SC.copy_into(c["vbuf"][k], c["vstale"][k]) for k in range(n)])
    real = SC.both(c["real_field"], *[SC.copy_into(c["vbuf"][k], c["vreal"][k]) for k in range(n)])
    return stale, real


@pytest.mark.parametrize("form", FORMS)
def test_remap_fixed_depth(harness, world, form):
    from mops_amd import engine
    c = world
    stale, real = _late_field_and_attrs(c, 2)
    got, _ = harness.case("remap_fixed_depth", form, stale, real,
                          lambda st: engine.remap_fixed_depth(c["dm"], c["late"], W, H, LAT, LON, DEPTH, n_attr=2,
                                                              vertex_attrs=tuple(c["vbuf"]), return_cells=True,
                                                              stream=st))
    if form == FORMS[0]:                                              # the restatement, directly, once
        d = c["d0"]
        derived = c["O"].Derived(d.vertex_ztop, d.vertex_vel, d.vertex_w, {k: d.attrs[k] for k in c["names"]})
        cells = c["O"].knn(c["mesh"], RR.depth_positions(W, H, LAT, LON))
        ref = RR.fixed_depth(c["mesh"], derived, W, H, LAT, LON, DEPTH, cells)
        valid = int((ref["code"] == RR.VALID).sum())
        assert 0.4 * W * H <= valid <= 0.95 * W * H
        images = got[0].cpu().numpy()
        assert np.array_equal(got[1].cpu().numpy().reshape(-1), cells)
        for k in range(2):
            assert np.array_equal(images[k], ref["images"][k], equal_nan=True), k


@pytest.mark.parametrize("form", FORMS)
def test_remap_fixed_latitude(harness, world, form):
    from mops_amd import engine
    c = world
    got, _ = harness.case("remap_fixed_latitude", form, c["stale_field"], c["real_field"],
                          lambda st: engine.remap_fixed_latitude(c["dm"], c["late"], W, H, LON, LATITUDE, c["drange"],
                                                                 return_cells=True, stream=st))
    image = got[0].cpu().numpy()
    assert np.isfinite(image[..., 0]).any() and np.isnan(image[..., 0]).any()


@pytest.mark.parametrize("form", FORMS)
def test_remap_fixed_layer(harness, world, form):
    from mops_amd import engine
    c = world
    got, _ = harness.case("remap_fixed_layer", form, c["stale_field"], c["real_field"],
                          lambda st: engine.remap_fixed_layer(c["dm"], c["late"], W, H, LAT, LON, FIXED_LAYER,
                                                              return_cells=True, stream=st))
    image = got[0].cpu().numpy()
    assert np.isfinite(image[..., 0]).any() and np.isnan(image[..., 0]).any()


@pytest.mark.parametrize("form", FORMS)
def test_remap_section(harness, world, form):
    from mops_amd import engine
    c = world
    stale, real = _late_field_and_attrs(c, 1)
    got, _ = harness.case("remap_section", form, stale, real,
                          lambda st: engine.remap_section(c["dm"], c["late"], PATH, W, SECTION_H, c["drange"],
                                                          vertex_attrs=(c["vbuf"][0],), return_cells=True, stream=st))
    if form == FORMS[0]:                                              # the restatement, directly, once
        pts, nrm, dist = SR.section_points(PATH, W)
        cells = c["O"].knn(c["mesh"], pts)
        ref = SR.section(c["mesh"], c["d0"], pts, nrm, SECTION_H, c["drange"], cells,
                         attrs=[c["d0"].attrs[c["names"][0]]])
        valid = ref["code"] == RR.VALID
        assert valid.any() and (~valid).any()
        assert got[1].tobytes() == dist.tobytes() and np.array_equal(got[2].cpu().numpy(), cells)
        assert np.array_equal(got[0].cpu().numpy(), ref["images"], equal_nan=True)


# ---- 5. the colour pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minmax", [False, True], ids=["rgba", "rgba+minmax"])
@pytest.mark.parametrize("form", FORMS)
def test_colormap_rgba(harness, world, form, minmax):
    import torch
    from mops_amd import engine
    c = world
    real, stale = (engine.remap_fixed_layer(c["dm"], f, W, H, LAT, LON, FIXED_LAYER) for f in c["f"])
    torch.cuda.synchronize()
    assert bool(torch.isnan(real[..., 0]).any()) and bool(torch.isfinite(real[..., 0]).any())
    buf = real.clone()
    harness.case(f"colormap_rgba(minmax={minmax})", form, SC.copy_into(buf, stale), SC.copy_into(buf, real),
                 lambda st: engine.colormap_rgba(buf, return_minmax=minmax, stream=st))


# ---- 6. to 8.: a lattice of particles --------------------------------------------------------------------------------
class _Flow:
    """One ParticleSet on the lattice's seeds, advanced through the late field (front) and snapshot 1 (back)."""

    def __init__(self, c, record_t):
        import torch
        from mops_amd.engine import FlowMapLattice, ParticleSet, TrajectoryConfig
        self.c, self.torch = c, torch
        self.lat = FlowMapLattice(LATTICE["W"], LATTICE["H"], LATTICE["lat"], LATTICE["lon"])
        cfg = TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=record_t,
                               depth=LATTICE["depth"], method=0)
        self.ps = ParticleSet(c["dm"], self.lat.seeds, LATTICE["depth"], cfg)
        self.n = self.ps.n
        # what the two fields give, on the default stream: last points and deaths in seed order, and the lines
        self.last, self.death, self.points = [], [], []
        for write in (c["real_field"], c["stale_field"]):
            write()
            self.reseed()
            torch.cuda.synchronize()
            self.advance(None)
            self.last.append(self.ps.last_points().clone())
            self.death.append(self.ps.original(self.ps.death).clone())
            self.points.append(self.ps.finalize(pathline=True)["points"].clone())
            torch.cuda.synchronize()
        dead = [int((d >= 0).sum()) for d in self.death]
        assert 0 < dead[0] < self.n and 0 < dead[1] < self.n
        assert not torch.equal(self.last[0], self.last[1]) and not torch.equal(self.death[0], self.death[1])

    def reseed(self):
        self.ps.reseed(self.lat.seeds, LATTICE["depth"])

    def advance(self, st):
        self.ps.advance(self.c["late"], self.c["f"][1], 0, N_STEPS, stream=st)

    def advance_compacted(self, st):
        """The same steps with a dead-particle compaction half way, all on ``st``."""
        ps = self.ps
        ps.advance(self.c["late"], self.c["f"][1], 0, HALF, stream=st)
        nrec = min(ps.K, HALF // ps.record_period(pathline=True) + 1)
        live = ps.compact(0, ps.n, st if st is not None else self.torch.cuda.current_stream(), records_written=nrec)
        ps.advance(self.c["late"], self.c["f"][1], HALF, N_STEPS, stream=st, live_count=live)


@pytest.fixture(scope="module")
def flow(world):
    return _Flow(world, R.RECORD_T)


@pytest.fixture(scope="module")
def flow_one_record(world):
    """One record per run: a particle that dies keeps its pre-written seed as its last point (quirks Q1, a9), so
    only its death step makes its pixel NaN -- with more records a dead particle's last point is zero already and
    the death steps decide nothing."""
    return _Flow(world, R.DURATION)


@pytest.mark.parametrize("value", [None, "speed"], ids=["count", "speed"])
@pytest.mark.parametrize("form", FORMS)
def test_density_map_behind_an_advance(harness, world, flow, form, value):
    """advance, ``accumulate(seeds=True)`` and ``image`` on ``side`` with no host synchronisation between them: the
    records the map bins are still being written when ``accumulate`` returns."""
    from mops_amd.engine import DensityMap
    m = DensityMap(*DENSITY, value=value)

    def before():
        flow.reseed()
        m.reset()

    def entry(st):
        flow.advance(st)
        m.accumulate(flow.ps, seeds=True, stream=st)
        return m.image(stream=st), m.accum

    got, _ = harness.case(f"DensityMap({value})", form, world["stale_field"], world["real_field"], entry, before=before,
                          no_host_sync=True)
    accum = got[1].cpu().numpy()
    assert int(accum[..., 0].sum()) > 0 and (value is None) == (not accum[..., 1].any())


@pytest.mark.parametrize("form", FORMS)
def test_density_accumulate_lines_under_a_stream_context(harness, world, flow, form):
    from mops_amd.engine import DensityMap
    m = DensityMap(*DENSITY)
    buf = flow.points[0].clone()

    def entry(st):
        SC.under(st, lambda: m.accumulate_lines(buf))
        return m.accum

    harness.case("DensityMap.accumulate_lines", form, SC.copy_into(buf, flow.points[1]),
                 SC.copy_into(buf, flow.points[0]), entry, before=m.reset)


@pytest.mark.parametrize("kind", ["contiguous", "sliced", "death_int64"])
@pytest.mark.parametrize("form", FORMS)
def test_ftle_of_late_inputs(harness, world, flow, form, kind):
    """``FlowMapLattice.ftle(stream=side)``: a late contiguous ``last``; a late [n, 4] tensor sliced to [:, :3] (the
    ``.contiguous()`` copy); a late int64 ``death`` (the ``.to(int32)`` copy)."""
    import torch
    lat = flow.lat
    last, death = flow.last[0].clone(), flow.death[0].clone()
    if kind == "contiguous":
        arg = last
        stale, real = SC.copy_into(last, flow.last[1]), SC.copy_into(last, flow.last[0])
    elif kind == "sliced":
        wide = torch.zeros((flow.n, 4), dtype=torch.float64, device="cuda")
        arg = wide[:, :3]
        assert not arg.is_contiguous()
        stale, real = SC.copy_into(arg, flow.last[1]), SC.copy_into(arg, flow.last[0])
    else:
        arg = last
        death = death.long()
        stale, real = SC.copy_into(death, flow.death[1].long()), SC.copy_into(death, flow.death[0].long())
    torch.cuda.synchronize()
    got, _ = harness.case(f"FlowMapLattice.ftle({kind})", form, stale, real,
                          lambda st: lat.ftle(arg, death, HORIZON, stream=st), no_host_sync=True)
    if (kind, form) == ("contiguous", FORMS[0]):                      # the restatement, directly, once
        img = got.cpu().numpy()
        want = F.ftle_image(lat.width, lat.height, lat.seeds.cpu().numpy(), flow.last[0].cpu().numpy(),
                            flow.death[0].cpu().numpy(), HORIZON, lat.wrap_lon)
        valid = ~np.isnan(want[:, :, 1])
        assert valid.any() and (~valid).any()
        for ch in (1, 2):
            assert img[:, :, ch].tobytes() == want[:, :, ch].tobytes(), ch
        assert np.array_equal(np.isnan(img[:, :, 0]), ~valid) and np.all(img[:, :, 3] == 1.0)


@pytest.mark.parametrize("form", FORMS)
def test_ftle_from_behind_an_advance(harness, world, flow_one_record, form):
    """``ftle_from(ps, horizon, stream=side)`` straight behind an advance with a compaction on ``side``: the death
    steps are put back in seed order (torch) while they and the slot ids are still being written."""
    import torch
    flow = flow_one_record
    lat, ps = flow.lat, flow.ps
    assert ps.K == 1
    # what a reordering on the wrong stream would hand the kernel: nobody dead yet -- another image
    alive = torch.full((flow.n,), -1, dtype=torch.int32, device="cuda")
    assert SC.to_bytes(lat.ftle(flow.last[0], alive, HORIZON)) != SC.to_bytes(lat.ftle(flow.last[0], flow.death[0],
                                                                                         HORIZON))

    def entry(st):
        flow.advance_compacted(st)
        return lat.ftle_from(ps, HORIZON, stream=st)

    got, _ = harness.case("FlowMapLattice.ftle_from", form, world["stale_field"], world["real_field"], entry,
                          before=flow.reseed, no_host_sync=True)
    ids = ps.ids.cpu().numpy()
    assert not np.array_equal(ids, np.arange(flow.n)) and np.array_equal(np.sort(ids), np.arange(flow.n))
    assert SC.to_bytes(got) == SC.to_bytes(lat.ftle(flow.last[0], flow.death[0], HORIZON))   # a compaction keeps them


@pytest.mark.parametrize("form", FORMS)
def test_last_points_behind_an_advance(harness, world, flow, form):
    def entry(st):
        flow.advance(st)
        return flow.ps.last_points(stream=st)

    got, _ = harness.case("ParticleSet.last_points", form, world["stale_field"], world["real_field"], entry,
                          before=flow.reseed, no_host_sync=True)
    assert SC.to_bytes(got) == SC.to_bytes(flow.last[0])


# ---- 9. two streams at once ------------------------------------------------------------------------------------------
def test_two_threads_two_streams_one_mesh(harness, world, engine_lib):
    """Two threads, each with its own side stream and its own field on the one mesh, four rounds each of the entries
    that allocate per-call scratch or synchronise: every result has the bytes of its serial truth, and no thread
    leaves an error message behind."""
    import torch
    from mops_amd import engine
    c = world
    dm = c["dm"]
    refs = [CC.census(c["O"], c["small_case"], k, 1) for k in (0.2, 0.05)]
    per = []
    for i in range(2):
        per.append(dict(field=c["f"][i], vattrs=tuple(c["vreal"] if i == 0 else c["vstale"]),
                        classes=_dev(c["classes"]["band" if i == 0 else "random"]),
                        labels=_dev(refs[i]["components"]), cls=_dev(refs[i]["classes"])))
    g = c["gdev"][0]
    torch.cuda.synchronize()

    def one(i, st):
        p = per[i]
        out = [engine.remap_fixed_depth(dm, p["field"], W, H, LAT, LON, DEPTH, n_attr=2, vertex_attrs=p["vattrs"],
                                        return_cells=True, stream=st),
               engine.velocity_gradient(dm, p["field"], stream=st),
               engine.label_components(dm, p["classes"], stream=st),
               engine.eddy_table(dm, p["labels"], p["cls"], c["area_dev"], g["vorticity"], g["okubo_weiss"], CC.LAYER,
                                 1, stream=st)]
        if st is not None:
            st.synchronize()
        else:
            torch.cuda.synchronize()
        return [SC.to_bytes(o) for o in out]

    want = [one(i, None) for i in range(2)]
    assert all(a != b for a, b in zip(*want))                         # the two threads compute different things
    got, errors = [[], []], []
    start = threading.Barrier(2)

    def worker(i):
        try:
            torch.cuda.set_device(0)
            side = torch.cuda.Stream()
            start.wait(timeout=60)
            for _ in range(4):
                got[i].append(one(i, side))
            assert engine_lib.mops_last_error() == b"", engine_lib.mops_last_error()
        except BaseException as e:  # noqa: BLE001 -- handed to the main thread
            errors.append((i, e))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    names = ("remap_fixed_depth", "velocity_gradient", "label_components", "eddy_table")
    for i in range(2):
        assert len(got[i]) == 4
        for r, res in enumerate(got[i]):
            for name, a, b in zip(names, res, want[i]):
                assert a == b, f"thread {i}, round {r}, {name}: " + SC.first_difference(a, b)
