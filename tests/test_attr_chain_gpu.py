"""GPU: temperature and salinity along chained pathlines (PathlineChain.run(attrs=True), MOPSPathline.run(
sample_attributes=True)) against the Python restatement of the reference's loop run pair by pair with the
reference caller's seed and depth rules (tests/test_chain.py's oracle_chain), and every mode of the chain against
its keep_lines result.  Every assertion is bit-exact."""
import importlib.util
import os
import weakref

import numpy as np
import pytest

import pathline_attr_reference as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EARTH_RADIUS_M = 6_371_000.0
NAMES = ["salinity", "temperature"]  # std::map order
GAP, DT, RT = 21600, 600, 3600
LINE_KEYS = ("points", "velocity", "lastPoint")


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _Setup:
    """Three synth snapshots on small_case with their device mesh and oracle preprocessing, shared by the module."""

    def __init__(self, O, mesh, n_snap=3):
        from mops_amd import synth
        from mops_amd.engine import DeviceMesh
        self.O, self.mesh = O, mesh
        self.snaps = [synth.make_snapshot(mesh, timestep=t, phase=0.35 * t) for t in range(n_snap)]
        self.derived = [O.preprocess(mesh, s) for s in self.snaps]
        self.dm = DeviceMesh.from_mesh(mesh)
        self.seeds = synth.uniform_band_seeds(120, seed=8)
        self._ref = {}
        self._keep = {}

    def chain(self, n=None, **kw):
        from mops_amd.chain import PathlineChain, snapshot_attr_factory, snapshot_field_factory
        n = n or len(self.snaps)
        if "timestamps" not in kw:
            kw.setdefault("gap_seconds", GAP)
        return PathlineChain(self.dm, snapshot_field_factory(self.dm, lambda i: self.snaps[i]), n,
                             make_attrs=snapshot_attr_factory(self.dm, lambda i: self.snaps[i]), **kw)

    def reference(self, euler, follow_last, per_particle):
        """MOPSPathline.run's rules (oracle_chain) on the restatement with its attribute channel; once per key."""
        key = (euler, follow_last, per_particle)
        if key in self._ref:
            return self._ref[key]
        O, seeds = self.O, self.seeds
        pdep = np.linspace(20.0, 600.0, len(seeds)).astype(np.float32) if per_particle else None
        att, last = [], None
        K = GAP // RT
        for p in range(len(self.snaps) - 1):
            s = seeds if (p == 0 or not follow_last) else last
            if pdep is not None and p > 0:
                pdep = np.clip(EARTH_RADIUS_M - np.linalg.norm(last, axis=1), 0.0, None).astype(np.float32)
            depths = pdep if pdep is not None else np.full(len(seeds), 300.0, dtype=np.float32)
            r = R.run(self.mesh, self.derived[p], self.derived[p + 1], s, depths, O.knn(self.mesh, s), DT, GAP, RT,
                      euler=euler)
            lines = R.attr_lines(O, s, r, K)
            att.append(lines[:, :, (0 if p == 0 else 1):])
            last = O.finalize_lines(s, r["rec_pos"], r["rec_vel"], K, with_attrs=False)["lastPoint"].copy()
        self._ref[key] = np.concatenate(att, 2)
        return self._ref[key]

    def keep(self, euler, **kw):
        """The keep_lines result of the default chain with attributes (the modes' reference), once per method."""
        if euler not in self._keep:
            got = self.chain().run(self.seeds, depth=300.0, method=1 if euler else 0, delta_t=DT, record_t=RT, attrs=True)
            self._keep[euler] = _host(got)
        return self._keep[euler]


def _host(res):
    out = {k: v.cpu().numpy() for k, v in res.items() if k != "attributes" and hasattr(v, "cpu")}
    if "attributes" in res:
        out["attributes"] = {k: v.cpu().numpy() for k, v in res["attributes"].items()}
    return out


@pytest.fixture(scope="module")
def setup(gpu, engine_lib, oracle_lib, small_case):
    return _Setup(oracle_lib, small_case[0])


@pytest.mark.parametrize("euler,follow_last,per_particle",
                         [(True, True, False), (False, True, False), (True, False, True), (False, True, True)],
                         ids=["euler", "rk4", "euler-perparticle-nofollow", "rk4-perparticle"])
def test_chain_attrs_match_restatement(setup, euler, follow_last, per_particle):
    pd = np.linspace(20.0, 600.0, len(setup.seeds)).astype(np.float32) if per_particle else None
    kw = dict(depth=300.0, particle_depths=pd, method=1 if euler else 0, delta_t=DT, record_t=RT,
              follow_last=follow_last)
    got = _host(setup.chain().run(setup.seeds, attrs=True, **kw))  # (RK4: compaction on by default)
    plain = _host(setup.chain().run(setup.seeds, **kw))
    want = setup.reference(euler, follow_last, per_particle)
    assert list(got["attributes"]) == NAMES and want.shape == (2, len(setup.seeds), 7 + 6)
    for a, name in enumerate(NAMES):
        assert np.array_equal(got["attributes"][name], want[a]), name
        assert np.array_equal(got[name], want[a]), name
    assert want[1].any()
    for k in LINE_KEYS + ("death_step",):
        assert got[k].tobytes() == plain[k].tobytes(), k
    # attrs off: no attributes key, quirk Q9 stays
    assert "attributes" not in plain
    assert np.array_equal(plain["temperature"], plain["velocity"][:, :, 0])
    assert np.array_equal(plain["salinity"], plain["velocity"][:, :, 1])
    # the split path gives the same bytes as the capture path
    split = _host(setup.chain().run(setup.seeds, attrs=True, capture_slots=0, **kw))
    for name in NAMES:
        assert split["attributes"][name].tobytes() == got["attributes"][name].tobytes(), name


def gpu_device():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _same_lines(got, want):
    for k in ("points", "velocity", "temperature", "salinity", "lastPoint"):
        assert got[k].tobytes() == want[k].tobytes(), k
    for name in NAMES:
        assert got["attributes"][name].tobytes() == want["attributes"][name].tobytes(), name


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_defer_lines(setup, euler):
    want = setup.keep(euler)
    got = setup.chain().run(setup.seeds, depth=300.0, method=1 if euler else 0, delta_t=DT, record_t=RT, attrs=True,
                            defer_lines=True)
    _same_lines(_host(got), want)


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_on_lines_chunks(setup, euler):
    import torch
    want = setup.keep(euler)
    n = len(setup.seeds)
    acc = {k: np.zeros_like(want[k]) for k in ("points", "velocity", "temperature", "salinity")}
    att = np.zeros((2, n, 13))
    col = {}

    def hook(p, lines, ids):
        i = ids.long().cpu().numpy()
        w = lines["points"].shape[1]
        c0 = col.setdefault(p, 0 if p == 0 else 7 + 6 * (p - 1))
        assert lines["attributes"].shape == (2, len(i), w) and len(i) <= 37
        for k in acc:
            acc[k][i, c0:c0 + w] = lines[k].cpu().numpy()
        att[:, i, c0:c0 + w] = lines["attributes"].cpu().numpy()

    res = setup.chain().run(setup.seeds, depth=300.0, method=1 if euler else 0, delta_t=DT, record_t=RT, attrs=True,
                            keep_lines=False, on_lines=hook, lines_chunk=37)
    torch.cuda.synchronize()
    for k in acc:
        assert acc[k].tobytes() == want[k].tobytes(), k
    for a, name in enumerate(NAMES):
        assert att[a].tobytes() == want["attributes"][name].tobytes(), name
    assert np.array_equal(res["lastPoint"].cpu().numpy(), want["lastPoint"]) and "attributes" not in res


def test_host_line_sink_carries_the_named_attributes(setup):
    from mops_amd.chain import HostLineSink
    want = setup.keep(True)
    n = len(setup.seeds)
    sink = HostLineSink(n, GAP // RT, gpu_device(), keep_all=True)
    setup.chain().run(setup.seeds, depth=300.0, method=1, delta_t=DT, record_t=RT, attrs=True, keep_lines=False,
                      on_lines=sink, lines_chunk=50)
    sink.synchronize()
    c0 = 0
    for p in range(2):
        h = sink.host(p)
        ids = h["ids"].numpy().astype(np.int64)
        w = h["points"].shape[1]
        for k in ("points", "temperature", "salinity"):
            assert np.array_equal(h[k].numpy(), want[k][ids, c0:c0 + w]), (p, k)
        c0 += w
    assert c0 == 13


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_unequal_pairs(gpu, engine_lib, oracle_lib, small_case, euler):
    """6 h / 2 h / 4 h pairs by timestamps: the slabs hold the longest pair; every mode of sampling agrees, and
    each pair's piece is what a two-snapshot chain of that pair alone samples from the same seeds."""
    from mops_amd.chain import pair_gaps
    s = _Setup(oracle_lib, small_case[0], n_snap=4)
    ts = ["0001-01-01_00:00:00", "0001-01-01_06:00:00", "0001-01-01_08:00:00", "0001-01-01_12:00:00"]
    assert pair_gaps(ts) == [21600, 7200, 14400]
    kw = dict(depth=300.0, method=1 if euler else 0, delta_t=DT, record_t=RT, attrs=True)
    got = _host(s.chain(timestamps=ts).run(s.seeds, follow_last=False, **kw))
    assert got["attributes"]["temperature"].shape == (len(s.seeds), 1 + 6 + 2 + 4)
    _same_lines(_host(s.chain(timestamps=ts).run(s.seeds, follow_last=False, capture_slots=0, **kw)), got)
    _same_lines(_host(s.chain(timestamps=ts).run(s.seeds, follow_last=False, defer_lines=True, **kw)), got)
    # pair 1 alone (follow_last=False: the same seeds): snapshots 1, 2 with a 2 h gap
    from mops_amd.chain import PathlineChain, snapshot_attr_factory, snapshot_field_factory
    one = PathlineChain(s.dm, snapshot_field_factory(s.dm, lambda i: s.snaps[i + 1]), 2, gap_seconds=7200,
                        make_attrs=snapshot_attr_factory(s.dm, lambda i: s.snaps[i + 1]))
    alone = _host(one.run(s.seeds, **kw))
    for name in NAMES:
        assert np.array_equal(got["attributes"][name][:, 7:9], alone["attributes"][name][:, 1:]), name
    assert np.array_equal(got["points"][:, 7:9], alone["points"][:, 1:])


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_segments_with_reorder_and_small_window(setup, euler):
    want = setup.keep(euler)
    got = setup.chain().run(setup.seeds, depth=300.0, method=1 if euler else 0, delta_t=DT, record_t=RT, attrs=True,
                            segment_steps=7, reorder=True, capture_slots=2, compact=False)
    _same_lines(_host(got), want)
    if not euler:  # and with the compaction between the 7-step launches
        got = setup.chain().run(setup.seeds, depth=300.0, method=0, delta_t=DT, record_t=RT, attrs=True,
                                segment_steps=7, capture_slots=2, compact=True, compact_chunks=4)
        _same_lines(_host(got), want)


def test_recycled_fields_attr_lifetimes(gpu, engine_lib, oracle_lib, small_case):
    """A recycling make_field (two fields resident, snapshot p's buffers re-derived as p + 2): the attribute
    tensors follow the fields -- snapshot p's are dropped before snapshot p + 2's are made."""
    import torch
    from mops_amd.chain import PathlineChain, snapshot_attr_factory
    from mops_amd.engine import DeviceField
    s = _Setup(oracle_lib, small_case[0], n_snap=5)
    keys = ("layerThickness", "bottomDepth", "zonalVelocity", "meridionalVelocity", "vertVelocityTop")

    def raw(i):
        return {k: torch.as_tensor(getattr(s.snaps[i], k), device="cuda") for k in keys}

    class Recycle:
        def __call__(self, i, stream):
            d = raw(i)
            torch.cuda.current_stream().synchronize()
            return DeviceField.from_device_snapshot(s.dm, d, timestep=i, stream=stream)

        def refill(self, field, i, stream):
            d = raw(i)
            stream.wait_stream(torch.cuda.current_stream())
            return field.rebuild_from_device(d, timestep=i, stream=stream.cuda_stream)

    inner = snapshot_attr_factory(s.dm, lambda i: s.snaps[i])
    refs, alive_at_call = {}, {}

    def make_attrs(i, stream):
        alive_at_call[i] = sorted(j for j, ws in refs.items() if any(w() is not None for w in ws))
        t = inner(i, stream)
        refs[i] = [weakref.ref(v) for v in t.values()]
        return t

    kw = dict(depth=250.0, method=1, delta_t=DT, record_t=RT, attrs=True)
    got = _host(PathlineChain(s.dm, Recycle(), 5, gap_seconds=GAP, prefetch=False, make_attrs=make_attrs).run(s.seeds, **kw))
    assert alive_at_call == {0: [], 1: [0], 2: [1], 3: [2], 4: [3]}
    want = _host(s.chain().run(s.seeds, **kw))  # fresh fields, prefetch on
    _same_lines(got, want)
    assert got["attributes"]["salinity"].shape[1] == 1 + 4 * 6


def test_refusals_and_defaults(setup):
    from mops_amd.chain import PathlineChain, snapshot_field_factory
    bare = PathlineChain(setup.dm, snapshot_field_factory(setup.dm, lambda i: setup.snaps[i]), 3, gap_seconds=GAP)
    with pytest.raises(ValueError, match="make_attrs"):
        bare.run(setup.seeds, depth=300.0, method=1, delta_t=DT, record_t=RT, attrs=True)

    class Collector:
        reads_records = True

        def __call__(self, p, last, ps):
            pass
    with pytest.raises(ValueError, match="reads_records"):
        setup.chain().run(setup.seeds, depth=300.0, method=1, delta_t=DT, record_t=RT, attrs=True, on_pair=Collector())
    res = setup.chain().run(setup.seeds, depth=300.0, method=1, delta_t=DT, record_t=RT)  # make_attrs given, attrs off
    assert "attributes" not in res
    assert np.array_equal(res["temperature"].cpu().numpy(), res["velocity"][:, :, 0].cpu().numpy())


def test_mopspathline_sample_attributes_and_binary_export(engine_lib, oracle_lib, gpu, tmp_path):
    """MOPSPathline.run(sample_attributes=True) on monthly files the test writes: the chain's values, by name;
    the default call is unchanged; export_pathlines_to_binary(include_scalars=True) round-trips the scalars."""
    scipy_io = pytest.importorskip("scipy.io")
    from mops_amd import synth
    from mops_amd.chain import PathlineChain, snapshot_attr_factory, snapshot_field_factory
    from mops_amd.engine import DeviceMesh
    from mops_amd.pathline import MOPSPathline
    rd = _module("test_mpas_reader")
    mesh = synth.make_mesh(8, n_levels=6)
    snaps = [synth.make_snapshot(mesh, timestep=t, phase=0.3 * t) for t in range(3)]
    rd._write_mesh(str(tmp_path / "mesh.nc"), mesh, 2)
    dates = ["0001-01-01", "0001-02-01", "0001-03-01"]
    C_, L_ = mesh.nCells, mesh.nVertLevels
    for d, s in zip(dates, snaps):
        f = scipy_io.netcdf_file(str(tmp_path / f"hist.am.timeSeriesStatsMonthly.{d}.nc"), "w", version=2)
        f.createDimension("Time", None); f.createDimension("nCells", C_)
        f.createDimension("nVertLevels", L_); f.createDimension("nVertLevelsP1", L_ + 1); f.createDimension("StrLen", 64)
        f.createVariable("xtime_startMonthly", "c", ("Time", "StrLen"))[0] = np.frombuffer(
            (d + "_00:00:00").ljust(64, "\0").encode(), dtype="S1")
        for var, arr, dim in (("timeMonthly_avg_layerThickness", s.layerThickness, "nVertLevels"),
                              ("timeMonthly_avg_velocityZonal", s.zonalVelocity, "nVertLevels"),
                              ("timeMonthly_avg_velocityMeridional", s.meridionalVelocity, "nVertLevels"),
                              ("timeMonthly_avg_vertVelocityTop", s.vertVelocityTop, "nVertLevelsP1"),
                              ("timeMonthly_avg_activeTracers_temperature", s.attributes["temperature"], "nVertLevels"),
                              ("timeMonthly_avg_activeTracers_salinity", s.attributes["salinity"], "nVertLevels")):
            f.createVariable(var, "d", ("Time", "nCells", dim))[0] = np.asarray(arr).reshape(C_, -1)
        f.createVariable("bottomDepth", "d", ("nCells",))[:] = s.bottomDepth
        f.close()
    yaml = rd.YAML.replace("        - name: bottomDepth",
                           "        - name: temperature\n"
                           "          possible_names: [temperature, timeMonthly_avg_activeTracers_temperature]\n"
                           "          optional: true\n"
                           "        - name: bottomDepth")
    assert "temperature" in yaml
    y = tmp_path / "mpas.yaml"
    y.write_text(yaml.format(prefix=str(tmp_path)))
    seeds = synth.uniform_band_seeds(90, seed=4)

    def run(**kw):
        p = MOPSPathline(str(y)).init("gpu")
        p.set_time(1, 1, 1, 3)
        p.set_seed(depth=150.0, points=seeds)
        return p.run(method="euler", delta_minutes=180, record_every_minutes=1440, **kw)
    lines, plain = run(sample_attributes=True), run()
    dm = DeviceMesh.from_mesh(mesh)
    chain = PathlineChain(dm, snapshot_field_factory(dm, lambda i: snaps[i]), 3, gap_seconds=[31 * 86400, 28 * 86400],
                          make_attrs=snapshot_attr_factory(dm, lambda i: snaps[i]))
    want = _host(chain.run(seeds, depth=150.0, method=1, delta_t=10800, record_t=86400, attrs=True))
    for k in ("points", "velocity", "temperature", "salinity", "lastPoint"):
        assert np.array_equal(np.stack([ln[k] for ln in lines]), want[k]), k
    assert np.stack([ln["temperature"] for ln in lines]).any()
    assert np.array_equal(want["temperature"], want["attributes"]["temperature"])
    # the default call: quirk Q9 as before, same points
    for ln, pl in zip(lines, plain):
        assert np.array_equal(pl["points"], ln["points"])
        assert np.array_equal(pl["temperature"], pl["velocity"][:, 0]) and np.array_equal(pl["salinity"], pl["velocity"][:, 1])
    # the binary export writes the named scalars (it goes by key)
    import json
    import struct
    from mops_amd import io
    stacked = {k: np.stack([ln[k] for ln in lines]) for k in ("points", "velocity", "temperature", "salinity")}
    out = tmp_path / "lines.bin"
    io.export_pathlines_to_binary(stacked, str(out), include_scalars=True)
    fields = json.loads((tmp_path / "lines.meta.json").read_text())["fields"]
    it, isal, nf = fields.index("temperature"), fields.index("salinity"), len(fields)
    b = out.read_bytes()
    assert struct.unpack_from("<i", b, 0)[0] == len(lines)
    off = 4
    for i in range(len(lines)):
        (m,) = struct.unpack_from("<i", b, off); off += 4
        rec = np.frombuffer(b, dtype="<f8", count=m * nf, offset=off).reshape(m, nf); off += m * nf * 8
        assert np.array_equal(rec[:, it], want["temperature"][i]) and np.array_equal(rec[:, isal], want["salinity"][i])
    assert off == len(b)
