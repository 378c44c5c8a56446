"""GPU: particle density maps (mops_density_accumulate / mops_density_image through engine.DensityMap,
PathlineChain.run(density=...), pyMOPS.MOPS_RunDensity and MOPS::MOPS_RunDensity) against the numpy restatement
(tests/density_reference.py, pinned by tests/test_density_cpu.py).

Every parity assertion is bytes-equal on the integer accumulator (and on the images).  The device's asin / atan2
may differ from libm's by ulps, so each comparison first asserts on the CPU that no valid point of its input lies
within 1e-6 of a pixel of a pixel edge (``_guard``) and then demands equality with nothing excluded."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import density_reference as D
import image_reference as IR
import pathline_attr_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = R.DURATION // R.RECORD_T  # 12
N_STEPS = R.DURATION // R.DELTA_T  # 36
NAMES = ["salinity", "temperature"]  # std::map order: the attribute slab's rows
GLOBAL = ((-90.0, 90.0), (-180.0, 180.0))
WINDOWS = {
    "64x32": (64, 32) + GLOBAL,
    "720x360": (720, 360) + GLOBAL,
    "256x128-dateline": (256, 128, (-40.0, 40.0), (150.0, 210.0)),
    "720x360-0to360": (720, 360, (-90.0, 90.0), (0.0, 360.0)),
}
KINDS = ((None, D.COUNT), ("speed", D.SPEED), ("temperature", D.VALUES))
R_EARTH = 6371000.0


def _guard(points, win):
    d = D.edge_distance(points, *win)
    assert d > D.EDGE_GUARD, f"a test point lies {d:.3g} of a pixel from a pixel edge"


def _host(t):
    return t.cpu().numpy()


class _Case:
    """small_case on the device, and per method one ParticleSet advanced over the whole pair with both attributes
    sampled, with host copies of its slabs (computed once, never modified)."""

    def __init__(self, mesh, s0, s1):
        from mops_amd.engine import DeviceField, DeviceMesh, cell_to_vertex_attr
        self.mesh = mesh
        self.dm = DeviceMesh.from_mesh(mesh)
        self.f0, self.f1 = DeviceField.from_snapshot(self.dm, s0), DeviceField.from_snapshot(self.dm, s1)
        self.front = [cell_to_vertex_attr(self.dm, s0.attributes[k]) for k in NAMES]
        self.back = [cell_to_vertex_attr(self.dm, s1.attributes[k]) for k in NAMES]
        self.seeds, self.depths = R.shared_seeds()
        self._run = {}

    def run(self, euler):
        if euler not in self._run:
            import torch
            from mops_amd.engine import ParticleSet, TrajectoryConfig
            cfg = TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=0.0,
                                   method=1 if euler else 0)
            ps = ParticleSet(self.dm, self.seeds, self.depths, cfg, n_attr=2)
            ps.advance(self.f0, self.f1, 0, N_STEPS, attrs=(self.front, self.back))
            torch.cuda.synchronize()
            self._run[euler] = types.SimpleNamespace(
                ps=ps, rec=_host(ps.records), attr=_host(ps.attr_records), seeds=_host(ps.seeds),
                death=_host(ps.death))
        return self._run[euler]


@pytest.fixture(scope="module")
def case(gpu, engine_lib, small_case):
    return _Case(*small_case)


def _map(win, value=None):
    from mops_amd.engine import DensityMap
    return DensityMap(win[0], win[1], win[2], win[3], value=value)


def _want(run, win, kind, k_range=None, seeds=False, n=None):
    n = R.N_SEEDS if n is None else n
    return D.records_accumulate(D.new_accum(win[0], win[1]), run.rec, n, *win, kind=kind, attr=run.attr[:, 1],
                                k_range=k_range, seeds=run.seeds if seeds else None)


# ---- 1. the accumulator against the restatement ------------------------------------------------------------
@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_accumulator_matches_restatement(case, euler, window):
    win = WINDOWS[window]
    run = case.run(euler)
    pts = run.rec[:, 0:3, :].transpose(0, 2, 1).reshape(-1, 3)
    _guard(pts, win)
    _guard(run.seeds, win)
    nonzero = int((np.abs(pts).sum(axis=1) != 0).sum())
    dead = int((run.death >= 0).sum())
    assert dead > 0 and nonzero < K * R.N_SEEDS  # some particles died: their later slots are zeros
    for value, kind in KINDS:
        m = _map(win, value)
        m.accumulate(run.ps)
        got = _host(m.accum)
        want = _want(run, win, kind)
        print(f"{window} {'euler' if euler else 'rk4'} {value}: dead {dead}, nonzero points {nonzero}, inside "
              f"{int(want[:, :, 0].sum())}, pixels {int((want[:, :, 0] > 0).sum())}")
        assert got.dtype == np.int64 and got.tobytes() == want.tobytes(), value
        if win[2:] == GLOBAL or window == "720x360-0to360":
            # a global window holds every valid point, and the dead particles' zero slots add nothing
            assert int(got[:, :, 0].sum()) == nonzero
        if kind == D.COUNT:
            assert not got[:, :, 1].any()
            m.reset()
            m.accumulate(run.ps, seeds=True)
            assert _host(m.accum).tobytes() == _want(run, win, kind, seeds=True).tobytes()
        else:
            assert got[:, :, 1].any()
            before = got.copy()
            m.accumulate(run.ps, seeds=True, record_range=(0, 0))  # an empty range adds nothing, seeds or not
            assert _host(m.accum).tobytes() == before.tobytes()


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_0_to_360_is_the_global_window_rolled(case, euler):
    run = case.run(euler)
    for value, _ in KINDS:
        a, b = _map(WINDOWS["720x360"], value), _map(WINDOWS["720x360-0to360"], value)
        a.accumulate(run.ps)
        b.accumulate(run.ps)
        assert np.array_equal(_host(b.accum), np.roll(_host(a.accum), 360, axis=1)), value


# ---- 2. shapes where the kernel can go wrong --------------------------------------------------------------
def _slab_set(run, n, pad=7, fill=-7.0):
    """The first n particles of a run as a set-like view with record_stride n + pad; padding columns = fill."""
    import torch
    stride = n + pad
    rec = np.full((K, 6, stride), fill)
    rec[:, :, :n] = run.rec[:, :, :n]
    att = np.full((K, 2, stride), fill)
    att[:, :, :n] = run.attr[:, :, :n]
    return types.SimpleNamespace(n=n, K=K, rec_stride=stride, n_attr=2,
                                 records=torch.as_tensor(rec, device="cuda"),
                                 attr_records=torch.as_tensor(att, device="cuda"),
                                 seeds=torch.as_tensor(np.ascontiguousarray(run.seeds[:max(n, 1)]), device="cuda"))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 96])
def test_particle_counts_padding_ranges_and_seeds(case, n):
    run = case.run(True)
    win = WINDOWS["64x32"]
    _guard(run.rec[:, 0:3, :].transpose(0, 2, 1).reshape(-1, 3), win)
    _guard(run.seeds, win)
    view = _slab_set(run, n)  # (a padding column of -7 would land in a pixel if it were read)
    for value, kind in KINDS:
        for k_range in ((0, K), (0, 0), (3, 4), (5, 12)):
            for seeds in (False, True):
                m = _map(win, value)
                m.accumulate(view, record_range=k_range, seeds=seeds)
                want = _want(run, win, kind, k_range=k_range, seeds=seeds, n=n)
                assert _host(m.accum).tobytes() == want.tobytes(), (value, k_range, seeds)
                if n == 0 or k_range == (0, 0):
                    assert not _host(m.accum).any()


def test_every_lane_on_the_same_pixels(case):
    """4096 copies of one live particle: every lane of every wave adds to the same pixels."""
    import torch
    run = case.run(True)
    live = int(np.flatnonzero(run.death < 0)[0])
    copies = 4096
    rec = np.repeat(run.rec[:, :, live:live + 1], copies, axis=2)
    att = np.repeat(run.attr[:, :, live:live + 1], copies, axis=2)
    one = types.SimpleNamespace(rec=rec, attr=att, seeds=np.repeat(run.seeds[live:live + 1], copies, axis=0))
    view = types.SimpleNamespace(n=copies, K=K, rec_stride=copies, n_attr=2, records=torch.as_tensor(rec, device="cuda"),
                                 attr_records=torch.as_tensor(att, device="cuda"),
                                 seeds=torch.as_tensor(one.seeds, device="cuda"))
    for window in ("64x32", "720x360"):
        win = WINDOWS[window]
        for value, kind in KINDS:
            m = _map(win, value)
            m.accumulate(view)
            got = _host(m.accum)
            assert int(got[:, :, 0].sum()) == copies * K
            assert (got[:, :, 0] % copies == 0).all()
            assert got.tobytes() == _want(one, win, kind, n=copies).tobytes()


def _points_set(points, values=None, velocity=None):
    """One record slot holding the given points (and velocities); attribute row 1 = values."""
    import torch
    p = np.asarray(points, dtype=np.float64)
    n = p.shape[0]
    rec = np.zeros((1, 6, n))
    rec[0, 0:3] = p.T
    if velocity is not None:
        rec[0, 3:6] = np.asarray(velocity, dtype=np.float64).T
    att = np.zeros((1, 2, n))
    if values is not None:
        att[0, 1] = values
    view = types.SimpleNamespace(n=n, K=1, rec_stride=n, n_attr=2, records=torch.as_tensor(rec, device="cuda"),
                                 attr_records=torch.as_tensor(att, device="cuda"),
                                 seeds=torch.as_tensor(np.ascontiguousarray(p), device="cuda"))
    return view, types.SimpleNamespace(rec=rec, attr=att, seeds=p)


def test_skipped_points_values_and_the_pole():
    nan, inf = float("nan"), float("inf")
    good = [R_EARTH * 0.6, R_EARTH * 0.5, R_EARTH * 0.3]
    pts = [good, [nan, 1.0, 1.0], [1.0, inf, 1.0], [1.0, 1.0, -inf], [0.0, 0.0, 0.0], [0.0, 0.0, R_EARTH], good, good,
           good, good]
    vals = [1.25, 1.0, 1.0, 1.0, 1.0, -3.5, nan, 2.0 ** 38, -inf, -(2.0 ** 38 - 1.0)]
    vel = [[v, 0.0, 0.0] for v in vals]
    win = WINDOWS["64x32"]
    _guard([good], win)
    view, host = _points_set(pts, vals, vel)
    for value, kind in KINDS:
        m = _map(win, value)
        m.accumulate(view)
        got = _host(m.accum)
        want = D.records_accumulate(D.new_accum(win[0], win[1]), host.rec, len(pts), *win, kind=kind, attr=host.attr[:, 1])
        assert got.tobytes() == want.tobytes(), value
        # the pole (0, 0, r) lands in row 0 (column: lon = atan2(0, 0) = 0)
        assert got[0, 32, 0] == 1 and got[0].sum(axis=0)[0] == 1
    cnt = _map(win)
    cnt.accumulate(view)
    assert int(_host(cnt.accum)[:, :, 0].sum()) == 6      # NaN, +-Inf and (0, 0, 0) positions are skipped
    val = _map(win, "temperature")
    val.accumulate(view)
    v = _host(val.accum)
    assert int(v[:, :, 0].sum()) == 3                     # and so are a non-finite value and 2^38
    assert int(v[0, 32, 1]) == int(-3.5 * 2 ** 24)
    spd = _map(win, "speed")
    spd.accumulate(view)
    assert int(_host(spd.accum)[:, :, 0].sum()) == 3 and int(_host(spd.accum)[0, 32, 1]) == int(3.5 * 2 ** 24)


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_twice_permuted_and_split(case, euler):
    import torch
    run = case.run(euler)
    win = WINDOWS["720x360"]
    for value, kind in KINDS:
        once = _map(win, value)
        once.accumulate(run.ps)
        base = _host(once.accum)
        once.accumulate(run.ps)
        assert np.array_equal(_host(once.accum), 2 * base), value  # accumulating twice doubles every entry
        split = _map(win, value)
        split.accumulate(run.ps, record_range=(0, 5))
        split.accumulate(run.ps, record_range=(5, 12))
        assert _host(split.accum).tobytes() == base.tobytes(), value
        perm = np.random.default_rng(17).permutation(R.N_SEEDS)
        view = types.SimpleNamespace(n=R.N_SEEDS, K=K, rec_stride=R.N_SEEDS, n_attr=2,
                                     records=torch.as_tensor(np.ascontiguousarray(run.rec[:, :, perm]), device="cuda"),
                                     attr_records=torch.as_tensor(np.ascontiguousarray(run.attr[:, :, perm]),
                                                                  device="cuda"),
                                     seeds=torch.as_tensor(np.ascontiguousarray(run.seeds[perm]), device="cuda"))
        shuffled = _map(win, value)
        shuffled.accumulate(view)
        assert _host(shuffled.accum).tobytes() == base.tobytes(), value
    once.reset()
    assert not _host(once.accum).any()


# ---- 3. the lines layout ---------------------------------------------------------------------------------
@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_lines_layout(case, euler):
    run = case.run(euler)
    lines = run.ps.finalize(pathline=True)
    points = lines["points"]
    assert tuple(points.shape) == (R.N_SEEDS, K + 1, 3)
    for window in ("64x32", "256x128-dateline"):
        win = WINDOWS[window]
        _guard(_host(points).reshape(-1, 3), win)
        slab, slab_seeds = _map(win), _map(win)
        slab.accumulate(run.ps)
        slab_seeds.accumulate(run.ps, seeds=True)
        a = _map(win)
        a.accumulate_lines(points[:, 1:])
        assert _host(a.accum).tobytes() == _host(slab.accum).tobytes()
        b = _map(win)
        b.accumulate_lines(_host(points))  # a host array, whole: the seeds too
        assert _host(b.accum).tobytes() == _host(slab_seeds.accum).tobytes()
        # values beside the points: [n, P] for an attribute map, velocities [n, P, 3] for a speed map
        t = _map(win, "temperature")
        vals = np.ascontiguousarray(run.ps.original(run.ps.attr_records[:, 1, :].T.contiguous()).cpu().numpy())
        t.accumulate_lines(points[:, 1:], vals)
        slab_t = _map(win, "temperature")
        slab_t.accumulate(run.ps)
        assert _host(t.accum).tobytes() == _host(slab_t.accum).tobytes()
        s = _map(win, "speed")
        vel = run.ps.original(run.ps.records[:, 3:6, :].permute(2, 0, 1).contiguous())
        s.accumulate_lines(points[:, 1:], vel)
        slab_s = _map(win, "speed")
        slab_s.accumulate(run.ps)
        assert _host(s.accum).tobytes() == _host(slab_s.accum).tobytes()
    with pytest.raises(ValueError):
        _map(win, "speed").accumulate_lines(points)        # a speed map needs velocities
    with pytest.raises(ValueError):
        _map(win).accumulate_lines(points[:, :, :2])


# ---- 4. the image -----------------------------------------------------------------------------------------
def test_image_and_colour(case):
    from mops_amd.engine import colormap_rgba
    run = case.run(True)
    win = WINDOWS["64x32"]
    m = _map(win, "temperature")
    m.accumulate(run.ps)
    acc = _host(m.accum)
    for nan_empty in (True, False):
        got = _host(m.image(nan_empty=nan_empty))
        want = D.image(acc, nan_empty=nan_empty)
        assert got.shape == (32, 64, 4) and got.tobytes() == want.tobytes(), nan_empty
    img = m.image()
    rgba = _host(colormap_rgba(img, channels=(0, 1, 2)))
    empty = acc[:, :, 0] == 0
    assert empty.any() and not empty.all()
    assert not rgba[:, empty].any()                       # empty pixels come out {0, 0, 0, 0}
    assert (rgba[:, ~empty][..., 3] == 255).all()
    for c in range(3):
        assert np.array_equal(rgba[c], IR.save_to_png_rgba(_host(img)[:, :, c])[0])


# ---- 5. the chain -----------------------------------------------------------------------------------------
EARTH_RADIUS_M = 6_371_000.0


class _Chain:
    """The 3-snapshot, 2-pair chain of tests/test_attr_chain_gpu.py on the shared 96 seeds: 36 steps and 12
    records per pair, 13 + 12 points per line."""

    def __init__(self, O, mesh):
        from mops_amd import synth
        from mops_amd.engine import DeviceMesh
        self.O, self.mesh = O, mesh
        self.snaps = [synth.make_snapshot(mesh, timestep=t, phase=0.35 * t) for t in range(3)]
        self.derived = [O.preprocess(mesh, s) for s in self.snaps]
        self.dm = DeviceMesh.from_mesh(mesh)
        self.seeds, _ = R.shared_seeds()
        self._ref, self._plain = {}, {}

    def chain(self):
        from mops_amd.chain import PathlineChain, snapshot_attr_factory, snapshot_field_factory
        return PathlineChain(self.dm, snapshot_field_factory(self.dm, lambda i: self.snaps[i]), 3,
                             gap_seconds=R.DURATION, make_attrs=snapshot_attr_factory(self.dm, lambda i: self.snaps[i]))

    def kw(self, follow_last):
        return dict(depth=300.0, method=1, delta_t=R.DELTA_T, record_t=R.RECORD_T, follow_last=follow_last, attrs=True)

    def reference(self, follow_last, wins):
        """The restatement's accumulators of the reference chain's records (tests/pathline_attr_reference.py run
        pair by pair with the reference caller's seed rule): the count map with pair 0's seeds, the temperature
        map of the records alone.  Also every point, for the edge guard."""
        if follow_last not in self._ref:
            O, seeds = self.O, self.seeds
            depths = np.full(len(seeds), 300.0, dtype=np.float32)
            cnt = D.new_accum(*wins[0][:2])
            tmp = D.new_accum(*wins[1][:2])
            allpts, last = [seeds], None
            for p in range(2):
                s = seeds if (p == 0 or not follow_last) else last
                r = R.run(self.mesh, self.derived[p], self.derived[p + 1], s, depths, O.knn(self.mesh, s), R.DELTA_T,
                          R.DURATION, R.RECORD_T, euler=True)
                assert r["names"] == NAMES
                rec = np.concatenate([r["rec_pos"], r["rec_vel"]], axis=2).transpose(1, 2, 0)  # [K, 6, n]
                att = r["rec_attr"][:, :, 1].T                                               # [K, n] temperature
                D.records_accumulate(cnt, rec, len(seeds), *wins[0], kind=D.COUNT, seeds=s if p == 0 else None)
                D.records_accumulate(tmp, rec, len(seeds), *wins[1], kind=D.VALUES, attr=att)
                allpts.append(r["rec_pos"].reshape(-1, 3))
                last = O.finalize_lines(s, r["rec_pos"], r["rec_vel"], K, with_attrs=False)["lastPoint"].copy()
            self._ref[follow_last] = (cnt, tmp, np.concatenate(allpts))
        return self._ref[follow_last]

    def plain(self, follow_last):
        if follow_last not in self._plain:
            self._plain[follow_last] = _chain_host(self.chain().run(self.seeds, **self.kw(follow_last)))
        return self._plain[follow_last]


def _chain_host(res):
    out = {k: v.cpu().numpy() for k, v in res.items() if k != "attributes" and hasattr(v, "cpu")}
    for k, v in res.get("attributes", {}).items():
        out["attributes." + k] = v.cpu().numpy()
    return out


@pytest.fixture(scope="module")
def chain_setup(gpu, engine_lib, oracle_lib, small_case):
    return _Chain(oracle_lib, small_case[0])


CHAIN_WINS = (WINDOWS["64x32"], WINDOWS["720x360"])
CHAIN_MODES = {
    "default": dict(),
    "nofollow": dict(),
    "compact": dict(compact=True, compact_chunks=4),
    "defer_lines": dict(defer_lines=True),
    "on_lines": dict(keep_lines=False, on_lines=lambda p, lines, ids: None, lines_chunk=37),
    "no_lines": dict(keep_lines=False),
    "capture0": dict(capture_slots=0),
    "segments": dict(segment_steps=7, capture_slots=2),
}


@pytest.mark.parametrize("mode", list(CHAIN_MODES))
def test_chain_density(chain_setup, mode):
    s = chain_setup
    follow_last = mode != "nofollow"
    want_cnt, want_tmp, pts = s.reference(follow_last, CHAIN_WINS)
    for w in CHAIN_WINS:
        _guard(pts, w)
    maps = [_map(CHAIN_WINS[0]), _map(CHAIN_WINS[1], "temperature")]
    res = _chain_host(s.chain().run(s.seeds, density=maps, **s.kw(follow_last), **CHAIN_MODES[mode]))
    cnt, tmp = _host(maps[0].accum), _host(maps[1].accum)
    print(f"{mode}: count {int(cnt[:, :, 0].sum())} of {25 * R.N_SEEDS} points, temperature samples "
          f"{int(tmp[:, :, 0].sum())}")
    assert cnt.tobytes() == want_cnt.tobytes()
    assert tmp.tobytes() == want_tmp.tobytes() and tmp[:, :, 1].any()
    # the run's other outputs are those of a run without density
    plain = s.plain(follow_last)
    assert set(res) <= set(plain) and {"lastPoint", "death_step", "attempted"} <= set(res)
    for k in res:
        assert res[k].tobytes() == plain[k].tobytes(), k
    if mode == "default":  # one map, not in a list
        one = _map(CHAIN_WINS[0])
        s.chain().run(s.seeds, density=one, **s.kw(True))
        assert _host(one.accum).tobytes() == want_cnt.tobytes()


def test_chain_density_refusals(chain_setup):
    s = chain_setup
    launches = []

    class Spy:
        def __init__(self, f):
            self.f = f

        def __call__(self, i, stream):
            launches.append(i)
            return self.f(i, stream)
    from mops_amd.chain import PathlineChain, snapshot_attr_factory, snapshot_field_factory
    chain = PathlineChain(s.dm, Spy(snapshot_field_factory(s.dm, lambda i: s.snaps[i])), 3, gap_seconds=R.DURATION,
                          make_attrs=snapshot_attr_factory(s.dm, lambda i: s.snaps[i]))
    tmap = _map(CHAIN_WINS[0], "temperature")
    kw = dict(depth=300.0, method=1, delta_t=R.DELTA_T, record_t=R.RECORD_T)
    with pytest.raises(ValueError, match="attrs=True"):
        chain.run(s.seeds, density=[_map(CHAIN_WINS[0]), tmap], **kw)
    assert launches == [] and not _host(tmap.accum).any()  # refused before a field was built or a kernel launched
    with pytest.raises(ValueError, match="samples no attribute"):
        chain.run(s.seeds, density=_map(CHAIN_WINS[0], "oxygen"), attrs=True, **kw)
    with pytest.raises(ValueError, match="DensityMap"):
        chain.run(s.seeds, density="count", **kw)
    # a count or speed map needs no attributes
    spd = _map(CHAIN_WINS[0], "speed")
    chain.run(s.seeds, density=spd, **kw)
    assert _host(spd.accum)[:, :, 1].any()


# ---- 6. pyMOPS and C++ ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pathlines(gpu, engine_lib, small_case):
    """A 96-seed pathline result with sampled attributes, as MOPS_RunPathLine's list[dict]."""
    from mops_amd import engine
    mesh, s0, s1 = small_case
    seeds, depths = R.shared_seeds()
    dm = engine.DeviceMesh.from_mesh(mesh)
    f0, f1 = engine.DeviceField.from_snapshot(dm, s0), engine.DeviceField.from_snapshot(dm, s1)
    attrs = {k: (engine.cell_to_vertex_attr(dm, s0.attributes[k]), engine.cell_to_vertex_attr(dm, s1.attributes[k]))
             for k in NAMES}
    cfg = engine.TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=0.0, method=1)
    got = engine.run_trajectories(dm, f0, f1, cfg, seeds, depths=depths, attrs=attrs)
    return [dict(lineID=i, points=got["points"][i], velocity=got["velocity"][i], temperature=got["temperature"][i],
                 salinity=got["salinity"][i], lastPoint=got["lastPoint"][i]) for i in range(len(seeds))]


def _lines_want(lines, win, key=None):
    pts = np.concatenate([ln["points"] for ln in lines])
    _guard(pts, win)
    val = None
    if key == "velocity":
        val = D.speed(np.concatenate([ln["velocity"] for ln in lines]))
    elif key is not None:
        val = np.concatenate([ln[key] for ln in lines])
    return D.image(D.accumulate(D.new_accum(win[0], win[1]), pts, *win, values=val))


def test_pymops_run_density(pathlines, tmp_path):
    from mops_amd import pyMOPS as M
    win = WINDOWS["256x128-dateline"]
    cfg = M.VisualizationSettings()
    cfg.imageSize, cfg.LatRange, cfg.LonRange = (win[0], win[1]), win[2], win[3]
    for value, key in ((None, None), ("temperature", "temperature"), ("salinity", "salinity"), ("speed", "velocity")):
        got = M.MOPS_RunDensity(pathlines, cfg, value)
        want = _lines_want(pathlines, win, key)
        assert got.shape == (128, 256, 4) and got.tobytes() == want.tobytes(), value
        assert np.nansum(got[:, :, 0]) > 100
    # lines of unequal length
    ragged = [dict(ln, points=ln["points"][:5 + i % 7], temperature=ln["temperature"][:5 + i % 7])
              for i, ln in enumerate(pathlines)]
    assert M.MOPS_RunDensity(ragged, cfg, "temperature").tobytes() == _lines_want(ragged, win, "temperature").tobytes()
    # usable with SaveToPNG unchanged
    count = M.MOPS_RunDensity(pathlines, cfg)
    png = str(tmp_path / "count.png")
    assert M.SaveToPNG(count, png, 0)
    assert np.array_equal(IR.decode_png(png), IR.save_to_png_rgba(count[:, :, 0])[0])
    # bad input: Error() and an empty image
    assert not M.MOPS_RunDensity(pathlines, cfg, "oxygen").any()
    assert M.MOPS_RunDensity(pathlines, None).size == 0
    bad = M.VisualizationSettings()
    bad.imageSize, bad.LatRange, bad.LonRange = (8, 4), (10.0, 10.0), (0.0, 90.0)
    assert not M.MOPS_RunDensity(pathlines, bad).any()


def test_cpp_run_density(pathlines, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "cpp", "density_api.cpp")
    exe = str(tmp_path / "density_api")
    libdir = os.path.join(ROOT, "mops_amd", "lib")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src,
                    "-L" + libdir, "-lmops_traj", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe],
                   check=True)
    win = WINDOWS["256x128-dateline"]
    d = str(tmp_path)
    pts = np.stack([ln["points"] for ln in pathlines])
    tmp = np.stack([ln["temperature"] for ln in pathlines])
    with open(os.path.join(d, "dims.txt"), "w") as f:
        f.write(f"{pts.shape[0]} {pts.shape[1]} {win[0]} {win[1]} {win[2][0]} {win[2][1]} {win[3][0]} {win[3][1]}\n")
    pts.astype(np.float64).tofile(os.path.join(d, "points"))
    tmp.astype(np.float64).tofile(os.path.join(d, "temperature"))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert r.stderr.count("[Error]") == 4
    for name, key in (("count", None), ("temperature", "temperature")):
        got = np.fromfile(os.path.join(d, name + ".f64")).reshape(win[1], win[0], 4)
        assert got.tobytes() == _lines_want(pathlines, win, key).tobytes(), name
    count = np.fromfile(os.path.join(d, "count.f64")).reshape(win[1], win[0], 4)
    rgba = IR.decode_png(os.path.join(d, "count.png"))
    assert np.array_equal(rgba, IR.save_to_png_rgba(count[:, :, 0])[0])
    assert not rgba[np.isnan(count[:, :, 0])].any() and (rgba[~np.isnan(count[:, :, 0])][:, 3] == 255).all()
