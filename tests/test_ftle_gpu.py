"""GPU: flow-map lattices and FTLE images (mops_flowmap_lattice / mops_ftle_image through engine.FlowMapLattice,
chain.EverDead) against the numpy restatement (tests/ftle_reference.py, pinned by tests/test_ftle_cpu.py).

Channels 1 and 2 (lambda_max, lambda_min) and the NaN pattern are bytes-equal to the restatement with nothing
excluded: the kernel uses + - * / sqrt only up to there, without contraction.  Channel 0 is the device's log: it is
compared with numpy.log of the device's own channel 1, divided by 2 * horizon.  The ROCm math documentation that
states the device log's ulp bound is not part of this installation, so -- as DESIGN.md section 3.17 records -- the
allowance is twice the largest difference observed over this file's cases on an MI355X (2 ulp, which already
contains glibc's log error and the division's rounding): ``LOG_ULPS`` = 4.  Every case prints its own figure."""
import numpy as np
import pytest

import ftle_reference as F
import pathline_attr_reference as R
import rk4_relocate_reference as RR

pytestmark = pytest.mark.gpu

LOG_ULPS = 4  # twice the largest observed difference (see the module docstring)
RELOCATE = 2  # MOPS_RK4_RELOCATE
N_STEPS = R.DURATION // R.DELTA_T  # 36


def _host(t):
    return t.cpu().numpy()


def _lattice(width, height, lat_range, lon_range):
    from mops_amd.engine import FlowMapLattice
    return FlowMapLattice(width, height, lat_range, lon_range)


def _check(lat, last, death, horizon, what=""):
    """The device image of ``lat`` for (last, death) against the restatement; returns the device image."""
    seeds = _host(lat.seeds)
    got = _host(lat.ftle(last, death, horizon))
    want = F.ftle_image(lat.width, lat.height, seeds, last, death, horizon, lat.wrap_lon)
    assert got.shape == (lat.height, lat.width, 4) and got.dtype == np.float64
    assert np.all(got[:, :, 3] == 1.0), what
    for ch in (1, 2):
        assert got[:, :, ch].tobytes() == want[:, :, ch].tobytes(), (what, ch)
    assert np.array_equal(np.isnan(got[:, :, 0]), np.isnan(want[:, :, 1])), what
    with np.errstate(all="ignore"):
        mine = np.log(got[:, :, 1]) / (2.0 * horizon)
    inf = np.isinf(mine)
    assert np.array_equal(got[:, :, 0][inf], mine[inf]), what
    d = F.ulp_distance(got[:, :, 0], mine)
    print(f"{what}: {int((~np.isnan(got[:, :, 1])).sum())} of {lat.n} pixels valid, channel 0 within {d} ulp of "
          f"numpy.log(channel 1) / (2 * horizon)")
    assert d <= LOG_ULPS, what
    return got


def _deformed(lat, k=0.4, swirl=0.2):
    """A smooth flow map on the lattice's angles: a shear plus a latitude-dependent squeeze; another radius."""
    la, lo = F.lattice_angles(lat.width, lat.height, lat.lat_range, lat.lon_range)
    la2 = la[:, None] + swirl * np.sin(2.0 * lo[None, :]) * np.cos(la[:, None])
    lo2 = lo[None, :] + k * la[:, None]
    return F.sphere(la2, lo2, F.RADIUS - 500.0).reshape(-1, 3)


# ---- 1. the lattice -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,lat,lon", [(1, 1, (-10.0, 10.0), (0.0, 40.0)), (5, 7, (-33.0, 71.5), (100.0, 260.0)),
                                         (257, 3, (-90.0, 90.0), (-180.0, 180.0)), (3, 257, (-80.0, 80.0), (0.0, 360.0))])
def test_lattice_bytes(gpu, engine_lib, W, H, lat, lon):
    la = _lattice(W, H, lat, lon)
    assert tuple(la.seeds.shape) == (W * H, 3) and la.seeds.is_cuda
    assert _host(la.seeds).tobytes() == F.lattice(W, H, lat, lon).tobytes()
    assert la.wrap_lon == (lon[1] - lon[0] == 360.0)


def test_lattice_is_the_fixed_depth_remapping_lattice(gpu, engine_lib, small_case):
    """The seeds are the positions remap_fixed_depth locates: its cell map is the cell map of the seeds."""
    import torch
    from mops_amd.engine import DeviceField, DeviceMesh, remap_fixed_depth
    mesh, s0, _ = small_case
    dm = DeviceMesh.from_mesh(mesh)
    df = DeviceField.from_snapshot(dm, s0)
    W, H, lat, lon = 24, 16, (-80.0, 80.0), (-180.0, 180.0)
    la = _lattice(W, H, lat, lon)
    _, cells = remap_fixed_depth(dm, df, W, H, lat, lon, 100.0, return_cells=True)
    mine = torch.empty((W * H,), dtype=torch.int32, device=la.seeds.device)
    dm.locate(la.seeds.data_ptr(), mine.data_ptr(), W * H, stream=torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(_host(mine).reshape(H, W), _host(cells))


# ---- 2. shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (5, 1), (1, 5)])
def test_degenerate_shapes_are_entirely_invalid(gpu, engine_lib, W, H):
    la = _lattice(W, H, (-10.0, 10.0), (0.0, 40.0))
    got = _check(la, _deformed(la), None, 1.0, f"{W}x{H}")
    assert np.isnan(got[:, :, :3]).all()


@pytest.mark.parametrize("W,H", [(2, 2), (3, 3), (257, 3), (3, 257)])
def test_shapes(gpu, engine_lib, W, H):
    la = _lattice(W, H, (-60.0, 66.0), (-45.0, 75.0))
    last = _deformed(la)
    got = _check(la, last, None, 3.0, f"{W}x{H}")
    assert not np.isnan(got[:, :, 1]).any()  # every pixel has a neighbour in both directions
    death = np.full(W * H, -1, dtype=np.int32)
    death[::5] = 4
    got = _check(la, last, death, 3.0, f"{W}x{H} with deaths")
    assert np.isnan(got.reshape(-1, 4)[::5, 1]).all()
    seeds = _host(la.seeds)
    rot = np.stack([-seeds[:, 1], seeds[:, 0], seeds[:, 2]], axis=1)  # an exact rigid map: the identity's bytes
    assert _host(la.ftle(rot, None, 3.0)).tobytes() == _host(la.ftle(seeds, None, 3.0)).tobytes()


def test_one_sided_rule_on_the_hand_made_case(gpu, engine_lib):
    la = _lattice(**F.DEAD_5x7)
    death, about = F.dead_case_5x7()
    last = F.shear_last(**F.DEAD_5x7, k=0.3)
    got = _check(la, last, death, 2.5, "5x7 dead patterns")
    nan = np.isnan(got[:, :, 1])
    assert nan[about["dead_centre"]] and nan[about["dead_jm_jp"]]
    assert not nan[about["dead_jm"]] and not nan[about["dead_ip"]]
    # death == NULL: the same particles dead through zero, then non-finite, last points
    for fill in (0.0, np.nan, np.inf, -np.inf):
        z = last.copy()
        z[death >= 0] = fill
        assert _check(la, z, None, 2.5, f"5x7 last = {fill}").tobytes() == got.tobytes(), fill
    z = last.copy()
    z[death >= 0, 1] = np.nan  # one component only
    assert _check(la, z, None, 2.5, "5x7 one NaN component").tobytes() == got.tobytes()


@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
def test_wrap_and_the_pole_row(gpu, engine_lib, wrap):
    """W = 4 over [-180, 180] wraps (columns 0 and 3 are neighbours); the same lattice with the switch turned off
    does not.  Row 0 is the pole (lat 90): its seeds differ in their last bits only."""
    la = _lattice(4, 5, (-90.0, 90.0), (-180.0, 180.0))
    assert la.wrap_lon and not _lattice(4, 5, (-90.0, 90.0), (-180.0, 179.0)).wrap_lon
    la.wrap_lon = wrap
    last = _deformed(la, k=0.1, swirl=0.05)
    got = _check(la, last, None, 1.0, f"4x5 pole, wrap {wrap}")
    assert not np.isnan(got[1:, :, 1]).any()
    death = np.full(20, -1, dtype=np.int32)
    death[4 * 2 + 3] = 0  # (2, 3): with wrap the j-1 of (2, 0)
    dead = _check(la, last, death, 1.0, f"4x5 pole, wrap {wrap}, a dead last column")
    assert (dead[2, 0].tobytes() != got[2, 0].tobytes()) == wrap
    if wrap:  # W = 2 with wrap: j-1 and j+1 are the same column
        two = _lattice(2, 3, (-60.0, 60.0), (-180.0, 180.0))
        assert np.isnan(_check(two, _deformed(two), None, 1.0, "2x3 wrap")[:, :, 1]).all()


def test_input_checks(gpu, engine_lib):
    la = _lattice(4, 3, (-10.0, 10.0), (0.0, 40.0))
    last = _host(la.seeds)
    for h in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            la.ftle(last, None, h)
    with pytest.raises(ValueError):
        la.ftle(last[:-1], None, 1.0)
    with pytest.raises(ValueError):
        la.ftle(last, np.zeros(5, dtype=np.int32), 1.0)
    from mops_amd.engine import FlowMapLattice
    for w, h in ((0, 3), (3, 0), (65536, 32768)):
        with pytest.raises(ValueError):
            FlowMapLattice(w, h, (-10.0, 10.0), (0.0, 40.0))


# ---- 3. end to end --------------------------------------------------------------------------------------------
E2E = dict(W=24, H=16, lat=(-80.0, 80.0), lon=(-180.0, 180.0), depth=300.0)


class _Case:
    def __init__(self, O, mesh):
        from mops_amd import synth
        from mops_amd.engine import DeviceField, DeviceMesh
        self.O, self.mesh = O, mesh
        self.snaps = [synth.make_snapshot(mesh, timestep=t, phase=0.35 * t) for t in range(3)]
        self.derived = [O.preprocess(mesh, s) for s in self.snaps]
        self.dm = DeviceMesh.from_mesh(mesh)
        self.fields = [DeviceField.from_snapshot(self.dm, s) for s in self.snaps[:2]]
        self.lat = _lattice(E2E["W"], E2E["H"], E2E["lat"], E2E["lon"])
        self.seeds = _host(self.lat.seeds)
        self.cells = O.knn(mesh, self.seeds)


@pytest.fixture(scope="module")
def case(gpu, engine_lib, oracle_lib, small_case):
    return _Case(oracle_lib, small_case[0])


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("method", [1, RELOCATE], ids=["euler", "rk4_relocate"])
def test_end_to_end_against_the_oracle(case, method, backward):
    """A 24 x 16 lattice over the shared mesh, 36 steps: the oracle's own last points and deaths (Euler: the C
    oracle; MOPS_RK4_RELOCATE: the restatement of tests/rk4_relocate_reference.py, assembled by the oracle) through
    the FTLE restatement give the device image's channels 1 and 2 and its NaN pattern byte for byte."""
    from mops_amd.engine import ParticleSet, TrajectoryConfig
    O, n = case.O, case.lat.n
    assert case.seeds.tobytes() == F.lattice(E2E["W"], E2E["H"], E2E["lat"], E2E["lon"]).tobytes()
    if method == 1:
        ref = O.run(case.mesh, case.derived[0], case.derived[1], case.seeds, depth=E2E["depth"], delta_t=R.DELTA_T,
                    duration=R.DURATION, record_t=R.RECORD_T, euler=True, backward=backward, cells=case.cells)
        last, death = ref["lastPoint"], ref["death"]
    else:
        ref = RR.run_case(O, case.mesh, case.derived[0], case.derived[1], case.seeds,
                          np.full(n, E2E["depth"], dtype=np.float32), backward=backward, relocate=True, cells=case.cells)
        last, death = RR.lines(O, ref)["lastPoint"], ref["death"]
    horizon = R.DURATION / 86400.0
    want = F.ftle_image(E2E["W"], E2E["H"], case.seeds, last, death, horizon, True)
    valid = ~np.isnan(want[:, :, 1])
    assert (~valid).any() and int((death >= 0).sum()) > 0  # land
    assert 2 * int(valid.sum()) >= n
    cfg = TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=E2E["depth"],
                           direction=1 if backward else 0, method=method)
    ps = ParticleSet(case.dm, case.lat.seeds, E2E["depth"], cfg, cells=case.cells)
    ps.advance(case.fields[0], case.fields[1], 0, N_STEPS)
    got = _host(case.lat.ftle_from(ps, horizon))
    assert np.array_equal(_host(ps.original(ps.death)), death)
    assert _host(ps.last_points()).tobytes() == last.tobytes()
    for ch in (1, 2):
        assert got[:, :, ch].tobytes() == want[:, :, ch].tobytes(), ch
    assert np.array_equal(np.isnan(got[:, :, 0]), ~valid) and np.all(got[:, :, 3] == 1.0)
    again = _check(case.lat, last, death, horizon, f"end to end, method {method}, backward {backward}")
    assert again.tobytes() == got.tobytes()
    print(f"method {method} backward {backward}: {int((death >= 0).sum())} dead, {int(valid.sum())} of {n} pixels valid, "
          f"ftle range {np.nanmin(got[:, :, 0]):.4g} .. {np.nanmax(got[:, :, 0]):.4g} per day")


def test_chain_drops_a_particle_that_died_in_any_pair(case):
    """Two pairs with MOPS_RK4 and record_t equal to the pair gap: a pair holds one record, so a particle that dies
    in pair 0 hands its pre-written seed on as its last point (quirks Q1, a9) and may survive pair 1.  The last
    pair's death_step calls it alive; chain.EverDead's mask makes its pixel NaN."""
    from mops_amd.chain import EverDead, PathlineChain, snapshot_field_factory
    O, GAP = case.O, R.DURATION
    kw = dict(depth=E2E["depth"], delta_t=R.DELTA_T, duration=GAP, record_t=GAP, euler=False)
    r0 = O.run(case.mesh, case.derived[0], case.derived[1], case.seeds, cells=case.cells, **kw)
    r1 = O.run(case.mesh, case.derived[1], case.derived[2], r0["lastPoint"], **kw)
    revived = (r0["death"] >= 0) & (r1["death"] < 0)
    assert revived.any(), "no particle of the lattice dies in pair 0 and survives pair 1"
    ever_ref = (r0["death"] >= 0) | (r1["death"] >= 0)
    chain = PathlineChain(case.dm, snapshot_field_factory(case.dm, lambda i: case.snaps[i]), 3, gap_seconds=GAP)
    ever = EverDead()
    res = chain.run(case.lat.seeds, depth=E2E["depth"], method=0, delta_t=R.DELTA_T, record_t=GAP, keep_lines=False,
                    on_pair=ever)
    assert ever.pairs == 2 and np.array_equal(_host(ever.mask), ever_ref)
    assert np.array_equal(_host(res["death_step"]), r1["death"])
    assert _host(res["lastPoint"]).tobytes() == r1["lastPoint"].tobytes()
    horizon = 2 * GAP / 86400.0
    death = _host(ever.death())
    got = _check(case.lat, r1["lastPoint"], death, horizon, "chain, ever dead")
    assert got.tobytes() == _host(case.lat.ftle(res["lastPoint"], ever.death(), horizon)).tobytes()
    assert np.isnan(got.reshape(-1, 4)[revived, 1]).all()
    naive = _host(case.lat.ftle(res["lastPoint"], res["death_step"], horizon)).reshape(-1, 4)
    print(f"chain: {int((r0['death'] >= 0).sum())} dead in pair 0, {int(revived.sum())} of them alive after pair 1, "
          f"{int((~np.isnan(naive[revived, 1])).sum())} of those would get a value from the last pair's deaths alone")
