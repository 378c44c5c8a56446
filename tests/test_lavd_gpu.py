"""GPU: the path-integral and LAVD entries (mops_level_mean, mops_path_integral_abs, mops_path_integral_image)
through engine.level_mean / vorticity_deviation / PathIntegral / FlowMapLattice.lavd and
PathlineChain.run(integrals=...), against the numpy restatement (tests/lavd_reference.py, pinned by
tests/test_lavd_cpu.py).  Every comparison is bit-exact, NaNs at equal places: the kernels use + - * / and fabs
only, without contraction, in the header's order."""
import numpy as np
import pytest

import census_reference as CR
import eddy_case as EC
import eddy_reference as ER
import lavd_reference as LR
import pathline_attr_reference as R

pytestmark = pytest.mark.gpu

NAME = "vorticity_deviation"
DT, RT, GAP = 600, 3600, 21600
K = GAP // RT
DEPTH = 300.0
W, H = EC.WIDTH, EC.HEIGHT   # 36 x 18 = 648 particles: no multiple of 64


def _host(t):
    return t.cpu().numpy()


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else \
        torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype)


# ---- 1. mops_level_mean ---------------------------------------------------------------------------------------
def _mean_data(C_, L_, seed):
    """Random signed data with NaNs scattered, zero and NaN weights, and (from two levels on) one level all NaN."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C_, L_)) * 1e-5
    w = rng.uniform(0.5, 2.0, C_) * 1e9
    if C_ > 2:
        x[rng.random((C_, L_)) < 0.1] = np.nan
        x[rng.integers(0, C_), rng.integers(0, L_)] = np.inf
        w[rng.random(C_) < 0.15] = 0.0
        w[rng.integers(0, C_)] = np.nan
        w[rng.integers(0, C_)] = -3.0
    if L_ > 1:
        x[:, L_ // 2] = np.nan
    return x, w


@pytest.mark.parametrize("side", [False, True], ids=["current", "side-stream"])
@pytest.mark.parametrize("C_,L_", [(1, 1), (63, 10), (64, 64), (65, 65), (129, 3), (None, 10)])
def test_level_mean(gpu, engine_lib, small_case, C_, L_, side):
    import torch
    from mops_amd.engine import level_mean
    if C_ is None:
        C_ = small_case[0].nCells
        assert C_ % LR.GROUP != 0 and C_ > 2000 and small_case[0].nVertLevels == L_   # a ragged last group
    x, w = _mean_data(C_, L_, seed=C_ * 131 + L_)
    want_m, want_s = LR.level_mean(x, w)
    dx, dw = _dev(x), _dev(w)
    torch.cuda.synchronize()
    if side:
        s = torch.cuda.Stream()
        mean, wsum = level_mean(dx, dw, stream=s)
        assert torch.cuda.current_stream() != s
        s.synchronize()
    else:
        mean, wsum = level_mean(dx, dw)
    assert tuple(mean.shape) == tuple(wsum.shape) == (L_,)
    assert LR.same(_host(mean), want_m), (C_, L_)
    assert _host(wsum).tobytes() == want_s.tobytes(), (C_, L_)
    if L_ > 1:
        assert np.isnan(want_m[L_ // 2]) and want_s[L_ // 2] == 0.0
        assert np.isfinite(np.delete(want_m, L_ // 2)).all()


def test_vorticity_deviation_composes_the_entries(gpu, engine_lib, oracle_lib, small_case):
    import torch
    from mops_amd.engine import DeviceField, DeviceMesh, cell_area, vorticity_deviation
    c = EC.small(oracle_lib, small_case)
    dm = DeviceMesh.from_mesh(c["mesh"])
    df = DeviceField.from_snapshot(dm, c["s0"])
    area = CR.cell_area(c["mesh"])
    vort = c["g0"]["vorticity"]
    mean, _ = LR.level_mean(vort, area)
    dev_c, got_mean = vorticity_deviation(dm, df, vertex=False)
    assert LR.same(_host(got_mean), mean) and LR.same(_host(dev_c), LR.deviation(vort, mean))
    dev_v, _ = vorticity_deviation(dm, df)
    assert LR.same(_host(dev_v), ER.cell_to_vertex_signed(c["mesh"], LR.deviation(vort, mean)))
    # a masked weight confines the mean; on a side stream the same bytes
    mask = np.where(np.arange(len(area)) % 2 == 0, area, 0.0)
    m2, _ = LR.level_mean(vort, mask)
    s = torch.cuda.Stream()
    dw = _dev(mask)
    torch.cuda.synchronize()
    d2, g2 = vorticity_deviation(dm, df, weight=dw, vertex=False, stream=s)
    s.synchronize()
    assert LR.same(_host(g2), m2) and LR.same(_host(d2), LR.deviation(vort, m2)) and not LR.same(m2, mean)
    assert _host(cell_area(dm)).tobytes() == area.tobytes()


# ---- 2. mops_path_integral_abs --------------------------------------------------------------------------------
class _FakeSet:
    """What PathIntegral.accumulate reads of a ParticleSet: an attribute slab [K][n_attr][stride], ids, cfg."""

    def __init__(self, slab, ids, record_t, n):
        import types
        self.attr_records, self.ids, self.n = slab, ids, n
        self.K, self.n_attr, self.rec_stride = int(slab.shape[0]), int(slab.shape[1]), int(slab.shape[2])
        self.cfg = types.SimpleNamespace(recordT=record_t)


@pytest.mark.parametrize("K_", [1, 7])
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_path_integral_slab_and_lines(gpu, engine_lib, n, K_):
    import torch
    from mops_amd.engine import PathIntegral
    rng = np.random.default_rng(n * 10 + K_)
    stride, n_attr, row = n + 3, 2, 1
    slab = rng.standard_normal((K_, n_attr, stride)) * 1e-5
    ids = rng.permutation(n).astype(np.int32)
    start = rng.uniform(0.0, 1.0, n)
    vals = slab[:, row, :n]                                  # [K, n] in slot order
    want = start.copy()
    want[ids] = LR.path_integral(vals, 3600.0, start=start[ids])
    ps = _FakeSet(_dev(slab), _dev(ids), -3600, n)           # (a backward run's recordT: |recordT| is the weight)
    it = PathIntegral(n)
    it.accum.copy_(_dev(start))                              # a pre-filled accumulator
    it.accumulate(ps, "b", names=["a", "b"])
    assert _host(it.accum).tobytes() == want.tobytes()
    # two calls over [0, 3) and [3, K) equal one call over [0, K): through the entry's own range
    if K_ == 7:
        from mops_amd import _lib
        import ctypes as C
        two = _dev(start)
        base = ps.attr_records.data_ptr() + 8 * row * stride
        for k0, k1 in ((0, 3), (3, 7)):
            _lib.check(engine_lib.mops_path_integral_abs(n, k0, k1, C.c_void_p(base), n_attr * stride, 1,
                                                         C.c_void_p(ps.ids.data_ptr()), 3600.0,
                                                         C.c_void_p(two.data_ptr()),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "mops_path_integral_abs")
        assert _host(two).tobytes() == want.tobytes()
        it.reset()
        it.accumulate(ps, "b", names=["a", "b"], n_records=3, weight=2.0)
        first = np.zeros(n); first[ids] = LR.path_integral(vals[:3], 2.0)
        assert _host(it.accum).tobytes() == first.tobytes()
    with pytest.raises(ValueError, match="samples no attribute"):
        it.accumulate(ps, "c", names=["a", "b"])
    # the lines layout [n, P] (seed order, identity ids), entry K dropped by default
    lines = np.concatenate([vals.T, np.full((n, 1), 7.0)], axis=1)
    il = PathIntegral(n)
    il.accumulate_lines(lines, 3600.0)
    assert _host(il.accum).tobytes() == LR.path_integral(vals, 3600.0).tobytes()
    il.accumulate_lines(_dev(lines), 0.5, skip_last=False)
    assert _host(il.accum).tobytes() == LR.path_integral(lines.T, 0.5, start=LR.path_integral(vals, 3600.0)).tobytes()
    # a NaN sample propagates, into its own particle only
    bad = vals.copy(); bad[K_ // 2, n // 2] = np.nan
    ib = PathIntegral(n)
    ib.accumulate_lines(bad.T.copy(), 1.0, skip_last=False)
    got = _host(ib.accum)
    assert np.isnan(got[n // 2]) and LR.same(got, LR.path_integral(bad, 1.0)) and np.isnan(got).sum() == 1


# ---- 3. mops_path_integral_image ------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [False, True], ids=["current", "side-stream"])
def test_path_integral_image(gpu, engine_lib, side):
    import torch
    from mops_amd.engine import FlowMapLattice
    la = FlowMapLattice(13, 5, (-10.0, 10.0), (0.0, 40.0))   # n = 65
    rng = np.random.default_rng(4)
    acc = rng.uniform(0.0, 3.0, la.n)
    acc[7] = np.inf; acc[9] = np.nan; acc[64] = 0.0
    death = np.full(la.n, -1, dtype=np.int32)
    death[::6] = 0; death[11] = 5
    dacc, dd = _dev(acc), _dev(death)
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if side else None
    for d, dn in ((None, None), (dd, death)):
        got = la.lavd(dacc, d, horizon=21600.0, stream=s)
        if side:
            s.synchronize()
        assert tuple(got.shape) == (5, 13, 4)
        assert LR.same(_host(got).reshape(-1, 4), LR.image(acc, dn, 21600.0))
    assert LR.same(_host(la.lavd(acc, death.astype(np.int64), horizon=2.0)).reshape(-1, 4), LR.image(acc, death, 2.0))
    with pytest.raises(ValueError):
        la.lavd(dacc[:-1], None, horizon=1.0)


# ---- 4. end to end: a single pair, and the chain --------------------------------------------------------------
class _Case:
    """Three synth snapshots on small_case, the lattice on eddy_case's window, and the restatement pair by pair
    with tests/test_chain.py's seed rules (pair p > 0 starts from pair p - 1's lastPoint)."""

    def __init__(self, O, mesh):
        from mops_amd import synth
        from mops_amd.engine import DeviceMesh, FlowMapLattice
        self.O, self.mesh = O, mesh
        self.snaps = [synth.make_snapshot(mesh, timestep=t, phase=0.35 * t) for t in range(3)]
        self.dm = DeviceMesh.from_mesh(mesh)
        self.lat = FlowMapLattice(W, H, EC.LAT, EC.LON)
        self.seeds = _host(self.lat.seeds)
        area = CR.cell_area(mesh)
        self.derived, self.means = [], []
        for s in self.snaps:
            d = O.preprocess(mesh, s)
            vort = ER.velocity_gradient(mesh, d.vertex_vel)["vorticity"]
            mean, _ = LR.level_mean(vort, area)
            v = ER.cell_to_vertex_signed(mesh, LR.deviation(vort, mean))
            self.means.append(mean)
            self.derived.append(O.Derived(d.vertex_ztop, d.vertex_vel, d.vertex_w, {NAME: v.reshape(-1)}))
        n = self.lat.n
        self.pairs = []   # per pair: dict(values [K, n], death, integral after the pair)
        s, acc = self.seeds, np.zeros(n)
        for p in range(2):
            depths = np.full(n, DEPTH, dtype=np.float32)
            r = R.run(mesh, self.derived[p], self.derived[p + 1], s, depths, O.knn(mesh, s), DT, GAP, RT, euler=True,
                      names=[NAME])
            vals = np.ascontiguousarray(r["rec_attr"][:, :, 0].T)
            acc = LR.path_integral(vals, float(RT), start=acc)
            lines = R.attr_lines(O, s, r, K)[0]
            self.pairs.append(dict(values=vals, death=r["death"].copy(), integral=acc.copy(), lines=lines))
            s = O.finalize_lines(s, r["rec_pos"], r["rec_vel"], K, with_attrs=False)["lastPoint"].copy()
        self._keep = None

    def chain(self, n_snap=3, make_field=None, **kw):
        from mops_amd.chain import PathlineChain, snapshot_field_factory, vorticity_deviation_factory
        mf = make_field or snapshot_field_factory(self.dm, lambda i: self.snaps[i])
        make_attrs = vorticity_deviation_factory(self.dm)
        return PathlineChain(self.dm, mf, n_snap, gap_seconds=GAP, make_attrs=make_attrs, **kw), make_attrs

    def run(self, n_snap=3, chain_kw=None, **kw):
        """(accum bytes-ready array, EverDead death, result, make_attrs) of one chain run with an integral."""
        from mops_amd.chain import EverDead
        from mops_amd.engine import PathIntegral
        chain, make_attrs = self.chain(n_snap, **(chain_kw or {}))
        it, ever = PathIntegral(self.lat.n), EverDead()
        kw.setdefault("keep_lines", False)
        res = chain.run(self.lat.seeds, depth=DEPTH, method=1, delta_t=DT, record_t=RT, attrs=True,
                        integrals={NAME: it}, on_pair=ever, **kw)
        return it, ever, res, make_attrs


@pytest.fixture(scope="module")
def case(gpu, engine_lib, oracle_lib, small_case):
    return _Case(oracle_lib, small_case[0])


def test_end_to_end_single_pair(case):
    n = case.lat.n
    p0 = case.pairs[0]
    horizon = float(K * RT)
    want = LR.image(p0["integral"], p0["death"], horizon)
    # the reference alone: enough live pixels, land, and a map that is not flat
    fin = np.isfinite(want[:, 0])
    assert 4 * int(fin.sum()) >= n and np.isnan(want[:, 0]).any() and np.unique(want[fin, 0]).size > 1
    assert np.array_equal(fin, p0["death"] < 0) and (want[fin, 0] >= 0).all()
    it, ever, res, make_attrs = case.run(n_snap=2, keep_lines=True)
    assert make_attrs.seen == [0, 1]
    for i in (0, 1):
        assert LR.same(_host(make_attrs.means[i]), case.means[i]), i
    assert np.array_equal(_host(res["death_step"]), p0["death"])
    assert LR.same(_host(res["attributes"][NAME]), p0["lines"])
    assert _host(it.accum).tobytes() == p0["integral"].tobytes()
    img = case.lat.lavd(it, ever.death(), horizon=horizon)
    assert tuple(img.shape) == (H, W, 4) and LR.same(_host(img).reshape(-1, 4), want)
    # the finished lines of the single pair give the same integral
    from mops_amd.engine import PathIntegral
    il = PathIntegral(n)
    il.accumulate_lines(res["attributes"][NAME], float(RT))
    assert _host(il.accum).tobytes() == p0["integral"].tobytes()
    print(f"single pair: {int(fin.sum())} of {n} pixels finite, LAVD {np.nanmin(want[:, 0]):.4g} .. "
          f"{np.nanmax(want[:, 0]):.4g}, mean |deviation| up to {np.nanmax(want[:, 1]):.4g} 1/s")


def test_chain_matches_the_pair_by_pair_restatement(case):
    want = case.pairs[1]["integral"]
    ever_ref = (case.pairs[0]["death"] >= 0) | (case.pairs[1]["death"] >= 0)
    it, ever, res, make_attrs = case.run(keep_lines=True)
    assert make_attrs.seen == [0, 1, 2]
    assert _host(it.accum).tobytes() == want.tobytes()
    assert not np.array_equal(want, case.pairs[0]["integral"])      # pair 1 added something
    assert np.array_equal(_host(ever.mask), ever_ref)
    horizon = float(2 * K * RT)
    img = _host(case.lat.lavd(it, ever.death(), horizon=horizon)).reshape(-1, 4)
    assert LR.same(img, LR.image(want, np.where(ever_ref, 0, -1), horizon))
    dead0 = case.pairs[0]["death"] >= 0
    assert dead0.any() and np.isnan(img[dead0, :3]).all() and (img[:, 3] == 1.0).all()
    case._keep = _host(it.accum).tobytes()
    # the integral left the run's other results alone
    plain = case.chain()[0].run(case.lat.seeds, depth=DEPTH, method=1, delta_t=DT, record_t=RT, attrs=True)
    for k in ("points", "lastPoint", "death_step"):
        assert _host(plain[k]).tobytes() == _host(res[k]).tobytes(), k
    assert _host(plain["attributes"][NAME]).tobytes() == _host(res["attributes"][NAME]).tobytes()


def _on_lines(p, lines, ids):
    pass


@pytest.mark.parametrize("mode", ["defer_lines", "on_lines", "compact", "segment_steps0", "capture_slots0",
                                  "no_prefetch", "segments_reorder"])
def test_chain_modes_give_the_keep_lines_bytes(case, mode):
    want = case.pairs[1]["integral"].tobytes()
    kw, ckw = {}, {}
    if mode == "defer_lines":
        kw = dict(keep_lines=True, defer_lines=True)
    elif mode == "on_lines":
        kw = dict(on_lines=_on_lines, lines_chunk=100)
    elif mode == "compact":
        kw = dict(compact=True)
    elif mode == "segment_steps0":
        kw = dict(segment_steps=0)
    elif mode == "capture_slots0":
        kw = dict(capture_slots=0)
    elif mode == "no_prefetch":
        ckw = dict(prefetch=False)
    else:
        kw = dict(segment_steps=7, reorder=True, capture_slots=2)
    it, ever, res, make_attrs = case.run(chain_kw=ckw, **kw)
    assert make_attrs.seen == [0, 1, 2], mode
    assert _host(it.accum).tobytes() == want, mode
    assert np.array_equal(_host(ever.mask), (case.pairs[0]["death"] >= 0) | (case.pairs[1]["death"] >= 0))


def test_recycled_fields_hand_the_refilled_field_on(case):
    """A recycling make_field (snapshot p's buffers re-derived as p + 2 on the compute stream): the derived
    factory sees every snapshot, with the field that holds it."""
    import torch
    from mops_amd.engine import DeviceField
    keys = ("layerThickness", "bottomDepth", "zonalVelocity", "meridionalVelocity", "vertVelocityTop")
    keep = []

    def raw(i):
        d = {k: torch.as_tensor(getattr(case.snaps[i], k), device="cuda") for k in keys}
        keep.append(d)
        return d

    class Recycle:
        def __call__(self, i, stream):
            d = raw(i)
            torch.cuda.current_stream().synchronize()
            return DeviceField.from_device_snapshot(case.dm, d, timestep=i, stream=stream)

        def refill(self, field, i, stream):
            d = raw(i)
            stream.wait_stream(torch.cuda.current_stream())
            return field.rebuild_from_device(d, timestep=i, stream=stream.cuda_stream)

    it, ever, res, make_attrs = case.run(chain_kw=dict(make_field=Recycle(), prefetch=False))
    assert make_attrs.seen == [0, 1, 2]
    assert _host(it.accum).tobytes() == case.pairs[1]["integral"].tobytes()


def test_overlap_stream_builds_the_derived_attributes_beside_the_pair(gpu, engine_lib, small_case):
    """The overlap schedule (device-generated snapshots, a CU-masked side stream): the integral equals the serial
    recycling chain's, and the factory saw field= for every snapshot on both."""
    import torch
    from mops_amd.chain import PathlineChain, cu_split_streams, vorticity_deviation_factory
    from mops_amd.engine import DeviceMesh, FlowMapLattice, PathIntegral
    from mops_amd.synth_device import DeviceFieldRecycler, DeviceSnapshotSource
    mesh = small_case[0]
    dm = DeviceMesh.from_mesh(mesh)
    lat = FlowMapLattice(W, H, EC.LAT, EC.LON)
    n_snap, out = 4, []
    for overlap in (False, True):
        rec = DeviceFieldRecycler(dm, DeviceSnapshotSource(mesh, "cuda"))
        compute, side = cu_split_streams("cuda", 8) if overlap else (torch.cuda.Stream(), None)
        if overlap:
            rec.side = side
        cs = torch.cuda.current_stream().cuda_stream
        bufs = [rec(i, cs) for i in range(3 if overlap else 2)]
        for b in bufs:
            rec.release(b)
        torch.cuda.synchronize()
        make_attrs = vorticity_deviation_factory(dm)
        chain = PathlineChain(dm, rec, n_snap, gap_seconds=GAP, prefetch=False, overlap_stream=side,
                              make_attrs=make_attrs)
        it = PathIntegral(lat.n)
        torch.cuda.synchronize()
        chain.run(lat.seeds, depth=DEPTH, method=1, delta_t=DT, record_t=RT, attrs=True, keep_lines=False,
                  integrals={NAME: it}, compute_stream=compute)
        torch.cuda.synchronize()
        assert make_attrs.seen == list(range(n_snap)), overlap
        out.append(_host(it.accum))
    assert out[0].tobytes() == out[1].tobytes() and np.isfinite(out[0]).all() and (out[0] > 0).any()


def test_refusals(case):
    from mops_amd.chain import PathlineChain, snapshot_attr_factory, snapshot_field_factory
    from mops_amd.engine import PathIntegral
    it = PathIntegral(case.lat.n)
    chain, _ = case.chain()
    with pytest.raises(ValueError, match="attrs=True"):
        chain.run(case.lat.seeds, depth=DEPTH, method=1, delta_t=DT, record_t=RT, integrals={NAME: it})
    with pytest.raises(ValueError, match="samples no attribute"):
        chain.run(case.lat.seeds, depth=DEPTH, method=1, delta_t=DT, record_t=RT, attrs=True, integrals={"salinity": it})
    with pytest.raises(ValueError, match="particles"):
        chain.run(case.lat.seeds, depth=DEPTH, method=1, delta_t=DT, record_t=RT, attrs=True,
                  integrals={NAME: PathIntegral(5)})
    with pytest.raises(ValueError, match="MOPS_RK4_RELOCATE"):
        chain.run(case.lat.seeds, depth=DEPTH, method=2, delta_t=DT, record_t=RT, attrs=True, integrals={NAME: it})
    # a make_attrs without wants_field is called exactly as before, and its names are what an integral may name
    calls = []
    inner = snapshot_attr_factory(case.dm, lambda i: case.snaps[i])

    def make_attrs(i, stream):
        calls.append(i)
        return inner(i, stream)
    files = PathlineChain(case.dm, snapshot_field_factory(case.dm, lambda i: case.snaps[i]), 3, gap_seconds=GAP,
                          make_attrs=make_attrs)
    with pytest.raises(ValueError, match="samples no attribute"):
        files.run(case.lat.seeds, depth=DEPTH, method=1, delta_t=DT, record_t=RT, attrs=True, integrals={NAME: it})
    files.run(case.lat.seeds, depth=DEPTH, method=1, delta_t=DT, record_t=RT, attrs=True, keep_lines=False,
              integrals={"salinity": it})
    assert calls[-3:] == [0, 1, 2] and float(it.accum.max()) > 0.0
