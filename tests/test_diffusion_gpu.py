"""GPU: the random-walk horizontal diffusion (mops_traj_advance_diffuse, mops_traj_advance_layer_diffuse,
traj_lane_kernel with its kick, mops_selftest_philox) against its Python restatement (tests/diffusion_reference.py, pinned to
the existing restatements at Kh = 0 by tests/test_diffusion_cpu.py).  Lines are built from the restatement's records
by the oracle's own assembly.  Every parity assertion is bit-exact.  Kh is in m^2/s."""
import ctypes as C

import numpy as np
import pytest

import diffusion_reference as D
import pathline_attr_reference as R
import rk4_relocate_reference as RR

pytestmark = pytest.mark.gpu

EULER, RK4, RELOCATE = 1, 0, 2
METHODS = {"euler": EULER, "rk4": RK4, "rk4_relocate": RELOCATE}
LINE_KEYS = ("points", "velocity", "temperature", "salinity", "lastPoint")
N_STEPS = R.DURATION // R.DELTA_T  # 36
LAYER = 4
SEED = 2024
KH = 2e4


def _host(t):
    return t.cpu().numpy()


def _cfg(method, layer, backward=False, kh=KH, seed=SEED, epoch=0, delta_t=R.DELTA_T, duration=R.DURATION,
         record_t=R.RECORD_T):
    from mops_amd.engine import TrajectoryConfig
    return TrajectoryConfig(deltaT=delta_t, simulationDuration=duration, recordT=record_t, depth=0.0,
                            direction=1 if backward else 0, method=method, layer=layer, diffusivity=kh, seed=seed,
                            epoch=epoch)


class _Case:
    """A mesh and a snapshot pair in the oracle and on the device; restatement runs are computed once per key and
    never modified."""

    def __init__(self, O, mesh, s0, s1):
        from mops_amd.engine import DeviceField, DeviceMesh
        self.O, self.mesh, self.snaps = O, mesh, (s0, s1)
        self.L = mesh.nVertLevels
        self.dm = DeviceMesh.from_mesh(mesh)
        self.r = (O.preprocess(mesh, s0), O.preprocess(mesh, s1))
        self.f = (DeviceField.from_snapshot(self.dm, s0), DeviceField.from_snapshot(self.dm, s1))
        self._ref = {}

    def ref(self, layer, pathline, method, backward=False, kh=KH, seeds=None, depths=None, key="shared", seed=SEED,
            epoch=0, **times):
        k = (key, layer, pathline, method, backward, kh, seed, epoch)
        if k not in self._ref:
            if seeds is None:
                seeds, depths = R.shared_seeds()
            self._ref[k] = D.run_case(self.O, self.mesh, self.r[0], self.r[1] if pathline else None, seeds, depths,
                                      layer=layer, euler=method == EULER, backward=backward,
                                      relocate=method == RELOCATE, kh=kh, seed=seed, epoch=epoch, **times)
        return self._ref[k]


@pytest.fixture(scope="module")
def case(gpu, engine_lib, oracle_lib, small_case):
    return _Case(oracle_lib, *small_case)


def _check(c, ref, layer, pathline, method, backward=False, kh=KH, **times):
    """run_trajectories with the diffusivity equals the restatement: lines, deaths, final positions, depths."""
    from mops_amd.engine import run_trajectories
    got = run_trajectories(c.dm, c.f[0], c.f[1] if pathline else None,
                           _cfg(method, layer, backward, kh=kh, **times), ref["seeds"], depths=ref["depths"],
                           cells=ref["cells"])
    want = D.lines(c.O, ref, pathline)
    what = (layer, pathline, method, backward, kh)
    assert np.array_equal(got["death_step"], ref["death"]), what
    for k in LINE_KEYS:
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    assert got["final_pos"].tobytes() == ref["final_pos"].tobytes(), what
    assert got["final_depth"].tobytes() == ref["final_depth"].tobytes(), what
    return got


# ---- the generator -------------------------------------------------------------------------------------------
def test_selftest_philox(gpu, engine_lib):
    import torch
    from mops_amd import _lib
    rows = [(0, 0, 0, 0, 0, 0), (0xFFFFFFFF,) * 6,
            (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)]
    rng = np.random.default_rng(11)
    rows += [tuple(int(v) for v in r) for r in rng.integers(0, 2 ** 32, size=(1024, 6), dtype=np.uint64)]
    a = np.array(rows, dtype=np.uint32)
    n = len(a)
    d_in = torch.as_tensor(a.view(np.int32), device="cuda")
    d_w = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    d_r = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    _lib.check(engine_lib.mops_selftest_philox(n, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_w.data_ptr()),
                                               C.c_void_p(d_r.data_ptr()), None), "mops_selftest_philox")
    torch.cuda.synchronize()
    words = _host(d_w).view(np.uint32)
    want = np.array([D.philox4x32_10(r[:4], r[4:]) for r in rows], dtype=np.uint32)
    assert np.array_equal(words, want)
    assert " ".join("%08x" % w for w in words[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert " ".join("%08x" % w for w in words[1]) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert " ".join("%08x" % w for w in words[2]) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    wr = np.array([[D.deviate(w[0]), D.deviate(w[1])] for w in want])
    assert _host(d_r).tobytes() == wr.tobytes()


# ---- layer mode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("method", list(METHODS), ids=list(METHODS))
@pytest.mark.parametrize("pathline", [False, True], ids=["streamline", "pathline"])
def test_layer_parity(case, pathline, method, backward):
    m = METHODS[method]
    ref = case.ref(LAYER, pathline, m, backward)
    _check(case, ref, LAYER, pathline, m, backward)
    alive = int((ref["death"] < 0).sum())
    print(f"layer {LAYER} {'pathline' if pathline else 'streamline'} {method} backward={backward}: alive {alive}, "
          f"kick-induced cell changes {int(ref['kick_changes'].sum())}")
    assert alive >= 20 and int(ref["kick_changes"].sum()) >= 30


def test_layer_parity_large_kh(case):
    ref = case.ref(LAYER, True, EULER, kh=2e5)
    _check(case, ref, LAYER, True, EULER, kh=2e5)
    assert int((ref["death"] < 0).sum()) >= 60


def test_layer_parity_pentagons(case):
    seeds, depths, _ = RR.pentagon_seeds(case.mesh)
    for m in (EULER, RELOCATE):
        ref = case.ref(LAYER, True, m, seeds=seeds, depths=depths, key="pentagon")
        _check(case, ref, LAYER, True, m)
        assert int(ref["kick_changes_poly"].sum()) >= 1


# ---- depth mode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("method", list(METHODS), ids=list(METHODS))
def test_depth_parity(case, method, backward):
    m = METHODS[method]
    ref = case.ref(None, True, m, backward)
    _check(case, ref, None, True, m, backward)
    alive = int((ref["death"] < 0).sum())
    print(f"depth pathline {method} backward={backward}: alive {alive}, kick-induced cell changes "
          f"{int(ref['kick_changes'].sum())}")
    assert alive >= 20 and int(ref["kick_changes"].sum()) >= 30
    assert np.any(ref["final_depth"] != ref["depths"])  # (the real w and the vertical update)


def test_depth_parity_zlevel(gpu, engine_lib, oracle_lib, small_case):
    from mops_amd import synth
    mesh = small_case[0]
    s0 = synth.make_snapshot(mesh, timestep=0, phase=0.0, topography="zlevel")
    s1 = synth.make_snapshot(mesh, timestep=1, phase=0.35, topography="zlevel")
    c = _Case(oracle_lib, mesh, s0, s1)
    for m in (EULER, RELOCATE):
        ref = c.ref(None, True, m, key="zlevel")
        _check(c, ref, None, True, m)
        assert int((ref["death"] < 0).sum()) >= 20


# ---- MAXV 12 and 20 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["me12", "me20"])
def test_wide_stencil(gpu, engine_lib, oracle_lib, key):
    """A MAXV 12 and a MAXV 20 mesh (tests/wide_case.py), Euler, in layer mode and in depth mode.  Kh = 2e4 with the
    240 s step of those cases is a kick scale of 5.4 km, twice the advective step."""
    import wide_case as W
    mesh, s0, s1 = W.world(key)
    c = _Case(oracle_lib, mesh, s0, s1)
    allseeds = W.seeds(key)
    seeds = np.concatenate([allseeds[128:160], allseeds[384:416]])
    depths = np.full(len(seeds), W.DEPTH, dtype=np.float32)
    nv = W.degrees(mesh)
    dt, duration, record_t = W.times(True)
    times = dict(delta_t=dt, duration=duration // 4, record_t=record_t // 3)  # 90 steps, a record every 10: 9
    for layer in (4, None):
        ref = c.ref(layer, True, EULER, seeds=seeds, depths=depths, key=key, **times)
        _check(c, ref, layer, True, EULER, **times)
        print(f"{key} layer={layer}: alive {int((ref['death'] < 0).sum())}, seeds in cells of more than 7 vertices "
              f"{int((nv[ref['cells']] > 7).sum())}, kick-induced cell changes {int(ref['kick_changes'].sum())}")
        assert int((nv[ref["cells"]] > 7).sum()) >= 16
        assert int((ref["death"] < 0).sum()) >= 8


@pytest.mark.parametrize("layer,pathline,m", [(4, False, EULER), (4, False, RK4), (4, False, RELOCATE), (4, True, RK4),
                                              (4, True, RELOCATE), (None, True, RK4), (None, True, RELOCATE)],
                         ids=["layer-stream-euler", "layer-stream-rk4", "layer-stream-relocate", "layer-path-rk4",
                              "layer-path-relocate", "depth-rk4", "depth-relocate"])
@pytest.mark.parametrize("key", ["me12", "me20"])
def test_wide_stencil_other_forms(gpu, engine_lib, oracle_lib, key, layer, pathline, m):
    """The seven forms of the per-lane kernel with the kick that test_wide_stencil does not launch at MAXV 12 and
    20, on its seeds and times (the restatement keeps 63 or 64 of the 64 alive in each)."""
    import wide_case as W
    mesh, s0, s1 = W.world(key)
    c = _Case(oracle_lib, mesh, s0, s1)
    allseeds = W.seeds(key)
    seeds = np.concatenate([allseeds[128:160], allseeds[384:416]])
    depths = np.full(len(seeds), W.DEPTH, dtype=np.float32)
    nv = W.degrees(mesh)
    dt, duration, record_t = W.times(True)
    times = dict(delta_t=dt, duration=duration // 4, record_t=record_t // 3)  # 90 steps, a record every 10: 9
    ref = c.ref(layer, pathline, m, seeds=seeds, depths=depths, key=key, **times)
    _check(c, ref, layer, pathline, m, **times)
    assert int((nv[ref["cells"]] > 7).sum()) >= 16
    assert int((ref["death"] < 0).sum()) >= 8


# ---- invariance ----------------------------------------------------------------------------------------------
def _orig(ps, t):  # [.., slot] -> [.., particle]
    import torch
    out = torch.empty_like(t)
    out[..., ps.ids.long()] = t
    return out.cpu().numpy()


def _set(case, ref, method, layer, **kw):
    from mops_amd.engine import ParticleSet
    return ParticleSet(case.dm, ref["seeds"], ref["depths"], _cfg(method, layer), cells=ref["cells"], **kw)


def _same_state(a, b):
    for k in ("records", "x", "y", "z", "depth", "death", "cell"):
        assert _orig(a, getattr(a, k)).tobytes() == _orig(b, getattr(b, k)).tobytes(), k


@pytest.mark.parametrize("layer,method", [(LAYER, EULER), (None, RELOCATE)], ids=["layer-euler", "depth-relocate"])
def test_invariance(case, layer, method):
    """One launch equals launches over [0, 7), [7, 20), [20, 36) with a reorder between them, advance_pipelined with
    and without compaction, use_order=False, and two particle sets of 40 and 56 particles with id_base 0 and 40; and
    the restatement."""
    import torch
    from mops_amd.engine import ParticleSet
    ref = case.ref(layer, True, method)
    want = D.lines(case.O, ref, True)
    f0, f1 = case.f
    one = _set(case, ref, method, layer)
    one.advance(f0, f1, 0, N_STEPS)
    fin = one.finalize(pathline=True)
    for k in LINE_KEYS:
        assert _host(fin[k]).tobytes() == want[k].tobytes(), k
    assert np.array_equal(_orig(one, one.death), ref["death"])
    assert np.array_equal(_orig(one, one.cell), ref["final_cell"])
    assert _orig(one, one.depth).tobytes() == ref["final_depth"].tobytes()
    two = _set(case, ref, method, layer)
    two.advance(f0, f1, 0, 7)
    two.reorder()
    two.advance(f0, f1, 7, 20)
    two.reorder()
    two.advance(f0, f1, 20, N_STEPS)
    _same_state(two, one)
    cur = torch.cuda.current_stream()
    for compact in (False, True):
        pip = _set(case, ref, method, layer)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for s in streams:
            s.wait_stream(cur)
        pip.advance_pipelined(f0, f1, 0, N_STEPS, streams, 3, compact=compact)
        for s in streams:
            cur.wait_stream(s)
        torch.cuda.synchronize()
        _same_state(pip, one)
    flat = _set(case, ref, method, layer, use_order=False)
    flat.advance(f0, f1, 0, N_STEPS)
    _same_state(flat, one)
    full = _orig(one, one.records)
    for lo, hi in ((0, 40), (40, R.N_SEEDS)):
        part = ParticleSet(case.dm, ref["seeds"][lo:hi], ref["depths"][lo:hi], _cfg(method, layer),
                           cells=ref["cells"][lo:hi], id_base=lo)
        part.advance(f0, f1, 0, N_STEPS)
        assert _orig(part, part.records).tobytes() == np.ascontiguousarray(full[:, :, lo:hi]).tobytes(), (lo, hi)
        assert np.array_equal(_orig(part, part.death), ref["death"][lo:hi])


# ---- Kh = 0 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", [LAYER, None], ids=["layer", "depth"])
def test_kh_zero_is_the_existing_entry(case, engine_lib, layer):
    """diffusivity 0 through advance and run_trajectories, and the _diffuse entries called with kh = 0: the bytes of
    the existing entries."""
    import torch
    from mops_amd import _lib
    from mops_amd.engine import ParticleSet, TrajectoryConfig, run_trajectories
    seeds, depths = R.shared_seeds()
    cells = case.O.knn(case.mesh, seeds)
    f0, f1 = case.f
    plain = TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, method=EULER,
                             layer=layer)
    zero = _cfg(EULER, layer, kh=0.0, seed=99, epoch=3)
    a = run_trajectories(case.dm, f0, f1, plain, seeds, depths=depths, cells=cells)
    b = run_trajectories(case.dm, f0, f1, zero, seeds, depths=depths, cells=cells)
    for k in LINE_KEYS + ("final_pos", "final_depth", "death_step"):
        assert a[k].tobytes() == b[k].tobytes(), k
    pa = ParticleSet(case.dm, seeds, depths, plain, cells=cells)
    pb = ParticleSet(case.dm, seeds, depths, zero, cells=cells)
    pa.advance(f0, f1, 0, N_STEPS)
    pb.advance(f0, f1, 0, N_STEPS)
    _same_state(pa, pb)
    # the C entries with kh = 0
    pc = ParticleSet(case.dm, seeds, depths, plain, cells=cells)
    dif = _lib.Diffusion(0.0, 5, 1, 7, C.c_void_p(pc.ids.data_ptr()))
    prt, c = pc.particles(), plain.ctype()
    rec = C.c_void_p(pc.records.data_ptr())
    if layer is None:
        st = engine_lib.mops_traj_advance_diffuse(case.dm.handle, f0.handle, f1.handle, C.byref(c), C.byref(prt),
                                                  C.byref(dif), 0, N_STEPS, rec, pc.rec_stride, None)
    else:
        s0, s1 = f0.layer_velocity(layer), f1.layer_velocity(layer)
        torch.cuda.synchronize()
        st = engine_lib.mops_traj_advance_layer_diffuse(case.dm.handle, C.c_void_p(s0.data_ptr()),
                                                        C.c_void_p(s1.data_ptr()), C.byref(c), C.byref(prt),
                                                        C.byref(dif), 0, N_STEPS, rec, pc.rec_stride, None)
    assert st == _lib.MOPS_OK
    torch.cuda.synchronize()
    _same_state(pc, pa)
    assert int((_orig(pa, pa.death) < 0).sum()) >= 20


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals(case, engine_lib):
    """A depth-mode streamline, attrs with diffusivity > 0, a negative and a NaN Kh: each refused before any launch."""
    import torch
    from mops_amd import _lib
    from mops_amd.chain import PathlineChain, snapshot_attr_factory, snapshot_field_factory
    from mops_amd.engine import ParticleSet, cell_to_vertex_attr, run_trajectories
    ref = case.ref(None, True, EULER)
    f0, f1 = case.f
    s0, s1 = case.snaps
    cfg = _cfg(EULER, None)
    ps = ParticleSet(case.dm, ref["seeds"], ref["depths"], cfg, cells=ref["cells"])
    att = (cell_to_vertex_attr(case.dm, s0.attributes["temperature"]),
           cell_to_vertex_attr(case.dm, s1.attributes["temperature"]))
    ps.records.fill_(-7.0)
    torch.cuda.synchronize()
    before = {k: getattr(ps, k).clone() for k in ("x", "y", "z", "depth", "cell", "death", "records")}
    lib, m = engine_lib, case.dm.handle
    prt, c = ps.particles(), cfg.ctype()
    rec = C.c_void_p(ps.records.data_ptr())
    ids = C.c_void_p(ps.ids.data_ptr())
    sl = C.c_void_p(f0.layer_velocity(LAYER).data_ptr())
    torch.cuda.synchronize()
    good = _lib.Diffusion(KH, SEED, 0, 0, ids)
    # a depth-mode streamline
    assert lib.mops_traj_advance_diffuse(m, f0.handle, None, C.byref(c), C.byref(prt), C.byref(good), 0, N_STEPS, rec,
                                         ps.rec_stride, None) == _lib.MOPS_ERR_UNSUPPORTED
    assert b"streamline" in lib.mops_last_error()
    with pytest.raises(ValueError, match="streamline"):
        run_trajectories(case.dm, f0, None, cfg, ref["seeds"], depths=ref["depths"], cells=ref["cells"])
    with pytest.raises(ValueError, match="streamline"):
        ps.advance(f0, None, 0, N_STEPS)
    with pytest.raises(ValueError, match="streamline"):
        ps.advance_pipelined(f0, None, 0, N_STEPS, [torch.cuda.current_stream()], 2)
    # a negative, a NaN and an infinite Kh
    for bad in (-1.0, float("nan"), float("inf")):
        d = _lib.Diffusion(bad, SEED, 0, 0, ids)
        assert lib.mops_traj_advance_diffuse(m, f0.handle, f1.handle, C.byref(c), C.byref(prt), C.byref(d), 0, N_STEPS,
                                             rec, ps.rec_stride, None) == _lib.MOPS_ERR_INVALID
        assert b"diffusivity" in lib.mops_last_error()
        assert lib.mops_traj_advance_layer_diffuse(m, sl, None, C.byref(c), C.byref(prt), C.byref(d), 0, N_STEPS, rec,
                                                   ps.rec_stride, None) == _lib.MOPS_ERR_INVALID
        with pytest.raises(ValueError, match="diffusivity"):
            run_trajectories(case.dm, f0, f1, _cfg(EULER, None, kh=bad), ref["seeds"], depths=ref["depths"],
                             cells=ref["cells"])
        ps.set_config(_cfg(EULER, None, kh=bad))
        with pytest.raises(ValueError, match="diffusivity"):
            ps.advance(f0, f1, 0, N_STEPS)
        ps.set_config(cfg)
    assert lib.mops_traj_advance_diffuse(m, f0.handle, f1.handle, C.byref(c), C.byref(prt), None, 0, N_STEPS, rec,
                                         ps.rec_stride, None) == _lib.MOPS_ERR_INVALID
    # attrs with diffusivity > 0
    with pytest.raises(ValueError, match="diffusivity"):
        run_trajectories(case.dm, f0, f1, cfg, ref["seeds"], attrs={"temperature": att})
    with pytest.raises(ValueError, match="diffusivity"):
        ps.advance(f0, f1, 0, N_STEPS, attrs=([att[0]], [att[1]]))
    with pytest.raises(ValueError, match="diffusivity"):
        ps.advance_pipelined(f0, f1, 0, N_STEPS, [torch.cuda.current_stream()], 2, attrs=([att[0]], [att[1]]))
    snaps = [s0, s1]
    chain = PathlineChain(case.dm, snapshot_field_factory(case.dm, lambda i: snaps[i]), 2, gap_seconds=R.DURATION,
                          make_attrs=snapshot_attr_factory(case.dm, lambda i: snaps[i]))
    kw = dict(depth=300.0, method=EULER, delta_t=R.DELTA_T, record_t=R.RECORD_T)
    with pytest.raises(ValueError, match="diffusivity"):
        chain.run(ref["seeds"], attrs=True, diffusivity=KH, **kw)
    with pytest.raises(ValueError, match="diffusivity"):
        chain.run(ref["seeds"], diffusivity=-1.0, **kw)
    torch.cuda.synchronize()
    for k, v in before.items():  # nothing was launched: state and records as they were
        assert torch.equal(getattr(ps, k), v), k
    # ... and the same call with a back field and a valid Kh runs
    assert lib.mops_traj_advance_diffuse(m, f0.handle, f1.handle, C.byref(c), C.byref(prt), C.byref(good), 0, N_STEPS,
                                         rec, ps.rec_stride, None) == _lib.MOPS_OK
    torch.cuda.synchronize()
    assert np.array_equal(_orig(ps, ps.death), ref["death"])


# ---- chain ---------------------------------------------------------------------------------------------------
GAPS = [21600, 7200]       # a six-hour and a two-hour pair
CHAIN_DT, CHAIN_RT = 600, 3600   # 36 + 12 steps, 6 + 2 records
CHAIN_DEPTH = 300.0
CHAIN_KH = 2e5             # (kick scale 26.8 km per ten-minute step)


class _ChainSetup:
    def __init__(self, O, mesh):
        from mops_amd import synth
        from mops_amd.engine import DeviceMesh
        self.O, self.mesh = O, mesh
        self.snaps = [synth.make_snapshot(mesh, timestep=t, phase=0.35 * t) for t in range(3)]
        self.derived = [O.preprocess(mesh, s) for s in self.snaps]
        self.dm = DeviceMesh.from_mesh(mesh)
        self.seeds, _ = R.shared_seeds()
        self._ref = {}

    def chain(self):
        from mops_amd.chain import PathlineChain, snapshot_field_factory
        return PathlineChain(self.dm, snapshot_field_factory(self.dm, lambda i: self.snaps[i]), 3, gap_seconds=GAPS)

    def reference(self, layer, epochs=(0, 1)):
        """The restatement chained by hand: pair by pair with the carried lastPoint (MOPSPathline.run's rules), pair p
        with epoch ``epochs[p]``."""
        key = (layer, tuple(epochs))
        if key in self._ref:
            return self._ref[key]
        O = self.O
        acc = {k: [] for k in ("points", "velocity", "temperature", "salinity")}
        recs = []
        last, death = None, None
        depths = np.full(len(self.seeds), CHAIN_DEPTH, dtype=np.float32)
        for p in range(2):
            s = self.seeds if p == 0 else last
            r = D.run_case(O, self.mesh, self.derived[p], self.derived[p + 1], s, depths, layer=layer, euler=True,
                           kh=CHAIN_KH, seed=SEED, epoch=epochs[p], delta_t=CHAIN_DT, duration=GAPS[p],
                           record_t=CHAIN_RT)
            fin = D.lines(O, r, True)
            for k in acc:
                acc[k].append(fin[k][:, (0 if p == 0 else 1):])
            recs.append(r)
            last, death = fin["lastPoint"].copy(), r["death"]
        out = {k: np.concatenate(v, 1) for k, v in acc.items()}
        out.update(lastPoint=last, death_step=death, pairs=recs)
        self._ref[key] = out
        return out


@pytest.fixture(scope="module")
def chain_setup(gpu, engine_lib, oracle_lib, small_case):
    return _ChainSetup(oracle_lib, small_case[0])


def _chain_kw(layer):
    return dict(depth=CHAIN_DEPTH, method=EULER, delta_t=CHAIN_DT, record_t=CHAIN_RT, layer=layer,
                diffusivity=CHAIN_KH, seed=SEED)


@pytest.mark.parametrize("mode", ["default", "defer", "sink", "compact"])
@pytest.mark.parametrize("layer", [None, LAYER], ids=["depth", "layer"])
def test_chain(chain_setup, layer, mode):
    import torch
    from mops_amd.chain import HostLineSink
    want = chain_setup.reference(layer)
    n = len(chain_setup.seeds)
    assert want["points"].shape == (n, 7 + 2, 3)
    assert int((want["death_step"] < 0).sum()) >= 20
    kw = _chain_kw(layer)
    if mode == "sink":
        sink = HostLineSink(n, GAPS[0] // CHAIN_RT, torch.device("cuda", torch.cuda.current_device()), keep_all=True)
        res = chain_setup.chain().run(chain_setup.seeds, keep_lines=False, on_lines=sink, lines_chunk=50, **kw)
        sink.synchronize()
        c0 = 0
        for p in range(2):
            h = sink.host(p)
            ids = h["ids"].numpy().astype(np.int64)
            w = h["points"].shape[1]
            for k in ("points", "temperature", "salinity"):
                assert np.array_equal(h[k].numpy(), want[k][ids, c0:c0 + w]), (p, k)
            c0 += w
        assert c0 == 9
        assert _host(res["lastPoint"]).tobytes() == want["lastPoint"].tobytes()
        return
    extra = dict(default={}, defer=dict(defer_lines=True), compact=dict(compact=True))[mode]
    got = chain_setup.chain().run(chain_setup.seeds, **extra, **kw)
    for k in LINE_KEYS:
        assert _host(got[k]).tobytes() == want[k].tobytes(), k
    assert np.array_equal(_host(got["death_step"]), want["death_step"])


@pytest.mark.parametrize("layer", [None, LAYER], ids=["depth", "layer"])
def test_chain_density(chain_setup, layer):
    """A count map of a diffusive chain: bytes-equal to density_reference fed with the restatement's records, under
    that file's own margin pre-check."""
    import density_reference as DR
    from mops_amd.engine import DensityMap
    win = (48, 24, (-90.0, 90.0), (-180.0, 180.0))
    want_run = chain_setup.reference(layer)
    acc = DR.new_accum(win[0], win[1])
    n = len(chain_setup.seeds)
    for p, r in enumerate(want_run["pairs"]):
        Kp = GAPS[p] // CHAIN_RT
        rec = np.zeros((Kp, 6, n))
        rec[:, 0:3, :] = r["rec_pos"].transpose(1, 2, 0)
        pts = rec[:, 0:3, :].transpose(0, 2, 1).reshape(-1, 3)
        assert DR.edge_distance(pts, *win) > DR.EDGE_GUARD
        assert DR.edge_distance(r["seeds"], *win) > DR.EDGE_GUARD
        DR.records_accumulate(acc, rec, n, *win, kind=DR.COUNT, seeds=r["seeds"] if p == 0 else None)
    m = DensityMap(win[0], win[1], win[2], win[3])
    chain_setup.chain().run(chain_setup.seeds, keep_lines=False, density=m, **_chain_kw(layer))
    got = _host(m.accum)
    assert int(acc[:, :, 0].sum()) > n
    assert got.dtype == np.int64 and got.tobytes() == acc.tobytes()


def test_chain_epochs(chain_setup):
    """The chain uses the epochs 0 and 1; with both forced equal the second pair draws other deviates."""
    want = chain_setup.reference(LAYER)
    same = chain_setup.reference(LAYER, epochs=(0, 0))
    kw = _chain_kw(LAYER)
    got = chain_setup.chain().run(chain_setup.seeds, epochs=[0, 0], **kw)
    for k in LINE_KEYS:
        assert _host(got[k]).tobytes() == same[k].tobytes(), k
    alive = (want["death_step"] < 0) & (same["death_step"] < 0)
    assert int(alive.sum()) >= 20
    assert np.array_equal(same["points"][:, :7], want["points"][:, :7])  # (pair 0: epoch 0 in both)
    assert np.all(np.any(same["points"][alive, 7:] != want["points"][alive, 7:], axis=(1, 2)))
