"""GPU: the pathline RK4 that locates each stage in its own cell (MOPS_RK4_RELOCATE, traj_lane_kernel) against
the Python restatement of the loop (tests/rk4_relocate_reference.py, pinned to the oracle with the switch off by
tests/test_rk4_relocate_cpu.py).  Lines are built from the restatement's records by the oracle's own assembly.
Every parity assertion is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import pathline_attr_reference as R
import rk4_relocate_reference as RR

pytestmark = pytest.mark.gpu

RELOCATE = 2  # MOPS_RK4_RELOCATE
LINE_KEYS = ("points", "velocity", "temperature", "salinity", "lastPoint")
EARTH_RADIUS_M = 6_371_000.0


class _Case:
    """A mesh and a snapshot pair on the device and in the oracle; restatement runs are computed once per key."""

    def __init__(self, O, mesh, s0, s1):
        from mops_amd.engine import DeviceField, DeviceMesh
        self.O, self.mesh, self.s0, self.s1 = O, mesh, s0, s1
        self.dm = DeviceMesh.from_mesh(mesh)
        self.f0, self.f1 = DeviceField.from_snapshot(self.dm, s0), DeviceField.from_snapshot(self.dm, s1)
        self.r0, self.r1 = O.preprocess(mesh, s0), O.preprocess(mesh, s1)
        self._ref = {}

    def ref(self, key, relocate, seeds, depths, backward=False, **kw):
        k = (key, relocate, backward)
        if k not in self._ref:
            self._ref[k] = RR.run_case(self.O, self.mesh, self.r0, self.r1, seeds, depths, backward=backward,
                                       relocate=relocate, **kw)
        return self._ref[k]


def _cfg(method, backward=False, delta_t=R.DELTA_T, duration=R.DURATION, record_t=R.RECORD_T):
    from mops_amd.engine import TrajectoryConfig
    return TrajectoryConfig(deltaT=delta_t, simulationDuration=duration, recordT=record_t, depth=0.0,
                            direction=1 if backward else 0, method=method)


@pytest.fixture(scope="module")
def case(gpu, engine_lib, oracle_lib, small_case):
    return _Case(oracle_lib, *small_case)


def _check(c, key, seeds, depths, backward=False, **times):
    """run_trajectories with method 2 equals the restatement with relocate, method 0 the one without."""
    from mops_amd.engine import run_trajectories
    out = {}
    for method, relocate in ((RELOCATE, True), (0, False)):
        ref = c.ref(key, relocate, seeds, depths, backward, **times)
        got = run_trajectories(c.dm, c.f0, c.f1, _cfg(method, backward, **times), ref["seeds"], depths=ref["depths"],
                               cells=ref["cells"])
        want = RR.lines(c.O, ref)
        assert np.array_equal(got["death_step"], ref["death"]), (key, method)
        for k in LINE_KEYS:
            assert got[k].tobytes() == want[k].tobytes(), (key, method, k)
        assert got["final_depth"].tobytes() == ref["final_depth"].tobytes(), (key, method)
        assert got["final_pos"].tobytes() == ref["final_pos"].tobytes(), (key, method)
        out[relocate] = ref
    return out[True], out[False]


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_parity_shared(case, backward):
    seeds, depths = R.shared_seeds()
    rel, plain = _check(case, "shared", seeds, depths, backward)
    assert int(rel["relocations"].sum()) >= 50 and int((rel["death"] < 0).sum()) > int((plain["death"] < 0).sum())


def test_parity_pentagons(case):
    seeds, depths, _ = RR.pentagon_seeds(case.mesh)
    rel, _ = _check(case, "pentagon", seeds, depths)
    assert int(rel["relocations_poly"].sum()) >= 10


def test_parity_two_hop(case):
    seeds, depths = R.shared_seeds()
    rel, _ = _check(case, "twohop", seeds, depths, delta_t=RR.TWO_HOP_DELTA_T,
                    duration=RR.TWO_HOP_STEPS * RR.TWO_HOP_DELTA_T,
                    record_t=RR.TWO_HOP_RECORD_EVERY * RR.TWO_HOP_DELTA_T)
    assert int(((rel["death"] > 0) & (rel["relocations"] > 0)).sum()) >= 3


def test_parity_zlevel(gpu, engine_lib, oracle_lib, small_case):
    from mops_amd import synth
    mesh = small_case[0]
    s0 = synth.make_snapshot(mesh, timestep=0, phase=0.0, topography="zlevel")
    s1 = synth.make_snapshot(mesh, timestep=1, phase=0.35, topography="zlevel")
    seeds, depths = R.shared_seeds()
    rel, _ = _check(_Case(oracle_lib, mesh, s0, s1), "zlevel", seeds, depths)
    assert int(rel["relocations"].sum()) >= 1


@pytest.mark.parametrize("max_edges", [10, 20], ids=["maxv12", "maxv20"])
def test_parity_wide_stencil(gpu, engine_lib, oracle_lib, max_edges):
    """maxEdges 10 / 20 select the MAXV 12 / 20 kernels."""
    from mops_amd import synth
    mesh = synth.make_mesh(16, n_levels=10, max_edges=max_edges)
    s0 = synth.make_snapshot(mesh, timestep=0)
    s1 = synth.make_snapshot(mesh, timestep=1, phase=0.35)
    seeds = synth.uniform_band_seeds(32, seed=41)
    depths = np.random.default_rng(3).uniform(5, 1500, 32).astype(np.float32)
    rel, plain = _check(_Case(oracle_lib, mesh, s0, s1), "wide", seeds, depths)
    print(f"max_edges {max_edges}: alive {int((rel['death'] < 0).sum())} (plain {int((plain['death'] < 0).sum())}), "
          f"relocations {int(rel['relocations'].sum())}")
    assert int(rel["relocations"].sum()) >= 10
    assert int((rel["death"] < 0).sum()) > int((plain["death"] < 0).sum())


@pytest.mark.parametrize("n", [0, 1], ids=["N0", "N1"])
def test_tiny_counts(case, n):
    from mops_amd.engine import run_trajectories
    seeds, depths = R.shared_seeds()
    if n == 0:
        got = run_trajectories(case.dm, case.f0, case.f1, _cfg(RELOCATE), np.zeros((0, 3)))
        assert got["points"].shape == (0, R.DURATION // R.RECORD_T + 1, 3)
        return
    shared = case.ref("shared", True, seeds, depths)
    sel = np.flatnonzero((shared["relocations"] > 0) & (shared["death"] < 0))[:1]  # a live particle that relocates
    assert len(sel) == 1
    rel, _ = _check(case, "one", seeds[sel], depths[sel])
    assert int(rel["relocations"].sum()) >= 1


def _orig(ps, t):  # [.., slot] -> [.., particle]
    import torch
    out = torch.empty_like(t)
    out[..., ps.ids.long()] = t
    return out.cpu().numpy()


def _set(case, ref, method=RELOCATE):
    from mops_amd.engine import ParticleSet
    return ParticleSet(case.dm, ref["seeds"], ref["depths"], _cfg(method), cells=ref["cells"])


def _same_state(a, b):
    for k in ("records", "x", "y", "z", "depth", "death", "cell"):
        assert _orig(a, getattr(a, k)).tobytes() == _orig(b, getattr(b, k)).tobytes(), k


def test_split_launches(case):
    """advance over [0, 13) then [13, 36) -- 13 is no record step -- equals one launch, with and without a reorder
    between the two, and so does advance_pipelined (with and without its compaction); the lines are the
    restatement's."""
    import torch
    seeds, depths = R.shared_seeds()
    ref = case.ref("shared", True, seeds, depths)
    want = RR.lines(case.O, ref)
    one = _set(case, ref)
    one.advance(case.f0, case.f1, 0, 36)
    fin = one.finalize(pathline=True)
    for k in LINE_KEYS:
        assert fin[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert np.array_equal(_orig(one, one.death), ref["death"])
    for reorder in (False, True):
        two = _set(case, ref)
        two.advance(case.f0, case.f1, 0, 13)
        if reorder:
            two.reorder()
        two.advance(case.f0, case.f1, 13, 36)
        _same_state(two, one)
    cur = torch.cuda.current_stream()
    for compact in (False, True):
        pip = _set(case, ref)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for s in streams:
            s.wait_stream(cur)
        pip.advance_pipelined(case.f0, case.f1, 0, 36, streams, 3, compact=compact)
        for s in streams:
            cur.wait_stream(s)
        torch.cuda.synchronize()
        fin = pip.finalize(pathline=True)
        for k in LINE_KEYS:
            assert fin[k].cpu().numpy().tobytes() == want[k].tobytes(), (compact, k)
        assert np.array_equal(_orig(pip, pip.death), ref["death"])


# ---- chain ---------------------------------------------------------------------------------------------------
GAP = R.DURATION


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
        return PathlineChain(self.dm, snapshot_field_factory(self.dm, lambda i: self.snaps[i]), 3, gap_seconds=GAP)

    def reference(self, follow_last):
        """The restatement pair by pair with the carried lastPoint (MOPSPathline.run's rules, as
        tests/test_attr_chain_gpu.py builds its reference)."""
        if follow_last in self._ref:
            return self._ref[follow_last]
        O = self.O
        acc = {k: [] for k in ("points", "velocity", "temperature", "salinity")}
        last, death = None, None
        depths = np.full(len(self.seeds), 300.0, dtype=np.float32)
        for p in range(2):
            s = self.seeds if (p == 0 or not follow_last) else last
            r = RR.run_case(O, self.mesh, self.derived[p], self.derived[p + 1], s, depths)
            fin = RR.lines(O, r)
            for k in acc:
                acc[k].append(fin[k][:, (0 if p == 0 else 1):])
            last, death = fin["lastPoint"].copy(), r["death"]
        out = {k: np.concatenate(v, 1) for k, v in acc.items()}
        out.update(lastPoint=last, death_step=death)
        self._ref[follow_last] = out
        return out


@pytest.fixture(scope="module")
def chain_setup(gpu, engine_lib, oracle_lib, small_case):
    return _ChainSetup(oracle_lib, small_case[0])


@pytest.mark.parametrize("mode", [dict(), dict(follow_last=False), dict(compact=True), dict(defer_lines=True),
                                  dict(follow_last=False, compact=True, defer_lines=True)],
                         ids=["default", "nofollow", "compact", "defer", "nofollow-compact-defer"])
def test_chain(chain_setup, mode):
    want = chain_setup.reference(mode.get("follow_last", True))
    got = chain_setup.chain().run(chain_setup.seeds, depth=300.0, method=RELOCATE, delta_t=R.DELTA_T,
                                  record_t=R.RECORD_T, **mode)
    assert want["points"].shape == (R.N_SEEDS, 13 + 12, 3)
    for k in LINE_KEYS:
        assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert np.array_equal(got["death_step"].cpu().numpy(), want["death_step"])


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals(case, engine_lib):
    """A streamline and every attribute entry are refused with the method, before any launch."""
    import torch
    from mops_amd import _lib
    from mops_amd.chain import PathlineChain, snapshot_attr_factory, snapshot_field_factory
    from mops_amd.engine import ParticleSet, cell_to_vertex_attr, run_trajectories
    seeds, depths = R.shared_seeds()
    ref = case.ref("shared", True, seeds, depths)
    cfg = _cfg(RELOCATE)
    ps = ParticleSet(case.dm, ref["seeds"], ref["depths"], cfg, cells=ref["cells"], n_attr=1, capture_slots=2)
    att = (cell_to_vertex_attr(case.dm, case.s0.attributes["temperature"]),
           cell_to_vertex_attr(case.dm, case.s1.attributes["temperature"]))
    ps.records.fill_(-7.0)
    ps.attr_records.fill_(-7.0)
    torch.cuda.synchronize()
    before = {k: getattr(ps, k).clone() for k in ("x", "y", "z", "depth", "cell", "death", "records", "attr_records")}
    prt, c = ps.particles(), cfg.ctype()
    fa, ba = (C.c_void_p * 1)(att[0].data_ptr()), (C.c_void_p * 1)(att[1].data_ptr())
    rec, slab = C.c_void_p(ps.records.data_ptr()), C.c_void_p(ps.attr_records.data_ptr())
    m, f0, f1 = case.dm.handle, case.f0.handle, case.f1.handle
    lib = engine_lib
    # a streamline never silently runs as the plain RK4
    assert lib.mops_traj_advance(m, f0, None, C.byref(c), C.byref(prt), 0, 36, rec, ps.rec_stride, None) == \
        _lib.MOPS_ERR_UNSUPPORTED
    assert b"MOPS_RK4_RELOCATE" in lib.mops_last_error()
    with pytest.raises(_lib.MopsError):
        run_trajectories(case.dm, case.f0, None, cfg, ref["seeds"], depths=ref["depths"], cells=ref["cells"])
    # the four attribute entries
    U = _lib.MOPS_ERR_UNSUPPORTED
    assert lib.mops_traj_sample_attrs(m, f0, f1, C.byref(c), C.byref(prt), 0, 1, fa, ba, slab, ps.rec_stride, None) == U
    assert b"MOPS_RK4_RELOCATE" in lib.mops_last_error()
    assert lib.mops_traj_advance_sampled(m, f0, f1, C.byref(c), C.byref(prt), 0, 36, rec, ps.rec_stride, 1, fa, ba, slab,
                                         ps.rec_stride, None) == U
    assert lib.mops_traj_advance_captured(m, f0, f1, C.byref(c), C.byref(prt), 0, 36, rec, ps.rec_stride, 1, fa, ba, slab,
                                          ps.rec_stride, C.c_void_p(ps.capture.data_ptr()), 2, None) == U
    n, P = R.N_SEEDS, R.DURATION // R.RECORD_T + 1
    hp = np.full((n, P, 3), -7.0)
    hl = np.full((1, n, P), -7.0)
    hs, hd = np.ascontiguousarray(ref["seeds"]), np.ascontiguousarray(ref["depths"], dtype=np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mops_run_pathline_attrs(m, f0, f1, C.byref(c), n, vp(hs), vp(hd), C.c_float(0), None, vp(hp), None, None,
                                       None, None, None, None, None, 1, fa, ba, vp(hl), None) == U
    assert np.all(hp == -7.0) and np.all(hl == -7.0)
    # Python: ValueError before any launch
    with pytest.raises(ValueError, match="RELOCATE"):
        run_trajectories(case.dm, case.f0, case.f1, cfg, ref["seeds"], attrs={"temperature": att})
    with pytest.raises(ValueError, match="RELOCATE"):
        ps.advance(case.f0, case.f1, 0, 36, attrs=([att[0]], [att[1]]))
    with pytest.raises(ValueError, match="RELOCATE"):
        ps.advance_pipelined(case.f0, case.f1, 0, 36, [torch.cuda.current_stream()], 2, attrs=([att[0]], [att[1]]))
    snaps = [case.s0, case.s1]
    chain = PathlineChain(case.dm, snapshot_field_factory(case.dm, lambda i: snaps[i]), 2, gap_seconds=GAP,
                          make_attrs=snapshot_attr_factory(case.dm, lambda i: snaps[i]))
    with pytest.raises(ValueError, match="RELOCATE"):
        chain.run(ref["seeds"], depth=300.0, method=RELOCATE, delta_t=R.DELTA_T, record_t=R.RECORD_T, attrs=True)
    torch.cuda.synchronize()
    for k, v in before.items():  # nothing was launched: state, records and slab as they were
        assert torch.equal(getattr(ps, k), v), k
    # ... and the same call with a back field runs
    assert lib.mops_traj_advance(m, f0, f1, C.byref(c), C.byref(prt), 0, 36, rec, ps.rec_stride, None) == _lib.MOPS_OK
    torch.cuda.synchronize()
    assert np.array_equal(_orig(ps, ps.death), ref["death"])
