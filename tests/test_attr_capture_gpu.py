"""GPU: the capture path of the attribute channel (mops_traj_advance_captured through ParticleSet): the
trajectory launch stores the step-start state of its interior sample steps and one batched kernel samples them
afterwards.  Its attribute slab, records and particle state must be the split path's (mops_traj_advance_sampled,
pinned to the Python restatement by tests/test_attr_sampling_gpu.py) byte for byte, for every window size."""
import ctypes as C

import numpy as np
import pytest

import pathline_attr_reference as R

pytestmark = pytest.mark.gpu

K = R.DURATION // R.RECORD_T
NAMES = ["salinity", "temperature"]  # std::map order
STATE = ("x", "y", "z", "depth", "cell", "death")


class _Case:
    """A mesh and a snapshot pair on the device and in the oracle, with the attributes' vertex arrays."""

    def __init__(self, O, mesh, s0, s1):
        from mops_amd.engine import DeviceField, DeviceMesh, cell_to_vertex_attr
        self.O, self.mesh = O, mesh
        self.dm = DeviceMesh.from_mesh(mesh)
        self.f0, self.f1 = DeviceField.from_snapshot(self.dm, s0), DeviceField.from_snapshot(self.dm, s1)
        self.r0, self.r1 = O.preprocess(mesh, s0), O.preprocess(mesh, s1)
        self.attrs = {k: (cell_to_vertex_attr(self.dm, s0.attributes[k]), cell_to_vertex_attr(self.dm, s1.attributes[k]))
                      for k in NAMES}
        self._ref = {}

    def lists(self, names=NAMES):
        return [self.attrs[k][0] for k in names], [self.attrs[k][1] for k in names]

    def ref(self, euler, backward):
        """The restatement, computed once per case and shared (never modified)."""
        key = (euler, backward)
        if key not in self._ref:
            self._ref[key] = R.run_shared(self.O, self.mesh, self.r0, self.r1, euler, backward)
        return self._ref[key]


@pytest.fixture(scope="module")
def case(gpu, engine_lib, oracle_lib, small_case):
    return _Case(oracle_lib, *small_case)


def _cfg(euler, backward=False, delta_t=R.DELTA_T, duration=R.DURATION, record_t=R.RECORD_T):
    from mops_amd.engine import TrajectoryConfig
    return TrajectoryConfig(deltaT=delta_t, simulationDuration=duration, recordT=record_t, depth=0.0,
                            direction=1 if backward else 0, method=1 if euler else 0)


def _snapshot(ps):
    """Slab, records and state of a particle set in the particles' seed order, as host arrays."""
    import torch
    torch.cuda.synchronize()
    ids = ps.ids.long()

    def orig(t):  # [.., slot] -> [.., particle]
        out = torch.empty_like(t)
        out[..., ids] = t
        return out.cpu().numpy()
    out = {k: orig(getattr(ps, k)) for k in STATE}
    out["records"] = orig(ps.records)
    if ps.attr_records is not None:
        out["slab"] = orig(ps.attr_records)
    return out


def _run(c, cfg, seeds, depths, cells, W, names=NAMES, ranges=None, reorder=False, expect_tile=False):
    """One run over the step ranges (default: one call).  W None: the plain advance without a slab; W 0: the
    split path; W > 0: the capture path with a window of W slots.  ``expect_tile``: every trajectory launch of
    every call must have selected the tile kernels (DeviceMesh.tile_selection)."""
    from mops_amd.engine import ParticleSet
    ps = ParticleSet(c.dm, seeds, depths, cfg, cells=cells, n_attr=0 if W is None else len(names),
                     capture_slots=W or 0)
    lists = None if W is None else c.lists(names)
    for b, e in ranges or [(0, cfg.n_steps)]:
        _, count = c.dm.tile_selection()
        ps.advance(c.f0, c.f1, b, e, attrs=lists)
        if expect_tile:
            flag, after = c.dm.tile_selection()
            assert after > count and flag == 1, (W, flag, after - count)
        if reorder:
            ps.reorder()
    return _snapshot(ps)


def _same(got, want, keys, what):
    for k in keys:
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_capture_equals_restatement_and_split(case, euler, backward):
    ref = case.ref(euler, backward)
    cfg = _cfg(euler, backward)
    args = (case, cfg, ref["seeds"], ref["depths"], ref["cells"])
    plain, split = _run(*args, None), _run(*args, 0)
    want = np.ascontiguousarray(ref["rec_attr"].transpose(1, 2, 0))  # [K][n_attr][n]
    assert np.array_equal(split["slab"], want)
    assert np.array_equal(plain["death"], ref["death"])
    if not euler:  # a death before the first record keeps the step-0 pre-write in slot 0
        early = (ref["death"] >= 1) & (ref["death"] < R.RECORD_T // R.DELTA_T)
        assert int(early.sum()) >= 1 and np.all(want[0][:, early] != 0.0)
    for W in (1, 5, 12):
        got = _run(*args, W)
        assert np.array_equal(got["slab"], want), W
        _same(got, split, ("slab", "records") + STATE, f"split W={W}")
        _same(got, plain, ("records",) + STATE, f"plain W={W}")


def _dense_seeds(mesh):
    """The seeding recipe of test_gpu_parity.test_pathline_cooperative_waves (forward variant), restated: 14
    cells x 45+ particles in one or two depth groups, 37 seeds on land."""
    from mops_amd import synth
    rng = np.random.default_rng(41)
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    cells = rng.choice(mesh.nCells, 14, replace=False)
    seeds, depths = [], []
    for j, c in enumerate(cells):
        k = 45 + j  # uneven counts: groups straddle wave boundaries
        u = cc[c] / np.linalg.norm(cc[c])
        jit = rng.normal(size=(k, 3)) * 2.0e4
        p = u + (jit - np.outer(jit @ u, u)) / 6.371e6
        seeds.append(p / np.linalg.norm(p, axis=1, keepdims=True) * 6.37101e6)
        depths.append(np.full(k, 300.0) if j < 7 else np.where(np.arange(k) % 2 == 0, 300.0, 1100.0))
    land = synth.uniform_band_seeds(400, seed=3)
    seeds.append(land[:37]); depths.append(np.full(37, 500.0))
    return np.concatenate(seeds), np.concatenate(depths).astype(np.float32)


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_dense_seeds_tile_kernels(case, euler):
    """The case of this file whose waves take the cooperative tile, the RK4 hand-off and the resumed kernel, in their
    plain and their capture instantiations (every launch is asserted to have selected the tile): the split path is
    the reference (the Python restatement is too slow at 360 steps x 800 particles)."""
    seeds, depths = _dense_seeds(case.mesh)
    assert len(seeds) % 64 != 0
    cfg = _cfg(euler, delta_t=120, duration=43200, record_t=3600)
    assert cfg.n_records == 12
    args = (case, cfg, seeds, depths, None)
    split = _run(*args, 0, expect_tile=True)
    assert (split["death"] >= 0).any() and (split["death"] < 0).any()
    alive = split["death"] < 0
    assert np.all(split["slab"][:, 1, alive] != 0.0)  # every slot of a live particle was sampled
    for W in (12, 3):
        _same(_run(*args, W, expect_tile=True), split, ("slab", "records") + STATE, f"W={W}")


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_chunks_with_reorder(case, euler):
    """7-step chunks -- starting on, ending on and straddling sample steps -- with a reorder between them."""
    ref = case.ref(euler, False)
    args = (case, _cfg(euler), ref["seeds"], ref["depths"], ref["cells"])
    one = _run(*args, 2)
    seg = _run(*args, 2, ranges=[(b, min(b + 7, 36)) for b in range(0, 36, 7)], reorder=True)
    _same(seg, one, ("slab", "records") + STATE, "chunks")
    assert np.array_equal(one["slab"], np.ascontiguousarray(ref["rec_attr"].transpose(1, 2, 0)))


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_record_every_step(case, euler):
    """ri == 1: every step is a sample step and step 0 is both the pre-write and record 0."""
    ref = case.ref(euler, False)
    cfg = _cfg(euler, delta_t=R.RECORD_T, duration=12 * R.RECORD_T, record_t=R.RECORD_T)
    assert cfg.n_steps == 12 and cfg.n_records == 12
    args = (case, cfg, ref["seeds"], ref["depths"], ref["cells"])
    split = _run(*args, 0)
    assert split["slab"][0].any()
    for W in (1, 5, 12):
        _same(_run(*args, W), split, ("slab", "records") + STATE, f"W={W}")
    _same(_run(*args, 4, ranges=[(0, 5), (5, 6), (6, 12)]), split, ("slab", "records") + STATE, "ranges")


def test_wide_stencil_takes_the_split_path(gpu, engine_lib, oracle_lib):
    """maxEdges 10 (MAXV 12) has no capture instantiation: the entry samples between launches, same results."""
    from mops_amd import synth
    mesh = synth.make_mesh(16, n_levels=10, max_edges=10)
    c = _Case(oracle_lib, mesh, synth.make_snapshot(mesh, timestep=0), synth.make_snapshot(mesh, timestep=1, phase=0.35))
    seeds = synth.uniform_band_seeds(32, seed=41)
    depths = np.random.default_rng(3).uniform(5, 1500, 32).astype(np.float32)
    for euler in (True, False):
        args = (c, _cfg(euler), seeds, depths, None)
        split = _run(*args, 0)
        assert split["slab"].any()
        _same(_run(*args, 5), split, ("slab", "records") + STATE, "maxv 12")


@pytest.mark.parametrize("names", [["temperature"], ["salinity", "temperature", "temperature", "salinity"]],
                         ids=["one", "four"])
def test_attribute_counts(case, names):
    ref = case.ref(True, False)
    args = (case, _cfg(True), ref["seeds"], ref["depths"], ref["cells"])
    split = _run(*args, 0, names=names)
    got = _run(*args, 5, names=names)
    _same(got, split, ("slab", "records") + STATE, "n_attr")
    want = ref["rec_attr"].transpose(1, 2, 0)
    for a, name in enumerate(names):
        assert np.array_equal(got["slab"][:, a], want[:, NAMES.index(name)])


@pytest.mark.parametrize("W", [0, 5], ids=["split", "capture"])
def test_compact_halfway(case, W):
    """RK4 (particles die at cell crossings): a compaction at step 18 moves the 7 slots written so far."""
    import torch
    from mops_amd.engine import ParticleSet
    ref = case.ref(False, False)
    cfg = _cfg(False)
    want = _run(case, cfg, ref["seeds"], ref["depths"], ref["cells"], W)
    assert (want["death"] >= 0).any() and (want["death"] < 0).any()
    ps = ParticleSet(case.dm, ref["seeds"], ref["depths"], cfg, cells=ref["cells"], n_attr=2, capture_slots=W)
    ps.advance(case.f0, case.f1, 0, 18, attrs=case.lists())
    nrec = min(ps.K, 18 // ps.record_period(pathline=True) + 1)
    assert nrec == 7
    live = ps.compact(0, ps.n, torch.cuda.current_stream(), records_written=nrec, attr_slots_written=nrec)
    ps.advance(case.f0, case.f1, 18, 36, live_count=live, attrs=case.lists())
    got = _snapshot(ps)
    assert 0 < int(live.item()) < ps.n
    _same(got, want, ("slab", "records") + STATE, "compact")


@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
@pytest.mark.parametrize("W", [0, 5], ids=["split", "capture"])
def test_pipelined_equals_one_call(case, W, compact):
    """2 particle parts (64 + 32 slots) on their own streams x 3 step chunks of 12."""
    import torch
    from mops_amd.engine import ParticleSet
    ref = case.ref(False, False)
    cfg = _cfg(False)
    want = _run(case, cfg, ref["seeds"], ref["depths"], ref["cells"], W)
    ps = ParticleSet(case.dm, ref["seeds"], ref["depths"], cfg, cells=ref["cells"], n_attr=2, capture_slots=W)
    cur = torch.cuda.current_stream()
    parts = [torch.cuda.Stream(), torch.cuda.Stream()]
    for st in parts:
        st.wait_stream(cur)
    ps.advance_pipelined(case.f0, case.f1, 0, 36, parts, 3, compact=compact, attrs=case.lists())
    for st in parts:
        cur.wait_stream(st)
    _same(_snapshot(ps), want, ("slab", "records") + STATE, "pipelined")


def test_argument_checks_with_real_handles(case, engine_lib):
    from mops_amd import _lib
    from mops_amd.engine import ParticleSet
    ref = case.ref(True, False)
    ps = ParticleSet(case.dm, ref["seeds"], ref["depths"], _cfg(True), cells=ref["cells"], n_attr=2, capture_slots=4)
    prt, cfg = ps.particles(), ps.cfg.ctype()
    fa = (C.c_void_p * 2)(*[t.data_ptr() for t in case.lists()[0]])
    ba = (C.c_void_p * 2)(*[t.data_ptr() for t in case.lists()[1]])
    ps.attr_records.fill_(-3.0)
    before = ps.attr_records.clone()
    rec_before = ps.records.clone()

    def call(back=case.f1.handle, stride=ps.rec_stride, cap=ps.capture.data_ptr(), slots=4):
        return engine_lib.mops_traj_advance_captured(
            case.dm.handle, case.f0.handle, back, C.byref(cfg), C.byref(prt), 0, 36, C.c_void_p(ps.records.data_ptr()),
            ps.rec_stride, 2, fa, ba, C.c_void_p(ps.attr_records.data_ptr()), stride, C.c_void_p(cap), slots, None)
    assert call(cap=None) == _lib.MOPS_ERR_INVALID and b"capture" in engine_lib.mops_last_error()
    assert call(slots=-1) == _lib.MOPS_ERR_INVALID
    assert call(stride=ps.n - 1) == _lib.MOPS_ERR_INVALID
    assert call(back=None) == _lib.MOPS_ERR_UNSUPPORTED
    import torch
    torch.cuda.synchronize()
    assert torch.equal(ps.attr_records, before) and torch.equal(ps.records, rec_before)  # refused before device work
    with pytest.raises(ValueError):
        ParticleSet(case.dm, ref["seeds"], ref["depths"], _cfg(True), cells=ref["cells"], capture_slots=4)
