"""GPU: the opt-in attribute channel of pathlines (mops_traj_sample_attrs / _advance_sampled / _finalize_attrs /
mops_run_pathline_attrs through engine.py) against the Python restatement of the reference's loop
(tests/pathline_attr_reference.py, pinned to the oracle by tests/test_attr_reference_cpu.py).  Every parity
assertion is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import pathline_attr_reference as R

pytestmark = pytest.mark.gpu

K = R.DURATION // R.RECORD_T
NAMES = ["salinity", "temperature"]  # std::map order
UNSAMPLED = ("points", "velocity", "lastPoint", "death_step", "final_depth", "final_pos", "cells")


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

    def ref(self, euler, backward, seeds=None, depths=None):
        """The restatement, computed once per case and shared (never modified)."""
        key = (euler, backward)
        if key not in self._ref:
            self._ref[key] = R.run_shared(self.O, self.mesh, self.r0, self.r1, euler, backward, seeds, depths)
        return self._ref[key]

    def cfg(self, euler, backward):
        from mops_amd.engine import TrajectoryConfig
        return TrajectoryConfig(deltaT=R.DELTA_T, simulationDuration=R.DURATION, recordT=R.RECORD_T, depth=0.0,
                                direction=1 if backward else 0, method=1 if euler else 0)


@pytest.fixture(scope="module")
def case(gpu, engine_lib, oracle_lib, small_case):
    return _Case(oracle_lib, *small_case)


def _check_parity(c, euler, backward, seeds=None, depths=None):
    from mops_amd.engine import run_trajectories
    ref = c.ref(euler, backward, seeds, depths)
    cfg = c.cfg(euler, backward)
    got = run_trajectories(c.dm, c.f0, c.f1, cfg, ref["seeds"], depths=ref["depths"], cells=ref["cells"], attrs=c.attrs)
    plain = run_trajectories(c.dm, c.f0, c.f1, cfg, ref["seeds"], depths=ref["depths"], cells=ref["cells"])
    want = R.attr_lines(c.O, ref["seeds"], ref, K)
    assert list(got["attributes"]) == NAMES
    for a, name in enumerate(NAMES):
        assert np.array_equal(got["attributes"][name], want[a]), name
        assert np.array_equal(got[name], want[a]), name            # temperature / salinity by name
    alive = ref["death"] < 0
    assert alive.any() and np.all(got["attributes"]["temperature"][alive, :K] != 0.0)
    # the restatement is the run the engine made, and sampling changed nothing else
    assert np.array_equal(got["death_step"], ref["death"])
    for k in UNSAMPLED:
        assert got[k].tobytes() == plain[k].tobytes(), k
    # option off: quirk Q9 as before
    assert np.array_equal(plain["temperature"], plain["velocity"][:, :, 0])
    assert np.array_equal(plain["salinity"], plain["velocity"][:, :, 1])
    assert "attributes" not in plain
    return ref


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_attr_parity(case, euler, backward):
    ref = _check_parity(case, euler, backward)
    death = ref["death"]
    if not euler:  # a death before the first record keeps the step-0 pre-write in slot 0
        assert int(((death >= 1) & (death < R.RECORD_T // R.DELTA_T)).sum()) >= 1


def test_attr_parity_zlevel(gpu, engine_lib, oracle_lib, small_case):
    from mops_amd import synth
    mesh = small_case[0]
    s0 = synth.make_snapshot(mesh, timestep=0, phase=0.0, topography="zlevel")
    s1 = synth.make_snapshot(mesh, timestep=1, phase=0.35, topography="zlevel")
    _check_parity(_Case(oracle_lib, mesh, s0, s1), False, False)


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_attr_parity_wide_stencil(gpu, engine_lib, oracle_lib, euler):
    """maxEdges 10 selects the MAXV 12 sampling kernels (the polygon from the per-cell array, not by rank)."""
    from mops_amd import synth
    mesh = synth.make_mesh(16, n_levels=10, max_edges=10)
    s0 = synth.make_snapshot(mesh, timestep=0)
    s1 = synth.make_snapshot(mesh, timestep=1, phase=0.35)
    seeds = synth.uniform_band_seeds(32, seed=41)
    depths = np.random.default_rng(3).uniform(5, 1500, 32).astype(np.float32)
    _check_parity(_Case(oracle_lib, mesh, s0, s1), euler, False, seeds, depths)


def test_one_attribute_and_names(case):
    """One attribute is enough; temperature / salinity follow the NAME, zeros where it is not sampled."""
    from mops_amd.engine import run_trajectories
    ref = case.ref(True, False)
    want = R.attr_lines(case.O, ref["seeds"], ref, K)
    got = run_trajectories(case.dm, case.f0, case.f1, case.cfg(True, False), ref["seeds"], depths=ref["depths"],
                           cells=ref["cells"], attrs={"salinity": case.attrs["salinity"]})
    assert np.array_equal(got["salinity"], want[0]) and not got["temperature"].any()
    got = run_trajectories(case.dm, case.f0, case.f1, case.cfg(True, False), ref["seeds"], depths=ref["depths"],
                           cells=ref["cells"], attrs={"theta": case.attrs["temperature"]})
    assert np.array_equal(got["attributes"]["theta"], want[1])
    assert not got["temperature"].any() and not got["salinity"].any()
    with pytest.raises(ValueError):
        run_trajectories(case.dm, case.f0, case.f1, case.cfg(True, False), ref["seeds"], attrs={})


def _particle_set(case, euler, n_attr=2):
    from mops_amd.engine import ParticleSet
    ref = case.ref(euler, False)
    return ref, ParticleSet(case.dm, ref["seeds"], ref["depths"], case.cfg(euler, False), cells=ref["cells"],
                            n_attr=n_attr)


@pytest.mark.parametrize("euler", [True, False], ids=["euler", "rk4"])
def test_particle_set_chunks_and_reorder(case, euler):
    """advance in 7-step chunks -- chunks that start on (14, 35), end on (20, 35) and straddle sample steps --
    with a reorder between them gives the slab, records and lines of one call."""
    import torch
    lists = ([case.attrs[k][0] for k in NAMES], [case.attrs[k][1] for k in NAMES])
    ref, one = _particle_set(case, euler)
    one.advance(case.f0, case.f1, 0, 36, attrs=lists)
    _, seg = _particle_set(case, euler)
    for b in range(0, 36, 7):
        seg.advance(case.f0, case.f1, b, min(b + 7, 36), attrs=lists)
        seg.reorder()
    torch.cuda.synchronize()

    def orig(ps, t):  # [.., slot] -> [.., particle]
        out = torch.empty_like(t)
        out[..., ps.ids.long()] = t
        return out.cpu().numpy()
    slab = orig(one, one.attr_records)
    assert np.array_equal(slab, np.ascontiguousarray(ref["rec_attr"].transpose(1, 2, 0)))  # [K][n_attr][n]
    assert orig(seg, seg.attr_records).tobytes() == slab.tobytes()
    assert orig(seg, seg.records).tobytes() == orig(one, one.records).tobytes()
    for k in ("x", "y", "z", "depth", "death"):
        assert orig(seg, getattr(seg, k)).tobytes() == orig(one, getattr(one, k)).tobytes(), k
    want = R.attr_lines(case.O, ref["seeds"], ref, K)
    for ps in (one, seg):
        fin = ps.finalize(pathline=True)
        assert np.array_equal(fin["attributes"].cpu().numpy(), want)
    part = {k: torch.empty_like(v[:40]) for k, v in fin.items() if k not in ("lastPoint", "attributes")}
    one.finalize_range(8, 48, part, pathline=True)
    ids = one.ids[8:48].long().cpu().numpy()
    assert np.array_equal(part["attributes"].cpu().numpy(), want[:, ids])


def test_compact_and_pipelined_refuse_a_slab(case):
    import torch
    _, ps = _particle_set(case, True)
    s = torch.cuda.current_stream()
    with pytest.raises(ValueError, match="attribute slab"):
        ps.compact(0, ps.n, s, records_written=1)
    with pytest.raises(ValueError, match="attribute slab"):
        ps.advance_pipelined(case.f0, case.f1, 0, 36, [s], 2)
    with pytest.raises(ValueError, match="n_attr"):
        _particle_set(case, True, n_attr=0)[1].advance(case.f0, case.f1, 0, 36, attrs=([], []))


@pytest.mark.parametrize("K_", [5, 30], ids=["K5", "K30"])  # both sides of the line assembly's one-pass limit
def test_finalize_attrs_hand_made(gpu, engine_lib, oracle_lib, K_):
    import torch
    from mops_amd import _lib
    n, na = 70, 2
    rng = np.random.default_rng(17 + K_)
    seeds = rng.normal(size=(n, 3))
    rec = rng.normal(size=(K_, 6, n))
    slab = rng.normal(size=(K_, na, n))
    seeds[3, 1] = np.inf                # a non-finite seed: every entry becomes entry 0
    rec[0, 0, 10] = np.nan              # record 0: entries 1.. become entry 0
    rec[K_ // 2, 2, 20] = np.nan        # the middle
    rec[K_ - 1, 1, 33] = -np.inf        # the last record: only the appended entry changes
    rec[1, 0, 65] = np.nan              # a slot of the last, partial block
    line = rng.permutation(n).astype(np.int32)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=gpu)
    d_seeds, d_rec, d_slab, d_line = d(seeds), d(rec), d(slab), d(line)
    out = torch.full((na, n, K_ + 1), -7.0, dtype=torch.float64, device=gpu)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(engine_lib.mops_traj_finalize_attrs(n, K_, p(d_seeds), p(d_rec), n, na, p(d_slab), n, p(d_line), p(out),
                                                   None), "mops_traj_finalize_attrs")
    got = out.cpu().numpy()
    ref = dict(rec_pos=np.ascontiguousarray(rec[:, 0:3, :].transpose(2, 0, 1)),
               rec_attr=np.ascontiguousarray(slab.transpose(2, 0, 1)))
    want = R.attr_lines(oracle_lib, seeds, ref, K_)
    assert np.array_equal(got[:, line], want)
    ident = torch.empty_like(out)
    _lib.check(engine_lib.mops_traj_finalize_attrs(n, K_, p(d_seeds), p(d_rec), n, na, p(d_slab), n, None, p(ident),
                                                   None), "mops_traj_finalize_attrs")
    assert np.array_equal(ident.cpu().numpy(), want)
    assert np.all(want[:, 3] == want[:, 3, :1]) and np.all(want[:, 10] == want[:, 10, :1])  # the cases bite
    assert np.all(want[:, 33, K_] == want[:, 33, K_ - 1]) and np.all(want[:, 0, K_] == 0.0)


def test_argument_checks_with_real_handles(case, engine_lib):
    from mops_amd import _lib
    _, ps = _particle_set(case, True)
    prt, cfg = ps.particles(), ps.cfg.ctype()
    fa = (C.c_void_p * 4)(*[case.attrs["salinity"][0].data_ptr()] * 4)
    ba = (C.c_void_p * 4)(*[case.attrs["salinity"][1].data_ptr()] * 4)
    before = ps.attr_records.clone()

    def call(step, n_attr, back=case.f1.handle, stride=ps.rec_stride):
        return engine_lib.mops_traj_sample_attrs(case.dm.handle, case.f0.handle, back, C.byref(cfg), C.byref(prt), step,
                                                 n_attr, fa, ba, C.c_void_p(ps.attr_records.data_ptr()), stride, None)
    assert call(0, 0) == _lib.MOPS_ERR_INVALID
    assert call(0, 5) == _lib.MOPS_ERR_INVALID
    assert call(1, 2) == _lib.MOPS_ERR_INVALID and b"sample step" in engine_lib.mops_last_error()
    assert call(36, 2) == _lib.MOPS_ERR_INVALID          # past the run
    assert call(0, 2, stride=ps.n - 1) == _lib.MOPS_ERR_INVALID
    assert call(0, 2, back=None) == _lib.MOPS_ERR_UNSUPPORTED
    assert np.array_equal(ps.attr_records.cpu().numpy(), before.cpu().numpy())  # refused before any device work
    assert call(0, 2) == _lib.MOPS_OK and call(2, 2) == _lib.MOPS_OK
