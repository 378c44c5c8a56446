"""GPU: fixed-layer streamlines and pathlines (mops_traj_advance_layer, traj_lane_kernel; the slice kernel behind
mops_field_layer_velocity) against the Python restatement of the layer step (tests/layer_reference.py, pinned to the
oracle by tests/test_layer_cpu.py).  Lines are built from the restatement's records by the oracle's own assembly.
Every parity assertion is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import layer_reference as LR
import pathline_attr_reference as R

pytestmark = pytest.mark.gpu

EULER, RK4, RELOCATE = 1, 0, 2
METHODS = {"euler": EULER, "rk4": RK4, "rk4_relocate": RELOCATE}
LINE_KEYS = ("points", "velocity", "temperature", "salinity", "lastPoint")
RAW_KEYS = ("layerThickness", "bottomDepth", "zonalVelocity", "meridionalVelocity", "vertVelocityTop")
N_STEPS = R.DURATION // R.DELTA_T  # 36
K = R.DURATION // R.RECORD_T       # 12


def _host(t):
    return t.cpu().numpy()


def _cfg(method, layer, backward=False, delta_t=R.DELTA_T, duration=R.DURATION, record_t=R.RECORD_T):
    from mops_amd.engine import TrajectoryConfig
    return TrajectoryConfig(deltaT=delta_t, simulationDuration=duration, recordT=record_t, depth=0.0,
                            direction=1 if backward else 0, method=method, layer=layer)


class _Case:
    """A mesh and a snapshot pair in the oracle and on the device, the fields made by each of the three paths;
    restatement runs are computed once per key and never modified."""

    def __init__(self, O, mesh, s0, s1):
        from mops_amd.engine import DeviceMesh
        self.O, self.mesh, self.snaps = O, mesh, (s0, s1)
        self.L = mesh.nVertLevels
        self.dm = DeviceMesh.from_mesh(mesh)
        self.r = (O.preprocess(mesh, s0), O.preprocess(mesh, s1))
        self._fields, self._ref = {}, {}

    def fields(self, path="snapshot"):
        if path not in self._fields:
            import torch
            from mops_amd.engine import DeviceField
            out = []
            for i, (s, r) in enumerate(zip(self.snaps, self.r)):
                if path == "snapshot":
                    out.append(DeviceField.from_snapshot(self.dm, s))
                elif path == "device":  # the fused derivation: the slice kernel reads the level-pair records
                    raw = {k: torch.as_tensor(getattr(s, k), device="cuda") for k in RAW_KEYS}
                    torch.cuda.synchronize()
                    out.append(DeviceField.from_device_snapshot(self.dm, raw, timestep=i))
                else:
                    out.append(DeviceField.from_derived(self.dm, r.vertex_ztop, r.vertex_vel, r.vertex_w))
            self._fields[path] = tuple(out)
        return self._fields[path]

    def ref(self, layer, pathline, method, backward=False, seeds=None, depths=None, key="shared", **times):
        k = (key, layer, pathline, method, backward)
        if k not in self._ref:
            if seeds is None:
                seeds, depths = R.shared_seeds()
            self._ref[k] = LR.run_case(self.O, self.mesh, self.r[0], self.r[1] if pathline else None, seeds, depths,
                                       layer, euler=method == EULER, backward=backward,
                                       relocate=method == RELOCATE, **times)
        return self._ref[k]


@pytest.fixture(scope="module")
def case(gpu, engine_lib, oracle_lib, small_case):
    return _Case(oracle_lib, *small_case)


def _check(c, ref, layer, pathline, method, backward=False, path="snapshot", **times):
    """run_trajectories in layer mode equals the restatement: lines, deaths, final positions, unchanged depths."""
    from mops_amd.engine import run_trajectories
    f0, f1 = c.fields(path)
    got = run_trajectories(c.dm, f0, f1 if pathline else None, _cfg(method, layer, backward, **times), ref["seeds"],
                           depths=ref["depths"], cells=ref["cells"])
    want = LR.lines(c.O, ref, pathline)
    what = (layer, pathline, method, backward, path)
    assert np.array_equal(got["death_step"], ref["death"]), what
    for k in LINE_KEYS:
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    assert got["final_pos"].tobytes() == ref["final_pos"].tobytes(), what
    assert got["final_depth"].tobytes() == ref["final_depth"].tobytes(), what
    assert got["final_depth"].tobytes() == np.asarray(ref["depths"], dtype=np.float32).tobytes(), what  # w = 0
    return got


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("method", list(METHODS), ids=list(METHODS))
@pytest.mark.parametrize("pathline", [False, True], ids=["streamline", "pathline"])
@pytest.mark.parametrize("k", [0, 4, -1], ids=["k0", "k4", "kLast"])
def test_parity_shared(case, k, pathline, method, backward):
    layer = k % case.L
    m = METHODS[method]
    ref = case.ref(layer, pathline, m, backward)
    _check(case, ref, layer, pathline, m, backward)
    alive = int((ref["death"] < 0).sum())
    print(f"layer {layer} {'pathline' if pathline else 'streamline'} {method} backward={backward}: alive {alive}, "
          f"relocations {int(ref['relocations'].sum())}")
    assert alive >= 20
    if m == RELOCATE:  # (the deepest layer is slow: few stage points leave their cell there)
        assert int(ref["relocations"].sum()) >= 1
        assert alive > int((case.ref(layer, pathline, RK4, backward)["death"] < 0).sum())


@pytest.mark.parametrize("path", ["device", "derived"])
@pytest.mark.parametrize("k", [0, 4, -1], ids=["k0", "k4", "kLast"])
def test_field_paths(case, k, path):
    """The slice kernel reads cellVertexVelocity (from_snapshot, from_derived) or the level-pair records (the fused
    derivation of from_device_snapshot; the last level from the second half of record L - 2): the same slice
    bytes, and the same lines."""
    import torch
    layer = k % case.L
    base = [_host(f.layer_velocity(layer).clone()) for f in case.fields("snapshot")]
    mine = [_host(f.layer_velocity(layer).clone()) for f in case.fields(path)]
    torch.cuda.synchronize()
    for a, b in zip(base, mine):
        assert a.size == case.mesh.nVertices * 4 and np.abs(a).sum() > 0
        assert a.tobytes() == b.tobytes()
    # the slice holds the oracle's vertex velocities of that layer (the engine's own vertex order: as sorted rows)
    want = np.asarray(case.r[0].vertex_vel).reshape(case.mesh.nVertices, case.L, 3)[:, layer, :]
    rows = base[0].reshape(-1, 4)
    assert not rows[:, 3].any()
    assert np.array_equal(np.sort(rows[:, :3].view("f8,f8,f8"), axis=0), np.sort(want.copy().view("f8,f8,f8"), axis=0))
    for pathline, m in ((False, EULER), (True, RK4), (True, RELOCATE)):
        _check(case, case.ref(layer, pathline, m), layer, pathline, m, path=path)


def _zlevel_snapshots(mesh, mask_dry):
    """The z-level world's snapshot pair; ``mask_dry``: the cell velocities of the levels below the sea floor (zero
    thickness) set to zero, as MPAS-O writes them -- mops_amd.synth leaves its analytic velocity there."""
    from mops_amd import synth
    out = []
    for t, phase in ((0, 0.0), (1, 0.35)):
        s = synth.make_snapshot(mesh, timestep=t, phase=phase, topography="zlevel")
        if mask_dry:
            dry = np.asarray(s.layerThickness).reshape(mesh.nCells, -1) == 0.0
            assert dry[:, -1].sum() > 100 and not dry[:, 0].any()
            for k in ("zonalVelocity", "meridionalVelocity"):
                a = np.asarray(getattr(s, k))
                v = a.reshape(mesh.nCells, -1).copy()
                v[dry] = 0.0
                setattr(s, k, v.reshape(a.shape))
        out.append(s)
    return out


@pytest.mark.parametrize("mask_dry", [False, True], ids=["synth", "dry-masked"])
def test_zlevel_deep_layer(gpu, engine_lib, oracle_lib, small_case, mask_dry):
    """The z-level world (small_z) at its deepest layer.  With the velocities below the sea floor zero
    (``dry-masked``) the zero-velocity rule fires: 27 of the 96 shared seeds start over dry cells and die at step 0.
    It does not fire after step 0 on these inputs, in either direction or at four times the step: the vertex
    interpolation lets the velocity go to zero continuously towards a dry cell, so a particle slows down before it
    and never enters.  The count is printed."""
    mesh = small_case[0]
    s0, s1 = _zlevel_snapshots(mesh, mask_dry)
    c = _Case(oracle_lib, mesh, s0, s1)
    layer = c.L - 1
    total = late = 0
    for pathline, m in ((False, EULER), (True, EULER), (True, RELOCATE), (False, RK4)):
        ref = c.ref(layer, pathline, m, key="zlevel")
        _check(c, ref, layer, pathline, m)
        _check(c, ref, layer, pathline, m, path="device")
        total += int(ref["zero_killed"].sum())
        late += int((ref["zero_killed"] & (ref["death"] > 0)).sum())
        print(f"zlevel mask_dry={mask_dry} layer {layer} pathline={pathline} method={m}: killed by the zero-velocity "
              f"rule {int(ref['zero_killed'].sum())} (after step 0: "
              f"{int((ref['zero_killed'] & (ref['death'] > 0)).sum())}), alive {int((ref['death'] < 0).sum())}")
        assert int((ref["death"] < 0).sum()) >= 20
    if mask_dry:
        assert total >= 4 * 20
    else:
        assert total == 0


def test_zero_velocity_rule_mid_run(gpu, engine_lib, oracle_lib):
    """The zero-velocity rule firing after step 0, on a constructed field.  The vertex interpolation takes the velocity
    to zero continuously towards a cell whose vertices are all zero, so a particle enters one only by a step longer
    than the cell: a 38 642-cell mesh (cells of about 110 km) with four-day steps.  The cells the particles of an
    unmasked Euler run end in get zero velocity at all their vertices; the particles then reach them mid-run -- an
    Euler step, or a located RK4 stage point, lands inside -- and the rule kills them there."""
    from mops_amd import synth
    from mops_amd.engine import DeviceField, DeviceMesh, run_trajectories
    O = oracle_lib
    mesh = synth.make_mesh(64, n_levels=10)
    snaps = [synth.make_snapshot(mesh, timestep=t, phase=0.35 * t) for t in range(2)]
    r = [O.preprocess(mesh, s) for s in snaps]
    seeds = synth.uniform_band_seeds(48, seed=5)
    depths = np.full(len(seeds), 100.0, dtype=np.float32)
    layer, dt = 4, 345600
    times = dict(delta_t=dt, duration=8 * dt, record_t=2 * dt)
    base = LR.run_case(O, mesh, r[0], r[1], seeds, depths, layer, euler=True, **times)
    moved = np.flatnonzero((base["death"] < 0) & (base["final_cell"] != base["cells"]))
    V, L = mesh.nVertices, mesh.nVertLevels
    voc = np.asarray(mesh.verticesOnCell).reshape(mesh.nCells, mesh.maxEdges).astype(np.int64) - 1
    nv = np.asarray(mesh.nEdgesOnCell).reshape(-1).astype(np.int64)
    masked = []
    for d in r:
        vel = np.asarray(d.vertex_vel).reshape(V, L, 3).copy()
        for c in sorted(set(int(base["final_cell"][i]) for i in moved)):
            vel[voc[c, :nv[c]]] = 0.0
        masked.append(O.Derived(d.vertex_ztop, vel.reshape(-1), d.vertex_w))
    dm = DeviceMesh.from_mesh(mesh)
    f = [DeviceField.from_derived(dm, d.vertex_ztop, d.vertex_vel, d.vertex_w) for d in masked]
    late = {}
    for pathline, m in ((True, EULER), (False, RELOCATE)):
        ref = LR.run_case(O, mesh, masked[0], masked[1] if pathline else None, seeds, depths, layer,
                          euler=m == EULER, relocate=m == RELOCATE, cells=base["cells"], **times)
        got = run_trajectories(dm, f[0], f[1] if pathline else None, _cfg(m, layer, **times), seeds, depths=depths,
                               cells=ref["cells"])
        want = LR.lines(O, ref, pathline)
        assert np.array_equal(got["death_step"], ref["death"]), (pathline, m)
        for k in LINE_KEYS:
            assert got[k].tobytes() == want[k].tobytes(), (pathline, m, k)
        late[m] = int((ref["zero_killed"] & (ref["death"] > 0)).sum())
        print(f"pathline={pathline} method={m}: killed by the zero-velocity rule after step 0: {late[m]} at steps "
              f"{sorted(set(ref['death'][ref['zero_killed']].tolist()))}, alive {int((ref['death'] < 0).sum())}")
    assert late[EULER] >= 5 and late[RELOCATE] >= 1


@pytest.mark.parametrize("key", ["me12", "me20"])
def test_wide_stencil(gpu, engine_lib, oracle_lib, key):
    """A MAXV 12 and a MAXV 20 mesh (tests/wide_case.py): seeds inside a wide cell and around the wide cells."""
    import wide_case as W
    mesh, s0, s1 = W.world(key)
    c = _Case(oracle_lib, mesh, s0, s1)
    allseeds = W.seeds(key)
    seeds = np.concatenate([allseeds[128:160], allseeds[384:416]])
    depths = np.full(len(seeds), W.DEPTH, dtype=np.float32)
    nv = W.degrees(mesh)
    for pathline, m in ((False, EULER), (True, EULER), (True, RK4), (False, RELOCATE)):
        dt, duration, record_t = W.times(m == EULER)
        times = dict(delta_t=dt, duration=duration, record_t=record_t)
        ref = c.ref(4, pathline, m, seeds=seeds, depths=depths, key=key, **times)
        _check(c, ref, 4, pathline, m, **times)
        print(f"{key} pathline={pathline} method={m}: alive {int((ref['death'] < 0).sum())}, seeds in cells of more "
              f"than 7 vertices {int((nv[ref['cells']] > 7).sum())}, relocations {int(ref['relocations'].sum())}")
        assert int((nv[ref["cells"]] > 7).sum()) >= 16
        assert int((ref["death"] < 0).sum()) >= 8


@pytest.mark.parametrize("pathline,m", [(False, RK4), (True, RELOCATE)], ids=["stream-rk4", "path-relocate"])
@pytest.mark.parametrize("key", ["me12", "me20"])
def test_wide_stencil_other_forms(gpu, engine_lib, oracle_lib, key, pathline, m):
    """The two forms of the per-lane kernel that test_wide_stencil does not launch at MAXV 12 and 20, on its seeds,
    over 90 steps with a record every 10 (the restatement keeps 63 or 64 of the 64 alive over twice as many)."""
    import wide_case as W
    mesh, s0, s1 = W.world(key)
    c = _Case(oracle_lib, mesh, s0, s1)
    allseeds = W.seeds(key)
    seeds = np.concatenate([allseeds[128:160], allseeds[384:416]])
    depths = np.full(len(seeds), W.DEPTH, dtype=np.float32)
    nv = W.degrees(mesh)
    dt, duration, record_t = W.times(True)
    times = dict(delta_t=dt, duration=duration // 4, record_t=record_t // 3)
    ref = c.ref(4, pathline, m, seeds=seeds, depths=depths, key=key, **times)
    _check(c, ref, 4, pathline, m, **times)
    assert int((nv[ref["cells"]] > 7).sum()) >= 16
    assert int((ref["death"] < 0).sum()) >= 8


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_particle_counts(case, n):
    seeds, depths = R.shared_seeds()
    live = np.flatnonzero(case.ref(4, True, EULER)["death"] < 0)
    sel = np.concatenate([live[:1], np.setdiff1d(np.arange(R.N_SEEDS), live[:1])])[:n]  # a live particle first
    for pathline, m in ((True, EULER), (False, RK4)):
        ref = case.ref(4, pathline, m, seeds=seeds[sel], depths=depths[sel], key=f"n{n}")
        _check(case, ref, 4, pathline, m)
    assert case.ref(4, True, EULER, key=f"n{n}")["death"][0] < 0


def _orig(ps, t):  # [.., slot] -> [.., particle]
    import torch
    out = torch.empty_like(t)
    out[..., ps.ids.long()] = t
    return out.cpu().numpy()


def _set(case, ref, method, layer):
    from mops_amd.engine import ParticleSet
    return ParticleSet(case.dm, ref["seeds"], ref["depths"], _cfg(method, layer), cells=ref["cells"])


def _same_state(a, b):
    for k in ("records", "x", "y", "z", "depth", "death", "cell"):
        assert _orig(a, getattr(a, k)).tobytes() == _orig(b, getattr(b, k)).tobytes(), k


@pytest.mark.parametrize("pathline,method", [(True, EULER), (False, RK4), (True, RELOCATE)],
                         ids=["pathline-euler", "streamline-rk4", "pathline-relocate"])
def test_split_launches(case, pathline, method):
    """Launches split at steps 7 and 20 -- neither a record step -- with a reorder between them equal one launch;
    so does advance_pipelined, with and without its compaction.  Final cells and depths are the restatement's."""
    import torch
    layer = 4
    ref = case.ref(layer, pathline, method)
    want = LR.lines(case.O, ref, pathline)
    f0, f1 = case.fields()
    back = f1 if pathline else None
    one = _set(case, ref, method, layer)
    one.advance(f0, back, 0, N_STEPS)
    fin = one.finalize(pathline=pathline)
    for k in LINE_KEYS:
        assert _host(fin[k]).tobytes() == want[k].tobytes(), k
    assert np.array_equal(_orig(one, one.death), ref["death"])
    assert np.array_equal(_orig(one, one.cell), ref["final_cell"])
    assert _orig(one, one.depth).tobytes() == ref["depths"].tobytes()
    for reorder in (False, True):
        two = _set(case, ref, method, layer)
        two.advance(f0, back, 0, 7)
        if reorder:
            two.reorder()
        two.advance(f0, back, 7, 20)
        if reorder:
            two.reorder()
        two.advance(f0, back, 20, N_STEPS)
        _same_state(two, one)
    cur = torch.cuda.current_stream()
    for compact in (False, True):
        pip = _set(case, ref, method, layer)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for s in streams:
            s.wait_stream(cur)
        pip.advance_pipelined(f0, back, 0, N_STEPS, streams, 3, compact=compact)
        for s in streams:
            cur.wait_stream(s)
        torch.cuda.synchronize()
        fin = pip.finalize(pathline=pathline)
        for k in LINE_KEYS:
            assert _host(fin[k]).tobytes() == want[k].tobytes(), (compact, k)
        assert np.array_equal(_orig(pip, pip.death), ref["death"])


def test_slices_made_on_another_stream(case):
    """Slices written on a side stream (DeviceField.layer_velocity) and launches on other streams -- ``advance`` on
    one, ``advance_pipelined`` on two more -- with no host synchronisation in between: the launches wait for the
    slices' events.  Fresh fields, so nothing is remembered from another test."""
    import torch
    from mops_amd.engine import DeviceField
    layer = 0
    ref = case.ref(layer, True, EULER)
    want = LR.lines(case.O, ref, True)
    f0, f1 = (DeviceField.from_snapshot(case.dm, s) for s in case.snaps)
    torch.cuda.synchronize()
    side, run = torch.cuda.Stream(), torch.cuda.Stream()
    for f in (f0, f1):
        f.layer_velocity(layer, stream=side)
    ps = _set(case, ref, EULER, layer)
    run.wait_stream(torch.cuda.current_stream())
    ps.advance(f0, f1, 0, N_STEPS, stream=run)
    pip = _set(case, ref, EULER, layer)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    pip.advance_pipelined(f0, f1, 0, N_STEPS, streams, 2)
    torch.cuda.synchronize()
    for got in (ps, pip):
        fin = got.finalize(pathline=True)
        for k in LINE_KEYS:
            assert _host(fin[k]).tobytes() == want[k].tobytes(), k
        assert np.array_equal(_orig(got, got.death), ref["death"])


# ---- chain ---------------------------------------------------------------------------------------------------
GAP = R.DURATION
CHAIN_LAYER = 4
CHAIN_DEPTH = 300.0


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

    def chain(self, recycle=False):
        import torch
        from mops_amd.chain import PathlineChain, snapshot_field_factory
        from mops_amd.engine import DeviceField
        if not recycle:
            return PathlineChain(self.dm, snapshot_field_factory(self.dm, lambda i: self.snaps[i]), 3, gap_seconds=GAP)
        s = self

        def raw(i):
            return {k: torch.as_tensor(getattr(s.snaps[i], k), device="cuda") for k in RAW_KEYS}

        class Recycle:  # fields rebuilt in place: snapshot 2 into snapshot 0's buffers
            def __call__(self, i, stream):
                d = raw(i)
                torch.cuda.current_stream().synchronize()
                return DeviceField.from_device_snapshot(s.dm, d, timestep=i, stream=stream)

            def refill(self, field, i, stream):
                d = raw(i)
                stream.wait_stream(torch.cuda.current_stream())
                return field.rebuild_from_device(d, timestep=i, stream=stream.cuda_stream)

        return PathlineChain(self.dm, Recycle(), 3, gap_seconds=GAP, prefetch=False)

    def reference(self, method):
        """The restatement chained by hand: pair by pair with the carried lastPoint (MOPSPathline.run's rules)."""
        if method in self._ref:
            return self._ref[method]
        O = self.O
        acc = {k: [] for k in ("points", "velocity", "temperature", "salinity")}
        recs = []
        last, death = None, None
        depths = np.full(len(self.seeds), CHAIN_DEPTH, dtype=np.float32)
        for p in range(2):
            s = self.seeds if p == 0 else last
            r = LR.run_case(O, self.mesh, self.derived[p], self.derived[p + 1], s, depths, CHAIN_LAYER,
                            euler=method == EULER, relocate=method == RELOCATE)
            fin = LR.lines(O, r, True)
            for k in acc:
                acc[k].append(fin[k][:, (0 if p == 0 else 1):])
            recs.append(r)
            last, death = fin["lastPoint"].copy(), r["death"]
        out = {k: np.concatenate(v, 1) for k, v in acc.items()}
        out.update(lastPoint=last, death_step=death, pairs=recs)
        self._ref[method] = out
        return out


@pytest.fixture(scope="module")
def chain_setup(gpu, engine_lib, oracle_lib, small_case):
    return _ChainSetup(oracle_lib, small_case[0])


@pytest.mark.parametrize("mode", [dict(), dict(defer_lines=True), dict(keep_lines=False), dict(recycle=True),
                                  dict(compact=True, method=RK4)],
                         ids=["default", "defer", "nolines", "recycle", "compact-rk4"])
def test_chain(chain_setup, mode):
    mode = dict(mode)
    method = mode.pop("method", EULER)
    recycle = mode.pop("recycle", False)
    want = chain_setup.reference(method)
    got = chain_setup.chain(recycle).run(chain_setup.seeds, depth=CHAIN_DEPTH, method=method, delta_t=R.DELTA_T,
                                         record_t=R.RECORD_T, layer=CHAIN_LAYER, **mode)
    keys = LINE_KEYS if mode.get("keep_lines", True) else ("lastPoint",)
    if mode.get("keep_lines", True):
        assert want["points"].shape == (R.N_SEEDS, 13 + 12, 3)
    else:
        assert "points" not in got
    for k in keys:
        assert _host(got[k]).tobytes() == want[k].tobytes(), k
    assert np.array_equal(_host(got["death_step"]), want["death_step"])
    assert int((want["death_step"] < 0).sum()) >= 20


def test_chain_density_of_a_layer(chain_setup):
    """A count map of a layer run: bytes-equal to density_reference fed with the restatement's records, under that
    file's own margin pre-check (no sample within EDGE_GUARD pixels of a pixel edge)."""
    import density_reference as D
    from mops_amd.engine import DensityMap
    win = (48, 24, (-90.0, 90.0), (-180.0, 180.0))
    want_run = chain_setup.reference(EULER)
    acc = D.new_accum(win[0], win[1])
    for p, r in enumerate(want_run["pairs"]):
        slab = np.ascontiguousarray(r["rec_pos"].transpose(1, 2, 0))  # [K, 3, n]
        rec = np.zeros((K, 6, R.N_SEEDS))
        rec[:, 0:3, :] = slab
        pts = rec[:, 0:3, :].transpose(0, 2, 1).reshape(-1, 3)
        assert D.edge_distance(pts, *win) > D.EDGE_GUARD
        assert D.edge_distance(r["seeds"], *win) > D.EDGE_GUARD
        D.records_accumulate(acc, rec, R.N_SEEDS, *win, kind=D.COUNT, seeds=r["seeds"] if p == 0 else None)
    m = DensityMap(win[0], win[1], win[2], win[3])
    chain_setup.chain().run(chain_setup.seeds, depth=CHAIN_DEPTH, method=EULER, delta_t=R.DELTA_T,
                            record_t=R.RECORD_T, layer=CHAIN_LAYER, keep_lines=False, density=m)
    got = _host(m.accum)
    print(f"layer density: {int(acc[:, :, 0].sum())} samples in {int((acc[:, :, 0] > 0).sum())} pixels")
    assert int(acc[:, :, 0].sum()) > R.N_SEEDS
    assert got.dtype == np.int64 and got.tobytes() == acc.tobytes()


def test_ftle_of_a_layer(case):
    """A 24 x 16 FlowMapLattice FTLE image from a layer run: channels 1, 2 and the NaN pattern bytes-equal to
    ftle_reference fed with the restatement's last points and deaths."""
    import ftle_reference as F
    from mops_amd.engine import FlowMapLattice, ParticleSet
    lat = FlowMapLattice(24, 16, (-40.0, 40.0), (-170.0, -100.0))
    seeds = _host(lat.seeds)
    assert seeds.tobytes() == F.lattice(24, 16, (-40.0, 40.0), (-170.0, -100.0)).tobytes()
    depths = np.full(len(seeds), 100.0, dtype=np.float32)
    ref = case.ref(4, True, RELOCATE, seeds=seeds, depths=depths, key="lattice")
    last = LR.lines(case.O, ref, True)["lastPoint"]
    f0, f1 = case.fields()
    ps = ParticleSet(case.dm, lat.seeds, depths, _cfg(RELOCATE, 4), cells=ref["cells"])
    ps.advance(f0, f1, 0, N_STEPS)
    got = _host(lat.ftle_from(ps, horizon=R.DURATION / 86400.0))
    want = F.ftle_image(24, 16, seeds, last, ref["death"], R.DURATION / 86400.0, lat.wrap_lon)
    valid = int((~np.isnan(want[:, :, 1])).sum())
    print(f"layer FTLE: {valid} of {lat.n} pixels valid")
    assert valid >= 24
    for ch in (1, 2):
        assert got[:, :, ch].tobytes() == want[:, :, ch].tobytes(), ch
    assert np.array_equal(np.isnan(got[:, :, 0]), np.isnan(want[:, :, 1]))
    assert np.all(got[:, :, 3] == 1.0)


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals(case, engine_lib):
    """A layer out of range, a null slice and attrs with a layer are refused before any launch."""
    import torch
    from mops_amd import _lib
    from mops_amd.chain import PathlineChain, snapshot_attr_factory, snapshot_field_factory
    from mops_amd.engine import ParticleSet, cell_to_vertex_attr, run_trajectories
    ref = case.ref(4, True, EULER)
    f0, f1 = case.fields()
    s0, s1 = case.snaps
    cfg = _cfg(EULER, 4)
    ps = ParticleSet(case.dm, ref["seeds"], ref["depths"], cfg, cells=ref["cells"])
    att = (cell_to_vertex_attr(case.dm, s0.attributes["temperature"]),
           cell_to_vertex_attr(case.dm, s1.attributes["temperature"]))
    ps.records.fill_(-7.0)
    slab = torch.full((case.mesh.nVertices * 4,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    before = {k: getattr(ps, k).clone() for k in ("x", "y", "z", "depth", "cell", "death", "records")}
    lib = engine_lib
    m = case.dm.handle
    I = _lib.MOPS_ERR_INVALID
    assert lib.mops_layer_velocity_bytes(m) == case.mesh.nVertices * 32
    # a layer outside [0, L)
    for bad in (-1, case.L, case.L + 7):
        assert lib.mops_field_layer_velocity(m, f0.handle, bad, C.c_void_p(slab.data_ptr()), None) == I
        assert b"layer" in lib.mops_last_error()
        with pytest.raises(_lib.MopsError):
            f0.layer_velocity(bad, out=slab)
        with pytest.raises(_lib.MopsError):
            run_trajectories(case.dm, f0, f1, _cfg(EULER, bad), ref["seeds"], depths=ref["depths"], cells=ref["cells"])
    assert lib.mops_field_layer_velocity(m, f0.handle, 4, None, None) == I
    # a null slice
    prt, c = ps.particles(), cfg.ctype()
    rec = C.c_void_p(ps.records.data_ptr())
    good = C.c_void_p(f0.layer_velocity(4).data_ptr())
    assert lib.mops_traj_advance_layer(m, None, None, C.byref(c), C.byref(prt), 0, N_STEPS, rec, ps.rec_stride, None) == I
    assert b"slice" in lib.mops_last_error()
    assert lib.mops_traj_advance_layer(m, None, good, C.byref(c), C.byref(prt), 0, N_STEPS, rec, ps.rec_stride, None) == I
    # attrs with a layer: ValueError before any launch
    with pytest.raises(ValueError, match="layer"):
        run_trajectories(case.dm, f0, f1, cfg, ref["seeds"], attrs={"temperature": att})
    with pytest.raises(ValueError, match="layer"):
        ps.advance(f0, f1, 0, N_STEPS, attrs=([att[0]], [att[1]]))
    with pytest.raises(ValueError, match="layer"):
        ps.advance_pipelined(f0, f1, 0, N_STEPS, [torch.cuda.current_stream()], 2, attrs=([att[0]], [att[1]]))
    snaps = [s0, s1]
    chain = PathlineChain(case.dm, snapshot_field_factory(case.dm, lambda i: snaps[i]), 2, gap_seconds=GAP,
                          make_attrs=snapshot_attr_factory(case.dm, lambda i: snaps[i]))
    with pytest.raises(ValueError, match="layer"):
        chain.run(ref["seeds"], depth=300.0, method=EULER, delta_t=R.DELTA_T, record_t=R.RECORD_T, attrs=True, layer=4)
    with pytest.raises(ValueError, match="layer"):
        chain.run(ref["seeds"], depth=300.0, method=EULER, delta_t=R.DELTA_T, record_t=R.RECORD_T, layer=case.L)
    torch.cuda.synchronize()
    for k, v in before.items():  # nothing was launched: state and records as they were
        assert torch.equal(getattr(ps, k), v), k
    assert bool((slab == -7.0).all())
    # ... and the same call with the slices runs
    back = C.c_void_p(f1.layer_velocity(4).data_ptr())
    assert lib.mops_traj_advance_layer(m, good, back, C.byref(c), C.byref(prt), 0, N_STEPS, rec, ps.rec_stride,
                                       None) == _lib.MOPS_OK
    torch.cuda.synchronize()
    assert np.array_equal(_orig(ps, ps.death), ref["death"])
