"""The trajectory step's trimmed arithmetic against what it replaces, bit for bit:
the pathline time-fraction table against the division, the no-scale division (dev::xdiv_ns) against `/`, the
guarded Wachspress quotient block against the plain block, and whole pathlines against the CPU oracle with
seeds and launch schedules that reach every branch of them."""
import ctypes

import numpy as np
import pytest

TABLE_NS = (1, 2, 3, 7, 720, 1440, 44640, 97, 10007, 65521)


def _table(engine_lib, n):
    out = np.full(max(n, 1), -1.0)
    cap = engine_lib.mops_traj_alpha_table(n, ctypes.c_void_p(out.ctypes.data))
    return out, int(cap)


def test_alpha_table_builder_matches_numpy(engine_lib):
    """The host-built table is the correctly rounded IEEE quotient s / n, as numpy divides; no table past the cap."""
    _, cap = _table(engine_lib, 1)
    assert cap >= 44640, "config 5's 44 640-step months must fit the table"
    for n in TABLE_NS + (cap,):
        t, _ = _table(engine_lib, n)
        assert np.array_equal(t, np.arange(n, dtype=np.float64) / np.float64(n)), n
    t, _ = _table(engine_lib, cap + 1)
    assert np.all(t == -1.0)


def _selftest(engine_lib, gpu, x, n, width, op):
    import torch
    d = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64).reshape(-1), device=gpu)
    out = torch.empty((n, width), dtype=torch.float64, device=gpu)
    assert engine_lib.mops_selftest_math(n, ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(out.data_ptr()), op,
                                         None) == 0
    return out.cpu().numpy()


@pytest.mark.gpu
def test_alpha_table_matches_device_division(gpu, engine_lib):
    """Every entry of the table equals (double)s / (double)n as the kernel divides it on the device."""
    _, cap = _table(engine_lib, 1)
    for n in TABLE_NS + (cap,):
        t, _ = _table(engine_lib, n)
        dev = _selftest(engine_lib, gpu, np.array([float(n)]), n, 1, 3)[:, 0]
        assert np.array_equal(t.view(np.int64), dev.view(np.int64)), n


def _edge_cluster(rng, e, n):
    """n magnitudes within a few ulps to a few percent of 2^e, on both sides."""
    m = np.ldexp(1.0, e) * (1.0 + rng.uniform(-0.03, 0.03, n))
    k = n // 4
    m[:k] = np.ldexp(1.0, e)
    m[k:2 * k] = np.nextafter(np.ldexp(1.0, e), 0.0)
    m[2 * k:3 * k] = np.nextafter(np.ldexp(1.0, e), np.inf)
    return m


@pytest.mark.gpu
def test_xdiv_ns_matches_division(gpu, engine_lib):
    """dev::xdiv_ns inside its window (and `/` outside it, as its callers run it) against `/`, bitwise:
    exponents over the whole double range, clusters at both window edges for both operands, trajectory-sized
    values, and specials.  In-window pairs must really take the no-scale path."""
    rng = np.random.default_rng(2024)
    n = 100000

    def rnd_sign(m):
        return m * np.sign(rng.uniform(-1, 1, m.shape) + 1e-300)

    anyexp = lambda k: rnd_sign(np.ldexp(rng.uniform(1.0, 2.0, k), rng.integers(-1074, 1024, k)))  # noqa: E731
    inwin = lambda k: rnd_sign(np.ldexp(rng.uniform(1.0, 2.0, k), rng.integers(-300, 300, k)))  # noqa: E731
    parts = [(anyexp(2 * n), anyexp(2 * n)), (inwin(n), inwin(n))]
    for e in (-300, 300):
        parts.append((rnd_sign(_edge_cluster(rng, e, n // 2)), inwin(n // 2)))
        parts.append((inwin(n // 2), rnd_sign(_edge_cluster(rng, e, n // 2))))
    # trajectory-sized: Wachspress numerators over denominators, 1 / sum, angle = arc / radius
    parts.append((rng.uniform(1e6, 4e11, n), rng.uniform(1e12, 1e22, n)))
    parts.append((np.ones(n // 2), rng.uniform(1e-16, 1e-6, n // 2)))
    parts.append((rnd_sign(rng.uniform(0.0, 400.0, n // 2)), rng.uniform(6.3e6, 6.4e6, n // 2)))
    sp = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, np.nextafter(2.2250738585072014e-308, 0),
                   np.inf, -np.inf, np.nan, 1.0, -1.0, 3.0, 2.0 ** -300, 2.0 ** 300, np.nextafter(2.0 ** 300, 0),
                   np.nextafter(2.0 ** -300, 0), 2.0 ** 1023, 2.0 ** -1022, 2.0 ** -969, 2.0 ** -970, 1.7976931348623157e308])
    parts.append((np.repeat(sp, len(sp)), np.tile(sp, len(sp))))
    eq = inwin(1000)
    parts.append((eq, eq))  # equal operands
    # exponent differences at the scale thresholds of the compiler's expansion (+-768, the quotient's and the
    # reciprocal's subnormal boundaries)
    for dlt in (767, 768, 769, 1021, 1022, 1023):
        eb = rng.integers(-1022, 1023 - dlt, 500)
        lo_, hi_ = np.ldexp(rng.uniform(1.0, 2.0, 500), eb), np.ldexp(rng.uniform(1.0, 2.0, 500), eb + dlt)
        parts += [(hi_, lo_), (lo_, hi_)]
    a = np.concatenate([p[0] for p in parts]); b = np.concatenate([p[1] for p in parts])
    assert len(a) >= 600000
    o = _selftest(engine_lib, gpu, np.stack([a, b], axis=1), len(a), 3, 4)
    assert np.array_equal(o[:, 0].view(np.int64), o[:, 1].view(np.int64)), "xdiv_ns != a / b"
    win = lambda v: (np.abs(v) >= 2.0 ** -300) & (np.abs(v) < 2.0 ** 300)  # noqa: E731
    assert np.array_equal(o[:, 2] == 1.0, win(a) & win(b)), "the window test differs from its definition"
    assert (o[:, 2] == 1.0).sum() > 200000
    fin = np.isfinite(a) & np.isfinite(b) & (b != 0)
    with np.errstate(all="ignore"):
        assert np.array_equal(o[fin, 1], a[fin] / b[fin]), "device `/` != host `/`"


@pytest.mark.gpu
def test_wachspress_block_matches_plain(gpu, engine_lib):
    """The guarded quotient block of dev::weights (six no-scale divisions, the sum, 1 / sum) against the plain
    block, bitwise including inf and where NaN falls.  The guard must fail on every degenerate hexagon (an
    area of 0, NaN or inf, a numerator of 0, operands outside its windows) and pass on the realistic ones."""
    rng = np.random.default_rng(77)
    n = 60000
    num = 4.0 * rng.uniform(1e6, 1e11, (n, 6))
    area = 2.0 * rng.uniform(1e6, 1e11, (n, 6)) * rng.uniform(1e-3, 1.0, (n, 6))  # p anywhere in the cell
    kind = np.zeros(n, dtype=np.int32)  # 0 = realistic
    k0 = 30000

    def mark(lo, hi, k):  # the rows lo..hi-1 (an index array: one column per row below)
        kind[lo:hi] = k
        return np.arange(lo, hi)

    s = mark(k0, k0 + 2000, 1); area[s, rng.integers(0, 6, 2000)] = 0.0           # one area exactly 0 (on an edge)
    s = mark(k0 + 2000, k0 + 4000, 1)                                              # several (on a vertex: two adjacent)
    j = rng.integers(0, 6, 2000); area[s, j] = 0.0; area[s, (j + 1) % 6] = 0.0
    s = mark(k0 + 4000, k0 + 5000, 1); area[s] = 0.0
    s = mark(k0 + 5000, k0 + 6000, 1); area[s, rng.integers(0, 6, 1000)] = np.nan
    s = mark(k0 + 6000, k0 + 7000, 1); area[s, rng.integers(0, 6, 1000)] = np.inf
    s = mark(k0 + 7000, k0 + 8000, 1); num[s, rng.integers(0, 6, 1000)] = 0.0
    s = mark(k0 + 8000, k0 + 9000, 1); num[s, rng.integers(0, 6, 1000)] = np.nan
    s = mark(k0 + 9000, k0 + 10000, 1); area[s, rng.integers(0, 6, 1000)] = 5e-324
    s = mark(k0 + 10000, k0 + 11000, 1); num[s, rng.integers(0, 6, 1000)] = -4.0e9
    # window edges: numerators around 2^+-100, denominators (products of two areas) around 2^+-190; which
    # side of the edge an item falls on is computed below, not assumed
    s = mark(k0 + 11000, k0 + 15000, 2)
    num[s, 0] = _edge_cluster(rng, 100, 4000)
    num[k0 + 13000:k0 + 15000, 0] = _edge_cluster(rng, -100, 2000)
    s = mark(k0 + 15000, k0 + 19000, 2)  # (areas 2^90, one near 2^100: two denominators near 2^190, four at 2^180)
    area[s] = np.ldexp(1.0, 90)
    area[s, 0] = _edge_cluster(rng, 100, 4000)
    area[k0 + 17000:k0 + 19000, :] = np.ldexp(1.0, -90)
    area[k0 + 17000:k0 + 19000, 0] = _edge_cluster(rng, -100, 2000)
    o = _selftest(engine_lib, gpu, np.concatenate([num, area], axis=1), n, 13, 5)
    fast, plain, passed = o[:, :6], o[:, 6:12], o[:, 12] == 1.0
    assert np.array_equal(fast.view(np.int64), plain.view(np.int64)), (
        f"guarded block != plain block on {np.sum(np.any(fast.view(np.int64) != plain.view(np.int64), axis=1))} items")
    # the guard's truth table from its definition
    with np.errstate(all="ignore"):
        den = area * np.roll(area, -1, axis=1)
        want = (np.all((num >= 2.0 ** -100) & (num < 2.0 ** 100), axis=1) &
                np.all((den >= 2.0 ** -190) & (den < 2.0 ** 190), axis=1))
    assert np.array_equal(passed, want), "the guard differs from its definition"
    assert not passed[kind == 1].any(), "a degenerate hexagon took the fast block"
    assert passed[kind == 0].mean() > 0.99, "realistic hexagons must take the fast block"
    assert passed[kind == 2].any() and not passed[kind == 2].all()
    assert np.isfinite(fast[passed]).all()
    # the degenerate items did produce inf / NaN weights, so their comparison above is not vacuous
    assert (~np.isfinite(plain[kind == 1])).any()


# ---------------------------------------------------------------- whole trajectories against the oracle
TOL_RAD = 1e-6


def _ang_err(a, b):
    na = np.linalg.norm(a, axis=-1)
    nb = np.linalg.norm(b, axis=-1)
    both = (na > 0) & (nb > 0) & np.isfinite(na) & np.isfinite(nb)
    c = np.sum(a * b, -1) / np.where(both, na * nb, 1.0)
    return np.where(both, np.arccos(np.clip(c, -1.0, 1.0)), 0.0)


def _assert_lines_match(got, ref, label):
    """Bit-exact match of one run against the oracle: death steps, where zeros and NaN fall, every point,
    velocity and final depth (the semantics of tests/test_gpu_parity.py's assert_lines_match)."""
    assert np.array_equal(got["death_step"], ref["death"]), f"{label}: death steps differ"
    for key in ("points", "lastPoint"):
        a, b = got[key], ref[key]
        assert np.array_equal(np.linalg.norm(a, axis=-1) == 0, np.linalg.norm(b, axis=-1) == 0), f"{label} {key} zeros"
        assert np.array_equal(np.isfinite(a), np.isfinite(b)), f"{label} {key} NaN pattern"
        e = _ang_err(a, b)
        assert e.max() < TOL_RAD, f"{label} {key}: max angular error {e.max()} rad"
        assert np.array_equal(a, b, equal_nan=True), (
            f"{label} {key}: not bit-exact ({np.mean(np.all(a == b, axis=-1)):.6f} of points equal, "
            f"max angular error {e.max():.3e} rad)")
    assert np.array_equal(got["velocity"], ref["velocity"], equal_nan=True), f"{label}: velocity not bit-exact"
    assert np.array_equal(got["final_depth"], ref["final_depth"], equal_nan=True), f"{label}: depth not bit-exact"


@pytest.fixture(scope="module")
def dev_small(gpu, engine_lib, small_case):
    from mops_amd.engine import DeviceField, DeviceMesh
    mesh, s0, s1 = small_case
    dm = DeviceMesh.from_mesh(mesh)
    return dm, DeviceField.from_snapshot(dm, s0), DeviceField.from_snapshot(dm, s1)


@pytest.fixture(scope="module")
def ref_small(oracle_lib, small_case):
    mesh, s0, s1 = small_case
    return oracle_lib.preprocess(mesh, s0), oracle_lib.preprocess(mesh, s1)


@pytest.fixture(scope="module")
def trim_seeds(small_case):
    """Dense cells (>= 45 particles per cell, so waves tile; one or two depth groups) as in
    test_pathline_cooperative_waves, then seeds exactly on polygon vertices (an area of exactly 0: inf / NaN
    weights, the plain quotient block), on edge midpoints, on cell centres, and over land (dead at step 0)."""
    from mops_amd import synth
    mesh, _, _ = small_case
    rng = np.random.default_rng(41)
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    vc = np.asarray(mesh.vertexCoord, dtype=np.float64).reshape(-1, 3)
    voc = np.asarray(mesh.verticesOnCell).reshape(mesh.nCells, -1).astype(np.int64) - 1
    nv = np.asarray(mesh.nEdgesOnCell).astype(np.int64)
    cells = rng.choice(mesh.nCells, 14, replace=False)
    seeds, depths = [], []
    for j, c in enumerate(cells):
        k = 45 + j
        u = cc[c] / np.linalg.norm(cc[c])
        jit = rng.normal(size=(k, 3)) * 2.0e4
        p = u + (jit - np.outer(jit @ u, u)) / 6.371e6
        seeds.append(p / np.linalg.norm(p, axis=1, keepdims=True) * 6.37101e6)
        depths.append(np.full(k, 300.0) if j < 7 else np.where(np.arange(k) % 2 == 0, 300.0, 1100.0))
    verts, mids = [], []
    for c in cells:
        ids = voc[c, :nv[c]]
        verts.append(vc[ids[:3]])                                   # the mesh's own doubles
        mids.append(0.5 * (vc[ids[:3]] + vc[np.roll(ids, -1)[:3]]))
    verts = np.concatenate(verts); mids = np.concatenate(mids)
    centres = cc[cells] * (synth.SEED_RADIUS / np.linalg.norm(cc[cells], axis=1, keepdims=True))
    land = synth.uniform_band_seeds(400, seed=3)[:37]
    special = np.concatenate([verts, mids, centres, cc[cells]])
    seeds += [special, land]
    depths += [np.full(len(special), 300.0), np.full(len(land), 500.0)]
    # The 149 special and land seeds sit one or two to a cell: with them alone the set has 86 runs of equal cells in
    # 14 waves, over the 6 per wave at which a slot-ordered launch still selects the tile kernels.  30 more
    # particles in each dense cell (after the seeds above, from a generator of their own, so those are unchanged)
    # bring it to 21 waves, and every launch of _run_segments selects the tile (asserted there).
    rng2 = np.random.default_rng(4141)
    for j, c in enumerate(cells):
        u = cc[c] / np.linalg.norm(cc[c])
        jit = rng2.normal(size=(30, 3)) * 2.0e4
        p = u + (jit - np.outer(jit @ u, u)) / 6.371e6
        seeds.append(p / np.linalg.norm(p, axis=1, keepdims=True) * 6.37101e6)
        depths.append(np.full(30, 300.0) if j < 7 else np.where(np.arange(30) % 2 == 0, 300.0, 1100.0))
    seeds = np.concatenate(seeds)
    assert len(seeds) % 64 != 0
    return seeds, np.concatenate(depths).astype(np.float32)


def _run_segments(dm, f0, f1, cfg, seeds, depths, cells, bounds):
    """The run as slot-ordered launches over [bounds[i], bounds[i+1]), assembled like run_trajectories' result;
    every launch is asserted to have selected the tile kernels (tests/tile_case.py)."""
    import tile_case
    return tile_case.run_slot_ordered(dm, f0, f1, cfg, seeds, depths, cells, expect_flag=1, bounds=bounds)


# RK4 runs with a time step at which particles die during the run on this 2.4k-cell mesh (a stage leaves the
# step's start cell, quirk Q1; found with the CPU oracle).  Euler keeps the usual 120 s, at which no Euler particle
# dies after step 0 here: the synthetic flow vanishes at the coast, and a step long enough to carry a particle
# past a neighbouring cell (400 000 s) rotates by angles at which the device library's sin / cos and the host's
# differ in the last bit -- the oracle comparison is then off by 2e-8 rad on the parent commit's engine just the
# same (measured), so it cannot test this change.  The death-step assertions therefore rest on the RK4 cases.
DELTA_T = {"euler": 120, "rk4": 3000}
# recordT as a function of deltaT: a multiple (a record every 5 steps); not one (period 4 steps, 90 record steps
# for K = 86 records: K cut short); not one, and the period no divisor of the step count (8 steps: 45, K = 43)
RECORD_T = {"every5": lambda dt: 5 * dt, "odd4": lambda dt: 4 * dt + dt // 6, "odd8": lambda dt: 8 * dt + dt // 3}


@pytest.mark.gpu
@pytest.mark.parametrize("rec", ["every5", "odd4", "odd8"])
@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_pathline_trims_parity(dev_small, ref_small, small_case, oracle_lib, trim_seeds, method, direction, rec):
    """Pathlines through the table-fed time fraction and the guarded quotient block, bit-exact against the
    oracle: through run_trajectories (a processing order: the plain kernels), and slot-ordered on the tile kernels
    (selection flag 1 asserted per launch) as one launch and as three launches whose boundaries fall between
    record steps.  Some particles are dead at step 0 and some survive; in the RK4 cases some die on a record step
    and some between record steps (see DELTA_T)."""
    from mops_amd.engine import TrajectoryConfig, run_trajectories
    mesh, _, _ = small_case
    dm, f0, f1 = dev_small
    r0, r1 = ref_small
    seeds, depths = trim_seeds
    euler, back = method == "euler", direction == "backward"
    dt = DELTA_T[method]
    dur, record_t = 360 * dt, RECORD_T[rec](dt)
    cfg = TrajectoryConfig(deltaT=dt, simulationDuration=dur, recordT=record_t, depth=0.0, method=1 if euler else 0,
                           direction=1 if back else 0)
    assert cfg.n_steps == 360
    got = run_trajectories(dm, f0, f1, cfg, seeds, depths=depths)
    ref = oracle_lib.run(mesh, r0, r1, seeds, depths=depths, delta_t=dt, duration=dur, record_t=record_t,
                         euler=euler, backward=back, cells=got["cells"])
    label = f"pathline {method} {direction} {rec}"
    _assert_lines_match(got, ref, label + " (one launch)")
    one = _run_segments(dm, f0, f1, cfg, seeds, depths, got["cells"], [0, cfg.n_steps])
    _assert_lines_match(one, ref, label + " (one launch, tile kernels)")
    period = record_t // dt
    bounds = [0, 101, 233, cfg.n_steps]
    assert all((b % period) not in (0, period - 1) for b in bounds[1:-1])
    if rec != "every5":
        assert record_t % dt != 0 and cfg.n_steps // period > cfg.n_records  # K cut short
    seg = _run_segments(dm, f0, f1, cfg, seeds, depths, got["cells"], bounds)
    _assert_lines_match(seg, ref, label + " (three launches)")
    death = ref["death"]
    assert (death == 0).any() and (death < 0).any()
    late = death[death > 0]
    print(f"{label}: {len(late)} die after step 0, {int(((late + 1) % period == 0).sum())} of them on a record step")
    if not euler:
        assert ((late + 1) % period == 0).any(), "no particle died on a record step"
        assert ((late + 1) % period != 0).any(), "no particle died between record steps"


@pytest.mark.gpu
def test_run_beyond_the_table_cap(gpu, engine_lib, dev_small, ref_small, small_case, oracle_lib):
    """A run one step longer than the table cap gets no table: the kernel divides, bit-exact against the oracle."""
    from mops_amd import synth
    from mops_amd.engine import TrajectoryConfig, run_trajectories
    mesh, _, _ = small_case
    dm, f0, f1 = dev_small
    r0, r1 = ref_small
    _, cap = _table(engine_lib, 1)
    n_steps = cap + 1
    seeds = synth.uniform_band_seeds(12, seed=11)
    dur = 2 * n_steps
    cfg = TrajectoryConfig(deltaT=2, simulationDuration=dur, recordT=dur // 4, depth=200.0, method=1)
    assert cfg.n_steps == n_steps and cfg.n_records == 4
    got = run_trajectories(dm, f0, f1, cfg, seeds)
    ref = oracle_lib.run(mesh, r0, r1, seeds, depth=200.0, delta_t=2, duration=dur, record_t=dur // 4, euler=True,
                         cells=got["cells"])
    _assert_lines_match(got, ref, "pathline beyond the table cap")
    assert (ref["death"] < 0).any()
