"""Meshes whose cells of seven and more vertices are alive, and the cases run on them.

TEST INFRASTRUCTURE ONLY: the product never imports this module.

tests/golden/voronoi_{me7,me12,me20}.npz (written by tests/golden/make_voronoi_meshes.py) hold Delaunay
triangulations with "wheels": a centre point and k points on a ring around it, so that the centre's Voronoi cell
has k vertices; the cells around a wheel get 7 to 9.  mops_amd.synth.make_mesh(triangulation=...) turns each
into a mesh in the reference's storage convention with maxEdges 7, 12 and 20 -- the three kernel instantiations.

The mean cell is 890 km across, so the flow of world() is 20 times synth's default and a run covers a day: a
particle then crosses a cell or two within a few hundred steps.  The step is kept at 240 s, under 3 km: an Euler step
turns the position by speed * deltaT / radius, and that angle has to stay below MAX_STEP_ANGLE.  Bit parity with
the oracle needs the device library's sin / cos to give the host library's doubles, which holds for small angles
only: measured on an MI355X, none of 8e6 angles below 1e-3 rad differ, 4 of 2e6 cosines in
[1e-3, 3e-3) do -- such as cos(0.0010925430624395252), which lies within 3e-7 ulp of a rounding tie.
"""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("me7", "me12", "me20")
MAX_EDGES = {"me7": 7, "me12": 12, "me20": 20}
# (lat, lon, k) in degrees; consecutive wheels form pairs 2.6 mean spacings apart (their rims touch)
WHEELS = {
    "me7": ((0.0, -150.0, 7), (0.0, -129.0, 7), (-35.0, -120.0, 7), (-35.0, -95.0, 7), (25.0, -45.0, 7),
            (25.0, -22.0, 7), (-30.0, 60.0, 7), (-30.0, 84.0, 7), (-45.0, -20.0, 7), (-45.0, 9.5, 7),
            (30.0, 175.0, 7), (30.0, -161.0, 7), (-50.0, -170.0, 7), (-50.0, -137.7, 7)),
    "me12": ((0.0, -150.0, 8), (0.0, -129.0, 12), (-35.0, -120.0, 9), (-35.0, -95.0, 10), (25.0, -45.0, 12),
             (25.0, -22.0, 8), (-30.0, 60.0, 10), (-30.0, 84.0, 9)),
    "me20": ((0.0, -150.0, 20), (0.0, -129.0, 16), (-35.0, -120.0, 13), (-35.0, -95.0, 20), (25.0, -45.0, 16),
             (25.0, -22.0, 13)),
}
MIN_HEPTAGONS = {"me7": 40, "me12": 0, "me20": 0}   # of the whole sphere, before the land is culled
N_LEVELS = 10
FLOW = dict(u0=10.0, u1=5.0)
DELTA_T, DURATION, RECORD_T = 240, 86400, 7200   # 360 steps, 12 records
MAX_STEP_ANGLE = 5.0e-4    # rad per step: half the smallest angle at which device and host cos were seen to differ


@functools.lru_cache(maxsize=None)
def load_mesh(key):
    from mops_amd import synth
    with np.load(os.path.join(HERE, "golden", f"voronoi_{key}.npz")) as z:
        assert z["points"].dtype == np.float64 and z["triangles"].dtype == np.int16
        tri = (z["points"], z["triangles"].astype(np.int64))
    return synth.make_mesh(0, n_levels=N_LEVELS, max_edges=MAX_EDGES[key], triangulation=tri)


@functools.lru_cache(maxsize=None)
def world(key):
    """(mesh, snapshot 0, snapshot 1)."""
    from mops_amd import synth
    mesh = load_mesh(key)
    return (mesh, synth.make_snapshot(mesh, timestep=0, phase=0.0, **FLOW),
            synth.make_snapshot(mesh, timestep=1, phase=0.35, **FLOW))


def degrees(mesh):
    return np.asarray(mesh.nEdgesOnCell).astype(np.int64)


def polygons(mesh):
    """Per cell its vertices [nv, 3] in verticesOnCell order."""
    voc = np.asarray(mesh.verticesOnCell).reshape(-1, mesh.maxEdges).astype(np.int64) - 1
    nv = degrees(mesh)
    vc = np.asarray(mesh.vertexCoord, dtype=np.float64).reshape(-1, 3)
    return [vc[voc[c, :nv[c]]] for c in range(mesh.nCells)]


def neighbours(mesh):
    """cellsOnCell, 0-based, -1 for none or padding."""
    return np.asarray(mesh.cellsOnCell).reshape(-1, mesh.maxEdges).astype(np.int64) - 1


def wheel_cells(mesh, key):
    """The cell of each wheel's centre (the centre is a mesh point, so the nearest cell centre is exact)."""
    from mops_amd import synth
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    out = []
    for lat, lon, k in WHEELS[key]:
        p = synth.latlon_to_xyz(lat, lon, synth.SPHERE_RADIUS)
        c = int(((cc - p) ** 2).sum(-1).argmin())
        assert degrees(mesh)[c] == k, (key, lat, lon, k, int(degrees(mesh)[c]))
        out.append(c)
    return out


def _around(mesh, cells, count, spread, rng):
    """``count`` seeds per cell, normally scattered ``spread`` metres around its centre."""
    from mops_amd import synth
    c = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)[np.repeat(cells, count)]
    c = c + rng.normal(scale=spread, size=c.shape)
    return c * (synth.SEED_RADIUS / np.linalg.norm(c, axis=1))[:, None]


@functools.lru_cache(maxsize=None)
def seeds(key):
    """The trajectory seeds of one mesh, ordered so that the 64-lane waves of a launch are of every kind, both in
    seed order (a ParticleSet with use_order=False launches in it) and in the engine's locality order
    (run_trajectories and ParticleSet sort the particles by their cell first, stably, so the particles of one cell
    stay together: 127 or more in a cell hold a whole aligned wave wherever the cell's block begins):

    * 2 x 64 seeds in hexagons only (whole waves inside hexagons);
    * 128 seeds inside the first wheel's centre cell and 128 inside the widest cell (whole waves in one wide cell);
    * per wide cell 24 seeds scattered 150 km around its centre, interleaved with as many around hexagons
      (waves that mix degrees);
    * boundary_seeds(): per wheel its centre, one of its vertices and points exactly on its edge planes;
    * 200 band seeds.
    """
    from mops_amd import synth
    mesh = load_mesh(key)
    nv = degrees(mesh)
    rng = np.random.default_rng(2025)
    hexes = np.flatnonzero(nv == 6)
    wide = np.flatnonzero(nv >= 7)
    wc = wheel_cells(mesh, key)
    parts = [_around(mesh, rng.choice(hexes, 128), 1, 1.0e5, rng),
             _around(mesh, [wc[0]], 128, 6.0e4, rng),
             _around(mesh, [int(np.argmax(nv))], 128, 6.0e4, rng)]
    a = _around(mesh, wide, 24, 1.5e5, rng)
    b = _around(mesh, rng.choice(hexes, len(wide)), 24, 1.5e5, rng)
    mixed = np.empty((2 * len(a), 3))
    mixed[0::2], mixed[1::2] = a, b
    parts.append(mixed)
    parts.append(boundary_seeds(key))
    parts.append(synth.uniform_band_seeds(200, seed=43))
    return np.concatenate(parts)


def edge_plane_points(poly, cc, cell, limit):
    """Up to ``limit`` points of one cell's edges that lie, in floating point, exactly on the edge's plane:
    dot(cross(a, b), p) == 0.0 with IsInMesh's operation order and >= 0 for the cell's other edges, and whose
    nearest cell centre is that cell's alone (ref_case.edge_seeds' condition, here on several points per edge)."""
    nxt = np.roll(poly, -1, axis=0)
    n = np.stack([poly[:, 1] * nxt[:, 2] - poly[:, 2] * nxt[:, 1], poly[:, 2] * nxt[:, 0] - poly[:, 0] * nxt[:, 2],
                  poly[:, 0] * nxt[:, 1] - poly[:, 1] * nxt[:, 0]], axis=-1)
    out = []
    for k in range(len(poly)):
        for t in np.arange(1, 64) / 64.0:
            p = poly[k] + t * (nxt[k] - poly[k])
            d = (n[:, 0] * p[0] + n[:, 1] * p[1]) + n[:, 2] * p[2]
            if d[k] == 0.0 and (d >= 0.0).all():
                d2 = ((cc - p) ** 2).sum(-1)
                two = np.sort(d2)[:2]
                if two[1] > two[0] and d2[cell] == two[0]:
                    out.append(p)
                    break
        if len(out) == limit:
            break
    return out


@functools.lru_cache(maxsize=None)
def boundary_seeds(key):
    """Per wheel: its centre and one vertex of its cell, both scaled to the seed radius, and up to 3 points
    exactly on the planes of its cell's edges (the IsInMesh boundary of a cell of 7 to 20 vertices)."""
    from mops_amd import synth
    mesh = load_mesh(key)
    polys = polygons(mesh)
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    out, on_plane = [], 0
    for c in wheel_cells(mesh, key):
        out += [p * (synth.SEED_RADIUS / np.linalg.norm(p)) for p in (cc[c], polys[c][0])]
        hits = edge_plane_points(polys[c], cc, c, 3)
        on_plane += len(hits)
        out += hits
    assert on_plane >= len(WHEELS[key]), (key, on_plane)
    return np.array(out)


MODES = [(pathline, euler, backward) for pathline in (False, True) for euler in (True, False)
         for backward in (False, True)]


def mode_name(pathline, euler, backward):
    return f"{'path' if pathline else 'stream'}_{'euler' if euler else 'rk4'}_{'backward' if backward else 'forward'}"


# ---- settings of the trajectory cases -----------------------------------------------------------------------
DEPTH = 300.0


def times(euler):
    """(deltaT, duration, recordT): 360 steps for Euler; 180 for RK4, which dies at every cell crossing (quirk
    Q1), so that more than half of its particles live to the end."""
    return (DELTA_T, DURATION, RECORD_T) if euler else (DELTA_T, DURATION // 2, RECORD_T // 2)


@functools.lru_cache(maxsize=None)
def derived(key):
    from oracle import oracle as O
    mesh, s0, s1 = world(key)
    return O.preprocess(mesh, s0), O.preprocess(mesh, s1)


@functools.lru_cache(maxsize=None)
def seed_cells(key):
    from oracle import oracle as O
    return O.knn(load_mesh(key), seeds(key))


@functools.lru_cache(maxsize=None)
def oracle_run(key, pathline, euler, backward, every_step=False):
    """oracle.run on seeds(key); ``every_step`` records every step (for the conditions on cell crossings)."""
    from oracle import oracle as O
    r0, r1 = derived(key)
    dt, duration, record_t = times(euler)
    return O.run(load_mesh(key), r0, r1 if pathline else None, seeds(key), depth=DEPTH, delta_t=dt,
                 duration=duration, record_t=dt if every_step else record_t, euler=euler, backward=backward,
                 cells=seed_cells(key))


# ---- images -------------------------------------------------------------------------------------------------
# (width, height, (lat range, lon range)): W != H, pixel counts no multiple of 64; each window holds a pair of
# wheels (the first six wheels stand at the same places in all three meshes) and reaches one of synth's land caps or the culled polar cap
WINDOWS = {"pacific": (45, 29, ((-14.0, 42.0), (-162.0, -92.0))), "atlantic": (41, 27, ((0.0, 40.0), (-58.0, 16.0))),
           "south": (39, 57, ((-88.0, -15.0), (-138.0, -78.0)))}
IMAGE_DEPTH = 2800.0   # between the shallowest and the deepest last-layer top: part of each window is out of range
IMAGE_LAYER = 4
# (width, height, lon range, latitude): rows through the centres of a pair of wheels
# (the first six wheels; the cells of 7 to 9 vertices around the wheels are the windows' to cover)
LATITUDES = {"lat_0": (37, 19, (-170.0, -105.0), 0.0), "lat_25": (35, 21, (-62.0, 14.0), 25.0),
             "lat_m35": (39, 23, (-140.0, -75.0), -35.0)}


@functools.lru_cache(maxsize=None)
def window_cells(key, win):
    import remap_reference as RR
    from oracle import oracle as O
    w, h, (lat, lon) = WINDOWS[win]
    return O.knn(load_mesh(key), RR.depth_positions(w, h, lat, lon))


@functools.lru_cache(maxsize=None)
def restated_depth(key, win, rule):
    import remap_reference as RR
    w, h, (lat, lon) = WINDOWS[win]
    return RR.fixed_depth(load_mesh(key), derived(key)[0], w, h, lat, lon, IMAGE_DEPTH, window_cells(key, win),
                          layer_rule=rule)


@functools.lru_cache(maxsize=None)
def restated_layer(key, win):
    import image_reference as IR
    w, h, (lat, lon) = WINDOWS[win]
    return IR.fixed_layer(load_mesh(key), derived(key)[0], w, h, lat, lon, IMAGE_LAYER, window_cells(key, win))


@functools.lru_cache(maxsize=None)
def latitude_cells(key, row):
    import remap_reference as RR
    from oracle import oracle as O
    w, _, lon, lat = LATITUDES[row]
    return O.knn(load_mesh(key), RR.latitude_positions(w, lon, lat))


def depth_range(mesh):
    return float(mesh.refBottomDepth[0]), float(mesh.refBottomDepth[-1])


@functools.lru_cache(maxsize=None)
def restated_latitude(key, row):
    import remap_reference as RR
    mesh = load_mesh(key)
    w, h, lon, lat = LATITUDES[row]
    return RR.fixed_latitude(mesh, derived(key)[0], w, h, lon, lat, depth_range(mesh), latitude_cells(key, row))


def valid_by_degree(mesh, cells, code):
    """{degree: valid pixels} over the cells of degree >= 7 (``cells`` per pixel, or per column of ``code``)."""
    import remap_reference as RR
    nv = degrees(mesh)
    cells = np.broadcast_to(np.asarray(cells).reshape((-1, code.shape[1])), code.shape)
    d = nv[cells[code == RR.VALID]]
    return {int(k): int((d == k).sum()) for k in np.unique(nv[nv >= 7])}


def coverage(code):
    """(valid, other) pixels; the tests ask for >= 40 % valid and >= 5 % NaN."""
    import remap_reference as RR
    valid = int((code == RR.VALID).sum())
    return valid, int(code.size) - valid


# ---- dense waves, and the small seed sets of the per-particle Python restatements ---------------------------
@functools.lru_cache(maxsize=None)
def dense_seeds(key):
    """test_gpu_parity.test_pathline_cooperative_waves' recipe (14 cells with 45..58 particles each scattered
    20 km around the centre, at one or two depths, and 37 band seeds) on 5 wide cells -- two wheel centres and
    three cells of a wheel's surroundings -- and 9 hexagons that border a wide cell on its western, upstream side,
    seeded towards that cell."""
    from mops_amd import synth
    mesh = load_mesh(key)
    nv, nb = degrees(mesh), neighbours(mesh)
    rng = np.random.default_rng(41)
    wc = wheel_cells(mesh, key)
    others = np.setdiff1d(np.flatnonzero(nv >= 7), wc)
    wide = list(wc[:2]) + list(rng.choice(others, 3, replace=False))
    lon = np.asarray(mesh.lon_cell)
    west = sorted({(int(n), int(c)) for c in np.flatnonzero(nv >= 7) for n in nb[c, :nv[c]]
                   if n >= 0 and nv[n] == 6 and 0.0 < np.sin(lon[c] - lon[n])})
    west = [west[i] for i in sorted(np.unique([n for n, _ in west], return_index=True)[1])]   # one per hexagon
    hexes = [west[i] for i in rng.choice(len(west), 9, replace=False)]
    cells = [c for pair in zip(hexes, wide + [None] * 4) for c in pair if c is not None]
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    seeds_, depths, ids = [], [], []
    for j, c in enumerate(cells):
        k = 45 + j
        if isinstance(c, tuple):    # a hexagon: 40 % of the way to the wide cell's centre (the shared edge is at 50 %)
            u = cc[c[0]] + 0.4 * (cc[c[1]] - cc[c[0]])
            c = c[0]
        else:
            u = cc[c]
        ids.append(int(c))
        u = u / np.linalg.norm(u)
        jit = rng.normal(size=(k, 3)) * 2.0e4
        p = u + (jit - np.outer(jit @ u, u)) / 6.371e6
        seeds_.append(p / np.linalg.norm(p, axis=1, keepdims=True) * 6.37101e6)
        depths.append(np.full(k, 300.0) if j < 7 else np.where(np.arange(k) % 2 == 0, 300.0, 1100.0))
    cells = ids
    assert len(cells) == 14 and sum(nv[c] >= 7 for c in cells) == 5
    seeds_.append(synth.uniform_band_seeds(400, seed=3)[:37]); depths.append(np.full(37, 500.0))
    return np.concatenate(seeds_), np.concatenate(depths).astype(np.float32), np.array(cells)


DENSE_TIMES = (240, 43200, 3600)   # 180 steps


@functools.lru_cache(maxsize=None)
def sample_seeds(key):
    """(seeds, float32 depths, cells) for the per-particle Python restatements: on the line between the centres
    of a wide cell and of a neighbour, 47 % of the way from either centre (the shared edge lies at 50 %, some 25 km
    on), so that a quarter-day run carries about half of them across it -- every 8th of these pairs, the boundary
    seeds and 20 band seeds: some 200 particles, no multiple of 64."""
    from mops_amd import synth
    from oracle import oracle as O
    mesh = load_mesh(key)
    nv, nb = degrees(mesh), neighbours(mesh)
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    pairs = [(c, n) for c in np.flatnonzero(nv >= 7) for n in nb[c, :nv[c]] if n >= 0][::8]
    near = [cc[a] + 0.47 * (cc[b] - cc[a]) for c, n in pairs for a, b in ((c, n), (n, c))]
    near = [q * (synth.SEED_RADIUS / np.linalg.norm(q)) for q in near]
    s = np.concatenate([np.array(near), boundary_seeds(key), synth.uniform_band_seeds(20, seed=47)])
    if len(s) % 64 == 0:
        s = s[:-1]
    d = np.random.default_rng(9).uniform(5, 1500, len(s)).astype(np.float32)
    d[::8] = 0
    return s, d, O.knn(mesh, s)


# 96 steps of 240 s with a record every 8: K = 12
SAMPLE_TIMES = (240, 23040, 1920)
