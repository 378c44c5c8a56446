"""The cooperative-tile selection restated, and runs that are asserted to have taken the tile kernels.

TEST INFRASTRUCTURE ONLY: the product never imports this module.

A pathline launch of ``mops_traj_advance`` on a maxEdges <= 7 mesh WITHOUT a processing order first runs
``coop_select_kernel`` over the particles' cells in slot order; its flag picks the tile kernels (Euler: the tile
step; RK4: the hand-off kernel and the resumed one) or the plain kernel.  ``run_trajectories`` always passes an
order, so it never selects and always runs the plain kernels; a ``ParticleSet`` keeps its state physically in slot
order and passes none.  ``DeviceMesh.tile_selection`` is the witness: a host count of the launches that selected
and the device flag of the last one.
"""
import numpy as np

WAVE = 64
MAX_SAMPLED = 4096   # coop_select_kernel samples at most this many waves ...
MAX_RUNS = 6         # ... and picks the tile when they hold at most this many runs of equal cells on average


def sampled_runs(cells_in_slot_order, n_live=None, every_wave=False):
    """(runs, S): the runs of equal cells, counted per 64-slot wave (the last one partial), summed over the S
    sampled waves w = j * waves // S, j < S = min(waves, 4096), of the first m = min(n, n_live) slots.
    ``every_wave``: over all waves instead (what the rule would count without the sampling)."""
    cells = np.asarray(cells_in_slot_order).reshape(-1)
    n = len(cells)
    m = n if n_live is None else min(n, int(n_live))
    waves = -(-m // WAVE)
    S = waves if every_wave else min(waves, MAX_SAMPLED)
    runs = 0
    for j in range(S):
        w = j * waves // S
        c = cells[WAVE * w:min(m, WAVE * w + WAVE)]
        runs += 1 + int(np.count_nonzero(c[1:] != c[:-1]))
    return runs, S


def select_rule(cells_in_slot_order, n_live=None, every_wave=False):
    """The flag coop_select_kernel writes: 1 iff S > 0 and runs <= 6 * S."""
    runs, S = sampled_runs(cells_in_slot_order, n_live, every_wave)
    return 1 if (S > 0 and runs <= MAX_RUNS * S) else 0


def centre_seeds(mesh, cells):
    """One seed per entry of ``cells`` at that cell's centre, scaled to the seed radius."""
    from mops_amd import synth
    c = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)[np.asarray(cells, dtype=np.int64)]
    return c * (synth.SEED_RADIUS / np.linalg.norm(c, axis=1))[:, None]


def selection(dm, stream=None):
    """(flag, count) of ``stream`` on the device mesh (blocking)."""
    return dm.tile_selection(stream)


def assert_selected(dm, count_before, expect_flag, stream=None, launches=1, what=""):
    """After ``launches`` pathline launches on ``stream``: each made a selection and the last fell ``expect_flag``.
    Returns the new count."""
    flag, count = dm.tile_selection(stream)
    assert count == count_before + launches, (
        f"{what}: {count - count_before} of {launches} launches ran the tile selection")
    assert flag == expect_flag, f"{what}: selection flag {flag}, expected {expect_flag}"
    return count


def run_slot_ordered(dm, f0, f1, cfg, seeds, depths, cells, expect_flag, bounds=None):
    """The pathline run through a ParticleSet -- state in slot order, no processing order, so the launch selects --
    as ``run_trajectories`` returns it: points, velocity, temperature, salinity, lastPoint, final_depth, death_step
    and cells in seed order.  One ``advance`` over the whole run (``bounds``: one per [bounds[i], bounds[i+1])),
    then ``finalize``.  Asserts that every launch made a selection and that it fell ``expect_flag``."""
    import torch
    from mops_amd.engine import ParticleSet
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    ps = ParticleSet(dm, seeds, cfg.depth if depths is None else depths, cfg, cells=cells)
    bounds = [0, cfg.n_steps] if bounds is None else list(bounds)
    _, count = dm.tile_selection()
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ps.advance(f0, f1, lo, hi)
        count = assert_selected(dm, count, expect_flag, what=f"slot-ordered launch [{lo}, {hi})")
    lines = ps.finalize(pathline=True)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in lines.items()}
    out["death_step"] = ps.original(ps.death).cpu().numpy()
    out["final_depth"] = ps.original(ps.depth).cpu().numpy()
    out["cells"] = cells.copy()
    out["slot_ids"] = ps.ids.cpu().numpy()   # slot -> seed index: wave w holds seeds slot_ids[64 w : 64 w + 64]
    return out


def dense_seeds(mesh):
    """test_gpu_parity.test_pathline_cooperative_waves' recipe (forward variant), restated: 14 cells x 45..58
    particles jittered by 20 km at one or two depths, and 37 band seeds -- 758 particles, 12 waves."""
    from mops_amd import synth
    rng = np.random.default_rng(41)
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    cells = rng.choice(mesh.nCells, 14, replace=False)
    seeds, depths = [], []
    for j, c in enumerate(cells):
        k = 45 + j
        u = cc[c] / np.linalg.norm(cc[c])
        jit = rng.normal(size=(k, 3)) * 2.0e4
        p = u + (jit - np.outer(jit @ u, u)) / 6.371e6
        seeds.append(p / np.linalg.norm(p, axis=1, keepdims=True) * 6.37101e6)
        depths.append(np.full(k, 300.0) if j < 7 else np.where(np.arange(k) % 2 == 0, 300.0, 1100.0))
    seeds.append(synth.uniform_band_seeds(400, seed=3)[:37]); depths.append(np.full(37, 500.0))
    return np.concatenate(seeds), np.concatenate(depths).astype(np.float32)


# ---- the RK4 hand-off, case by case -------------------------------------------------------------------------
HANDOFF_GROUPS = 9   # MOPS_COOP_G_PR: the hand-off kernel's tile holds at most this many (cell, layer, layer) groups
SPLIT_LAYERS = (0, 2, 4, 6, 8)


def _around_cell(mesh, cell, count, spread, rng, cells_of):
    """``count`` seeds scattered ``spread`` metres around the cell's centre that locate to that cell."""
    from mops_amd import synth
    c = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)[cell]
    p = c + rng.normal(scale=spread, size=(8 * count, 3))
    p *= (synth.SEED_RADIUS / np.linalg.norm(p, axis=1))[:, None]
    p = p[cells_of(p) == cell][:count]
    assert len(p) == count
    return p


def handoff_case(mesh, derived, morton, cells_of, wide_spread):
    """Seeds (with float32 depths, cells and each seed's role) whose 64-lane waves, in the engine's locality order,
    are each of one kind -- every group is 64 particles of one cell (or of two cells next to each other in the
    order), and the one partial group sits in the last cell of the order:

    * "nonhex": 64 particles 20 km around the centre of a cell that is no hexagon;
    * "quiet":  64 particles 20 km around a hexagon's centre;
    * "dying":  64 particles ``wide_spread`` metres around a hexagon's centre, so that some reach its edges;
    * "split":  2 x 32 particles 20 km around the centres of two hexagons that are neighbours in the order, each at
      the mid-depths of the layers SPLIT_LAYERS of its own column: 10 (cell, layer) groups;
    * "tail":   30 particles in the last hexagon of the order (the partial wave).

    ``morton``: the cells in the engine's locality order; ``cells_of(points)``: their nearest cells; ``derived``:
    oracle.preprocess of the front snapshot (its cell-centre layer tops place the "split" depths)."""
    nv = np.asarray(mesh.nEdgesOnCell).astype(np.int64)
    L = mesh.nVertLevels
    ztop = np.asarray(derived.cell_ztop).reshape(mesh.nCells, L)
    depth_of = -ztop[:, -1]
    deep = (nv == 6) & (depth_of > 0.6 * depth_of.max())
    rank = np.empty(mesh.nCells, dtype=np.int64)
    rank[morton] = np.arange(mesh.nCells)
    rng = np.random.default_rng(59)
    hexes = morton[deep[morton]]                      # deep hexagons in the order
    pair = next(i for i in range(len(hexes) // 3, len(hexes) - 1) if rank[hexes[i + 1]] == rank[hexes[i]] + 1)
    split = (int(hexes[pair]), int(hexes[pair + 1]))
    quiet, dying = int(hexes[len(hexes) // 5]), int(hexes[len(hexes) // 2 + 7])
    tail = int(hexes[-1])
    live = [c for c in np.flatnonzero(nv != 6) if depth_of[c] > 0.3 * depth_of.max()]
    nonhex = int(live[len(live) // 2])
    assert len({quiet, dying, tail, nonhex, *split}) == 6
    seeds, depths, roles = [], [], []

    def add(role, cell, count, spread, d):
        seeds.append(_around_cell(mesh, cell, count, spread, rng, cells_of))
        depths.append(np.broadcast_to(np.asarray(d, dtype=np.float64), (count,)).copy())
        roles.extend([role] * count)

    add("nonhex", nonhex, 64, 2.0e4, 300.0)
    add("quiet", quiet, 64, 2.0e4, 300.0)
    add("dying", dying, 64, wide_spread, 300.0)
    for c in split:
        mid = np.array([-0.5 * (ztop[c, k] + ztop[c, k + 1]) for k in SPLIT_LAYERS])
        add("split", c, 32, 2.0e4, mid[np.arange(32) % len(mid)])
    add("tail", tail, 30, 2.0e4, 300.0)
    seeds = np.concatenate(seeds)
    return seeds, np.concatenate(depths).astype(np.float32), cells_of(seeds).astype(np.int32), np.array(roles)


def lane_cells(mesh, ref, cells, cells_of):
    """[n, n_steps] the cell each particle starts step s from, taken from the oracle's every-step points (s = 0:
    the seed cell; s > 0: the nearest cell of the point recorded after step s - 1), -1 past its death; and
    [n, n_steps] whether the particle is still in the step loop at step s (it has not died before s)."""
    death = np.asarray(ref["death"])
    pts = ref["points"]                       # [n, K + 1, 3]: the seed, then the point after each step
    n, n_steps = pts.shape[0], pts.shape[1] - 1
    steps = np.arange(n_steps)
    in_loop = (death[:, None] < 0) | (death[:, None] >= steps[None, :])
    at = np.full((n, n_steps), -1, dtype=np.int64)
    at[:, 0] = cells
    past = in_loop[:, 1:]
    at[:, 1:][past] = cells_of(pts[:, 1:n_steps][past])
    return at, in_loop
