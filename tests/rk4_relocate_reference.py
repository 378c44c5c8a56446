"""Per-particle restatement of the pathline RK4 loop with a ``relocate`` switch, in plain Python floats.

TEST INFRASTRUCTURE ONLY (like oracle/ and tests/pathline_attr_reference.py): the product never imports this module.
``relocate=False`` is Kernel::PathLine's RK4 (MPASOVisualizerKernels.cpp:1329-1483) as tests/pathline_attr_reference.py
restates it -- tests/test_rk4_relocate_cpu.py pins it to the CPU oracle bit for bit.  ``relocate=True`` is the engine's
MOPS_RK4_RELOCATE (include/mops_traj.h): before ``calc_velocity_at`` each of stages 2, 3 and 4
is located by the step's own one-hop walk (:1361-1381, GetCellNeighborsIdx), always from the step's cell: the argmin of
the Euclidean distance from the stage point over the step cell's neighbours in cellsOnCell order, then the cell itself
(ids outside [0, C) skipped, strict <, first minimum, from DBL_MAX); the stage is evaluated in that cell.  The
particle's own cell is not changed by a stage.  Everything else -- the alphas, the mean, the chord step, the vertical
update, the records, the step-0 pre-writes, the deaths -- is the reference's.

The helpers are imported from pathline_attr_reference, not copied.
"""
import numpy as np

from pathline_attr_reference import (DBL_MAX, DELTA_T, DURATION, RECORD_T, _clamp, _dmax, _Field, _len, _rk4_mean,
                                     advect_on_sphere, calc_velocity_at, shared_seeds)
from remap_reference import _div


def run(mesh, front, back, seeds, depths, cells, delta_t, duration, record_t, backward=False, relocate=False):
    """The pathline RK4 loop for every seed.  Returns rec_pos / rec_vel [N, K, 3] (zero-initialised), final_pos,
    final_depth (float32), death (-1 = alive, else the step the particle died at), cell_changes [N], and
    relocations [N] (stage evaluations whose stage cell differed from the step's cell) with relocations_poly [N]
    (those of them where the step's cell or the stage cell has nv != 6)."""
    ff, fb = _Field(mesh, front, []), _Field(mesh, back, [])
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    N = seeds.shape[0]
    K = int(duration // record_t)
    n_steps = int(duration // delta_t)
    dt_i = (-1 if backward else 1) * int(delta_t)
    C = mesh.nCells
    me = mesh.maxEdges
    coc = (np.asarray(mesh.cellsOnCell).reshape(-1, me).astype(np.int64) - 1).tolist()
    cc = [tuple(r) for r in np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3).tolist()]
    rec_pos = np.zeros((N, K, 3)); rec_vel = np.zeros((N, K, 3))
    final_pos = seeds.copy()
    final_depth = np.asarray(depths, dtype=np.float32).copy()
    death = np.full(N, -1, dtype=np.int32)
    changes = np.zeros(N, dtype=np.int64)
    reloc = np.zeros(N, dtype=np.int64)
    reloc_poly = np.zeros(N, dtype=np.int64)
    interval = int(record_t // delta_t)

    def nearest(neig, start, q):  # the one-hop walk (:1361-1381)
        best, cell = DBL_MAX, start
        for cid in neig:
            if cid < 0 or cid >= C:
                continue
            c = cc[cid]
            ln = _len((c[0] - q[0], c[1] - q[1], c[2] - q[2]))
            if ln < best:
                best, cell = ln, cid
        return cell

    for pid in range(N):
        p = tuple(float(x) for x in seeds[pid])
        dep32 = np.float32(final_depth[pid])
        first_vel = True
        rec_idx = 0
        cell = -1
        neig = []

        def stage_cell(q):
            if not relocate:
                return cell
            sc = nearest(neig, cell, q)
            if sc != cell:
                reloc[pid] += 1
                if ff.nv[cell] != 6 or ff.nv[sc] != 6:
                    reloc_poly[pid] += 1
            return sc

        for step in range(n_steps):
            alpha = float(step) / float(n_steps)
            depth = -1.0 * float(dep32)
            if step == 0:  # first_loop (:1351-1360)
                cell = int(cells[pid])
                if cell < 0 or cell >= C:
                    death[pid] = step
                    break
                rec_pos[pid, 0] = p
            else:  # one-hop walk (:1361-1381)
                if cell < 0 or cell >= C:
                    death[pid] = step
                    break
                old = cell
                cell = nearest(neig, cell, p)
                if cell != old:
                    changes[pid] += 1
            nvc = ff.nv[cell]  # GetCellNeighborsIdx (TBBKernel.h:74-101): the neighbours, then the cell itself
            neig = coc[cell][:nvc] + [cell]
            r = _len(p)
            dt = float(dt_i)
            dalpha = dt / float(duration)
            a1 = alpha
            s1 = calc_velocity_at(ff, fb, p, cell, depth, a1)
            s2 = s3 = s4 = None
            if s1 is not None:
                p2 = advect_on_sphere(p, s1[0], dt * 0.5)
                a2 = _clamp(a1 + 0.5 * dalpha, 0.0, 1.0)
                s2 = calc_velocity_at(ff, fb, p2, stage_cell(p2), depth, a2)
            if s2 is not None:
                p3 = advect_on_sphere(p, s2[0], dt * 0.5)
                a3 = _clamp(a1 + 0.5 * dalpha, 0.0, 1.0)
                s3 = calc_velocity_at(ff, fb, p3, stage_cell(p3), depth, a3)
            if s3 is not None:
                p4 = advect_on_sphere(p, s3[0], dt)
                a4 = _clamp(a1 + dalpha, 0.0, 1.0)
                s4 = calc_velocity_at(ff, fb, p4, stage_cell(p4), depth, a4)
            if s4 is None:
                death[pid] = step
                break
            hvel = tuple(_rk4_mean(s1[0][i], s2[0][i], s3[0][i], s4[0][i]) for i in range(3))
            vvel = _rk4_mean(s1[1], s2[1], s3[1], s4[1])
            xt = tuple(p[i] + hvel[i] * dt for i in range(3))
            xl = _len(xt)
            newp = tuple(_div(xt[i], xl) * r for i in range(3)) if xl > 1e-12 else p
            if first_vel:
                first_vel = False
                rec_vel[pid, 0] = hvel
            nd = float(dep32) - vvel * float(dt_i)  # vertical update (:1458-1467)
            nd = _dmax(0.0, nd)
            r_new = _dmax(1.0, r + vvel * float(dt_i))
            dep32 = np.float32(nd)
            nl = _len(newp)
            if nl > 1e-12:
                newp = tuple(_div(newp[i], nl) * r_new for i in range(3))
            p = newp
            if interval > 0 and (step + 1) % interval == 0:  # :1470-1481
                if rec_idx < K:
                    rec_pos[pid, rec_idx] = p
                    rec_vel[pid, rec_idx] = hvel
                rec_idx += 1
        final_pos[pid] = p
        final_depth[pid] = dep32
    return dict(rec_pos=rec_pos, rec_vel=rec_vel, final_pos=final_pos, final_depth=final_depth, death=death,
                cell_changes=changes, relocations=reloc, relocations_poly=reloc_poly)


def run_case(O, mesh, front, back, seeds, depths, backward=False, relocate=True, delta_t=DELTA_T, duration=DURATION,
             record_t=RECORD_T, cells=None):
    """``run`` with the oracle's 1-NN seed cells (or the given ones); the inputs ride along in the result."""
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    depths = np.asarray(depths, dtype=np.float32)
    if cells is None:
        cells = O.knn(mesh, seeds)
    ref = run(mesh, front, back, seeds, depths, cells, delta_t, duration, record_t, backward=backward,
              relocate=relocate)
    ref.update(seeds=seeds, depths=depths, cells=np.asarray(cells), K=int(duration // record_t))
    return ref


def run_shared(O, mesh, front, back, backward=False, relocate=True):
    """``run_case`` on the attribute tests' shared 96 seeds over 36 six-hour steps."""
    seeds, depths = shared_seeds()
    return run_case(O, mesh, front, back, seeds, depths, backward=backward, relocate=relocate)


# ---- the further cases of the relocation tests ---------------------------------------------------------------
PENTAGON_RADIUS = 6371010.0
PENTAGON_DEPTH = 200.0
TWO_HOP_DELTA_T = 864000
TWO_HOP_STEPS = 12
TWO_HOP_RECORD_EVERY = 3


def pentagon_seeds(mesh):
    """Seeds at the centres of the mesh's pentagons and of their neighbours, scaled to PENTAGON_RADIUS; depths
    PENTAGON_DEPTH.  (seeds [M, 3], depths [M] float32, pentagon cell ids)."""
    nv = np.asarray(mesh.nEdgesOnCell).reshape(-1).astype(np.int64)
    me = mesh.maxEdges
    coc = np.asarray(mesh.cellsOnCell).reshape(-1, me).astype(np.int64) - 1
    cc = np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3)
    pent = np.flatnonzero(nv == 5)
    ids = []
    for c in pent:
        ids.append(int(c))
        ids.extend(int(q) for q in coc[c, :nv[c]] if 0 <= q < mesh.nCells)
    p = cc[np.asarray(ids, dtype=np.int64)]
    seeds = p / np.linalg.norm(p, axis=1, keepdims=True) * PENTAGON_RADIUS
    return seeds, np.full(len(ids), PENTAGON_DEPTH, dtype=np.float32), pent


def lines(O, ref):
    """The finalized lines of a ``run`` result through the oracle's own assembly (as the attribute tests)."""
    return O.finalize_lines(ref["seeds"], ref["rec_pos"], ref["rec_vel"], ref["K"], with_attrs=True)
