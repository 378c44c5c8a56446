"""Per-particle restatement of the layer step (include/mops_traj.h) in plain Python floats.

TEST INFRASTRUCTURE ONLY (like oracle/ and tests/rk4_relocate_reference.py): the product never imports this module.
A layer run is the reference's StreamLine / PathLine loop (Kernel::StreamLine, MPASOVisualizerKernels.cpp:874-1003;
Kernel::PathLine, :1329-1483) as the oracle's ``run_particle`` states it, with ``calc_velocity_at`` replaced by the
layer evaluation at layer k:

1. the reference's cell guards, ``IsInMesh`` and the Wachspress weights of the cell;
2. ``h_f = sum_v w_v * cellVertexVelocity_front[v*L + k]`` in vertex order (TBBKernel::CalcVelocity); a streamline
   takes ``h = h_f``, a pathline ``h = h_b*alpha + h_f*(1 - alpha)`` with ``h_b`` from the back snapshot;
3. the evaluation fails -- the particle dies at that step -- where ``sqrt((x*x + y*y) + z*z) < 1e-12`` for ``h``;
4. the vertical velocity is 0.0.

Everything else is the loop's own: the one-hop walk, the Euler rotation, the RK4 stages / alphas / mean / chord step,
the two recording rules (pathline: ``(step + 1) % (recordT // deltaT) == 0``; streamline: ``run_time % recordT ==
0``), the step-0 pre-writes, the deaths, the vertical-update lines with ``w = 0``.  ``relocate=True`` locates each of
RK4's stages 2-4 by the step's one-hop walk from the step's cell, as tests/rk4_relocate_reference.py does.

The helpers are imported from pathline_attr_reference / remap_reference, not copied.  tests/test_layer_cpu.py pins
this module to the CPU oracle bit for bit.
"""
import numpy as np

from pathline_attr_reference import (DBL_MAX, DELTA_T, DURATION, MAX_VERTEX_NUM, MAX_VERTICAL_LEVEL_NUM, RECORD_T,
                                     _clamp, _dmax, _Field, _len, _rk4_mean, advect_on_sphere,
                                     position_after_rotation, rotation_axis, shared_seeds)
from remap_reference import _div, is_in_mesh, wachspress

ZERO_NORM = 1e-12


def layer_velocity_at(ff, fb, pos, cell, layer, alpha):
    """The layer evaluation.  (h, False) on success; (None, True) where the zero-velocity rule fails it and
    (None, False) where a guard or IsInMesh does."""
    L = ff.L
    if cell < 0 or L <= 1 or L > MAX_VERTICAL_LEVEL_NUM:
        return None, False
    nv = ff.nv[cell]
    if nv <= 0 or nv > MAX_VERTEX_NUM:
        return None, False
    ids = ff.voc[cell][:nv]
    poly = [ff.vc[v] for v in ids]
    if not is_in_mesh(poly, pos):
        return None, False
    w = wachspress(pos, poly)
    hf = ff.velocity(ids, w, layer)
    if fb is None:
        h = tuple(hf)
    else:
        hb = fb.velocity(ids, w, layer)
        h = tuple(hb[i] * alpha + hf[i] * (1.0 - alpha) for i in range(3))
    if _len(h) < ZERO_NORM:
        return None, True
    return h, False


def run(mesh, front, back, seeds, depths, cells, layer, delta_t, duration, record_t, euler=True, backward=False,
        relocate=False):
    """The layer loop for every seed; ``back`` None = a streamline.  Returns rec_pos / rec_vel [N, K, 3]
    (zero-initialised), final_pos, final_depth (float32), death (-1 = alive, else the step the particle died at),
    final_cell, zero_killed [N] bool (the zero-velocity rule killed it), relocations [N] (stage evaluations whose
    cell differed from the step's cell)."""
    layer = int(layer)
    if not 0 <= layer < mesh.nVertLevels:
        raise ValueError("layer out of range")
    ff = _Field(mesh, front, [])
    fb = None if back is None else _Field(mesh, back, [])
    pathline = fb is not None
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
    final_cell = np.asarray(cells, dtype=np.int32).copy()
    zero_killed = np.zeros(N, dtype=bool)
    reloc = np.zeros(N, dtype=np.int64)
    interval = int(record_t // delta_t)

    def nearest(neig, start, q):  # the one-hop walk (:902-922, :1361-1381)
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
        run_time = 0
        cell = -1
        neig = []

        def fail(step, zero):
            death[pid] = step
            zero_killed[pid] = zero

        for step in range(n_steps):
            alpha = float(step) / float(n_steps)
            run_time += dt_i if pathline else abs(dt_i)
            if step == 0:  # first_loop
                cell = int(cells[pid])
                if cell < 0 or cell >= C:
                    death[pid] = step
                    break
                rec_pos[pid, 0] = p
            else:
                if cell < 0 or cell >= C:
                    death[pid] = step
                    break
                cell = nearest(neig, cell, p)
            nvc = ff.nv[cell]  # GetCellNeighborsIdx: the neighbours, then the cell itself
            neig = coc[cell][:nvc] + [cell]
            r = _len(p)
            if euler:
                hvel, zero = layer_velocity_at(ff, fb, p, cell, layer, alpha)
                if hvel is None:
                    fail(step, zero)
                    break
                axis = rotation_axis(p, hvel)
                speed = _len(hvel)
                theta = (speed * dt_i) / _dmax(1e-12, r)
                newp = position_after_rotation(p, axis, theta)
            else:
                dt = float(dt_i)
                dalpha = dt / float(duration) if pathline else 0.0
                a1 = alpha
                a2 = _clamp(a1 + 0.5 * dalpha, 0.0, 1.0)
                a4 = _clamp(a1 + dalpha, 0.0, 1.0)
                stages = []
                q = p
                dead = False
                for st, (h, a) in enumerate(((0.0, a1), (dt * 0.5, a2), (dt * 0.5, a2), (dt, a4))):
                    sc = cell
                    if st > 0:
                        q = advect_on_sphere(p, stages[-1], h)
                        if relocate:
                            sc = nearest(neig, cell, q)
                            if sc != cell:
                                reloc[pid] += 1
                    s, zero = layer_velocity_at(ff, fb, q, sc, layer, a)
                    if s is None:
                        fail(step, zero)
                        dead = True
                        break
                    stages.append(s)
                if dead:
                    break
                s1, s2, s3, s4 = stages
                hvel = tuple(_rk4_mean(s1[i], s2[i], s3[i], s4[i]) for i in range(3))
                xt = tuple(p[i] + hvel[i] * dt for i in range(3))
                xl = _len(xt)
                newp = tuple(_div(xt[i], xl) * r for i in range(3)) if xl > 1e-12 else p
            vvel = 0.0  # the layer step's vertical velocity; the vertical-update lines stay
            nd = float(dep32) - vvel * float(dt_i)
            nd = _dmax(0.0, nd)
            r_new = _dmax(1.0, r + vvel * float(dt_i))
            dep32 = np.float32(nd)
            nl = _len(newp)
            if nl > 1e-12:
                newp = tuple(_div(newp[i], nl) * r_new for i in range(3))
            if first_vel:
                first_vel = False
                rec_vel[pid, 0] = hvel
            p = newp
            if pathline:
                record = interval > 0 and (step + 1) % interval == 0
            else:
                record = record_t > 0 and run_time % int(record_t) == 0
            if record:
                if rec_idx < K:
                    rec_pos[pid, rec_idx] = p
                    rec_vel[pid, rec_idx] = hvel
                rec_idx += 1
        final_pos[pid] = p
        final_depth[pid] = dep32
        final_cell[pid] = cell
    return dict(rec_pos=rec_pos, rec_vel=rec_vel, final_pos=final_pos, final_depth=final_depth, death=death,
                final_cell=final_cell, zero_killed=zero_killed, relocations=reloc)


def run_case(O, mesh, front, back, seeds, depths, layer, euler=True, backward=False, relocate=False, delta_t=DELTA_T,
             duration=DURATION, record_t=RECORD_T, cells=None):
    """``run`` with the oracle's 1-NN seed cells (or the given ones); the inputs ride along in the result."""
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    depths = np.asarray(depths, dtype=np.float32)
    if cells is None:
        cells = O.knn(mesh, seeds)
    ref = run(mesh, front, back, seeds, depths, cells, layer, delta_t, duration, record_t, euler=euler,
              backward=backward, relocate=relocate)
    ref.update(seeds=seeds, depths=depths, cells=np.asarray(cells), K=int(duration // record_t))
    return ref


def run_shared(O, mesh, front, back, layer, euler=True, backward=False, relocate=False):
    """``run_case`` on the attribute tests' shared 96 seeds over 36 six-hour steps."""
    seeds, depths = shared_seeds()
    return run_case(O, mesh, front, back, seeds, depths, layer, euler=euler, backward=backward, relocate=relocate)


def lines(O, ref, pathline):
    """The finalized lines of a ``run`` result through the oracle's own assembly."""
    return O.finalize_lines(ref["seeds"], ref["rec_pos"], ref["rec_vel"], ref["K"], with_attrs=pathline)
