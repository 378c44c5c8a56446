"""Per-particle restatement of the random-walk horizontal diffusion (include/mops_traj.h) in
plain Python integers and floats.

TEST INFRASTRUCTURE ONLY (like oracle/ and tests/layer_reference.py): the product never imports this module.
It holds Philox4x32-10, the deviate conversion and the kick, and the engine's three per-particle loops with the kick
inserted after the step's position update and before the record test:

* ``run_layer``          tests/layer_reference.py's loop (streamline / pathline, Euler / RK4 / RK4 with relocation);
* ``run_path``           tests/pathline_attr_reference.py's depth-mode pathline loop (Euler / RK4), without attributes;
* ``run_path_relocate``  tests/rk4_relocate_reference.py's loop with ``relocate=True``.

The helpers are imported from those modules, not copied.  With ``kh = 0`` no kick is applied and each loop is its
original bit for bit (tests/test_diffusion_cpu.py pins that).
"""
import math

import numpy as np

from layer_reference import layer_velocity_at
from pathline_attr_reference import (DBL_MAX, DELTA_T, DURATION, RECORD_T, _clamp, _dmax, _Field, _len, _rk4_mean,
                                     advect_on_sphere, calc_velocity_at, position_after_rotation, rotation_axis,
                                     shared_seeds)
from remap_reference import _div

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 as in Random123: 4 counter words, 2 key words -> 4 output words."""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def deviate(w):
    """((double)(int32_t)w + 0.5) * 2^-31: exact, symmetric, in (-1, 1), never 0."""
    w = int(w) & M32
    return (float(w - (1 << 32) if w & 0x80000000 else w) + 0.5) * 2.0 ** -31


def deviates(seed, gid, step, epoch):
    """(R1, R2) of particle ``gid`` at global step ``step``: key (seed lo, seed hi), counter (gid lo, gid hi, step,
    epoch), output words 0 and 1."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    gid = int(gid) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((gid & M32, gid >> 32, int(step) & M32, int(epoch) & M32), (seed & M32, seed >> 32))
    return deviate(w[0]), deviate(w[1])


def kick_scale(kh, delta_t):
    """s = sqrt(6.0 * Kh * (double)|delta_t|)."""
    return math.sqrt(6.0 * float(kh) * float(abs(int(delta_t))))


def kick(p, s, R1, R2):
    """One kick of position p (the header's statement, expression by expression)."""
    x, y, z = p
    r = _len(p)
    rho = math.sqrt(x * x + y * y)
    if rho > 1e-6:
        ex, ey = _div(-y, rho), _div(x, rho)
    else:
        ex, ey = 1.0, 0.0
    with np.errstate(all="ignore"):  # (r == 0 -- a dead particle re-seeded at the origin by a chain -- gives NaN, as IEEE)
        nx, ny, nz = _div(0.0 - z * ey, r), _div(z * ex, r), _div(x * ey - y * ex, r)
    a, b = R1 * s, R2 * s
    d = (a * ex + b * nx, a * ey + b * ny, b * nz)
    axis = rotation_axis(p, d)
    theta = _div(_len(d), _dmax(1e-12, r))
    return position_after_rotation(p, axis, theta)


def _mesh_tables(mesh):
    C = mesh.nCells
    me = mesh.maxEdges
    coc = (np.asarray(mesh.cellsOnCell).reshape(-1, me).astype(np.int64) - 1).tolist()
    cc = [tuple(r) for r in np.asarray(mesh.cellCoord, dtype=np.float64).reshape(-1, 3).tolist()]

    def nearest(neig, start, q):  # the one-hop walk
        best, cell = DBL_MAX, start
        for cid in neig:
            if cid < 0 or cid >= C:
                continue
            c = cc[cid]
            ln = _len((c[0] - q[0], c[1] - q[1], c[2] - q[2]))
            if ln < best:
                best, cell = ln, cid
        return cell

    return C, coc, nearest


def _run(mesh, front, back, seeds, depths, cells, layer, delta_t, duration, record_t, euler, backward, relocate, kh,
         seed, epoch, ids, id_base):
    """The three loops in one body: ``layer`` None = the depth-mode pathline (pathline_attr_reference.run /
    rk4_relocate_reference.run), else layer_reference.run.  Each line is the original loop's; the kick is the
    only addition."""
    depth_mode = layer is None
    ff = _Field(mesh, front, [])
    fb = None if back is None else _Field(mesh, back, [])
    if depth_mode and fb is None:
        raise ValueError("the depth-mode loop is the pathline's")
    if not depth_mode and not 0 <= int(layer) < mesh.nVertLevels:
        raise ValueError("layer out of range")
    pathline = fb is not None
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    N = seeds.shape[0]
    ids = np.arange(N, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    K = int(duration // record_t)
    n_steps = int(duration // delta_t)
    dt_i = (-1 if backward else 1) * int(delta_t)
    C, coc, nearest = _mesh_tables(mesh)
    nvs = ff.nv
    rec_pos = np.zeros((N, K, 3)); rec_vel = np.zeros((N, K, 3))
    final_pos = seeds.copy()
    final_depth = np.asarray(depths, dtype=np.float32).copy()
    death = np.full(N, -1, dtype=np.int32)
    final_cell = np.asarray(cells, dtype=np.int32).copy()
    kick_changes = np.zeros(N, dtype=np.int64)       # steps whose walk found another cell than it would have
    kick_changes_poly = np.zeros(N, dtype=np.int64)  # without the previous step's kick ... with nv != 6 on a side
    interval = int(record_t // delta_t)
    s = kick_scale(kh, delta_t)
    kicking = float(kh) != 0.0

    def evaluate(p, cell, depth, alpha):
        """(h, w) or None."""
        if depth_mode:
            r = calc_velocity_at(ff, fb, p, cell, depth, alpha)
            return None if r is None else (r[0], r[1])
        h, _ = layer_velocity_at(ff, fb, p, cell, int(layer), alpha)
        return None if h is None else (h, 0.0)

    for pid in range(N):
        p = tuple(float(x) for x in seeds[pid])
        dep32 = np.float32(final_depth[pid])
        first_vel = True
        rec_idx = 0
        run_time = 0
        cell = -1
        neig = []
        unkicked = None  # the position before the previous step's kick
        gid = int(id_base) + int(ids[pid])
        for step in range(n_steps):
            alpha = float(step) / float(n_steps)
            depth = -1.0 * float(dep32)
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
                old = cell
                cell = nearest(neig, old, p)
                if unkicked is not None:
                    other = nearest(neig, old, unkicked)
                    if other != cell:
                        kick_changes[pid] += 1
                        if nvs[other] != 6 or nvs[cell] != 6:
                            kick_changes_poly[pid] += 1
            nvc = nvs[cell]  # GetCellNeighborsIdx: the neighbours, then the cell itself
            neig = coc[cell][:nvc] + [cell]
            r = _len(p)
            if euler:
                ev = evaluate(p, cell, depth, alpha)
                if ev is None:
                    death[pid] = step
                    break
                hvel, vvel = ev
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
                        q = advect_on_sphere(p, stages[-1][0], h)
                        if relocate:
                            sc = nearest(neig, cell, q)
                    ev = evaluate(q, sc, depth, a)
                    if ev is None:
                        dead = True
                        break
                    stages.append(ev)
                if dead:
                    death[pid] = step
                    break
                s1, s2, s3, s4 = stages
                hvel = tuple(_rk4_mean(s1[0][i], s2[0][i], s3[0][i], s4[0][i]) for i in range(3))
                vvel = _rk4_mean(s1[1], s2[1], s3[1], s4[1]) if depth_mode else 0.0
                xt = tuple(p[i] + hvel[i] * dt for i in range(3))
                xl = _len(xt)
                newp = tuple(_div(xt[i], xl) * r for i in range(3)) if xl > 1e-12 else p
            if first_vel:
                first_vel = False
                rec_vel[pid, 0] = hvel
            nd = float(dep32) - vvel * float(dt_i)  # vertical update
            nd = _dmax(0.0, nd)
            r_new = _dmax(1.0, r + vvel * float(dt_i))
            dep32 = np.float32(nd)
            nl = _len(newp)
            if nl > 1e-12:
                newp = tuple(_div(newp[i], nl) * r_new for i in range(3))
            p = newp
            if kicking:  # the kick: after the position update, before the record test
                unkicked = p
                R1, R2 = deviates(seed, gid, step, epoch)
                p = kick(p, s, R1, R2)
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
                final_cell=final_cell, kick_changes=kick_changes, kick_changes_poly=kick_changes_poly)


def run_layer(mesh, front, back, seeds, depths, cells, layer, delta_t, duration, record_t, euler=True, backward=False,
              relocate=False, kh=0.0, seed=0, epoch=0, ids=None, id_base=0):
    """layer_reference.run with the kick (``back`` None = a streamline)."""
    return _run(mesh, front, back, seeds, depths, cells, int(layer), delta_t, duration, record_t, euler, backward,
                relocate, kh, seed, epoch, ids, id_base)


def run_path(mesh, front, back, seeds, depths, cells, delta_t, duration, record_t, euler=True, backward=False, kh=0.0,
             seed=0, epoch=0, ids=None, id_base=0):
    """pathline_attr_reference.run (no attributes) with the kick."""
    return _run(mesh, front, back, seeds, depths, cells, None, delta_t, duration, record_t, euler, backward, False, kh,
                seed, epoch, ids, id_base)


def run_path_relocate(mesh, front, back, seeds, depths, cells, delta_t, duration, record_t, backward=False, kh=0.0,
                      seed=0, epoch=0, ids=None, id_base=0):
    """rk4_relocate_reference.run(relocate=True) with the kick."""
    return _run(mesh, front, back, seeds, depths, cells, None, delta_t, duration, record_t, False, backward, True, kh,
                seed, epoch, ids, id_base)


def run_case(O, mesh, front, back, seeds, depths, layer=None, euler=True, backward=False, relocate=False, kh=0.0,
             seed=0, epoch=0, ids=None, id_base=0, delta_t=DELTA_T, duration=DURATION, record_t=RECORD_T, cells=None):
    """One of the loops with the oracle's 1-NN seed cells (or the given ones); the inputs ride along."""
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    depths = np.asarray(depths, dtype=np.float32)
    if cells is None:
        cells = O.knn(mesh, seeds)
    ref = _run(mesh, front, back, seeds, depths, cells, layer, delta_t, duration, record_t, euler, backward, relocate,
               kh, seed, epoch, ids, id_base)
    ref.update(seeds=seeds, depths=depths, cells=np.asarray(cells), K=int(duration // record_t))
    return ref


def run_shared(O, mesh, front, back, **kw):
    """``run_case`` on the attribute tests' shared 96 seeds over 36 six-hour steps."""
    seeds, depths = shared_seeds()
    return run_case(O, mesh, front, back, seeds, depths, **kw)


def lines(O, ref, pathline=True):
    """The finalized lines of a run through the oracle's own assembly."""
    return O.finalize_lines(ref["seeds"], ref["rec_pos"], ref["rec_vel"], ref["K"], with_attrs=pathline)
